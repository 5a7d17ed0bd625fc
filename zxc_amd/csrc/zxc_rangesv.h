/* zxc_rangesv.h — the rules of zxc_mi355x_decompress_rangesv_device on top of zxc_ranges.h: ranges whose destinations are absolute
 * device addresses of any alignment (zxc_dev_rangev_t) instead of offsets into one aligned buffer. What is new is what the address
 * changes: the early verdict (no capacity; a wrapping or zero base), the direct rule (the block's own address decides the
 * alignment, the range's own destination bounds the decoders' spill), job (r, j) with its copy record, and the final verdict. The
 * index, zr_wanted, zr_block_verdict and zr_shape are the sibling's as they are. Plain inline C that hipcc and a host C compiler
 * both take, so that the kernels of zxc_ranges_device.hip and the CPU tests run the same lines.
 *
 * Addresses are counted from one base, the decode launch's d_out (the work area's 256-byte aligned base), modulo 2^64: a
 * destination may lie above or below the work area, and the decode and copy kernels only ever add such an offset to that base in
 * 64 bits (the convention of takev, zxc_take_device.hip). The base is a multiple of 16, so an offset has its address's alignment. */
#ifndef ZXC_RANGESV_H
#define ZXC_RANGESV_H
#include "../../include/zxc_mi355x_rangesv.h"
#include "zxc_ranges.h"

/* the archive side of a range, as the sibling's functions take it (its destination is counted from its own base: dst_off 0) */
ZC_FN zxc_dev_range_t zrv_range(zxc_dev_rangev_t r) {
    zxc_dev_range_t s;
    s.offset = r.offset; s.len = r.len; s.dst_off = 0;
    return s;
}
/* What is decided before any block is looked at: -> 1 and *result when the range is answered already, 0 when its blocks decide.
 * The sibling's order with the destination checks restated: there is no capacity, so DST_TOO_SMALL is len > max_len or an end
 * base + len that reaches 2^64 (behind it every address of the range is below 2^64 and no sum below wraps); a zero base with a
 * length is zav_entry_flags' ZXC_ERROR_NULL_INPUT (zxc_appendv.h), refused and never dereferenced. Then zr_range_final_dict for
 * the same (offset, len) and a destination of exactly len bytes, whose first four checks have passed by now. */
ZC_FN int zrv_range_final(const zr_index_t* ix, zxc_dev_rangev_t r, uint64_t src_size, uint64_t max_len, uint32_t block_size,
                          int have_dict, uint32_t have_id, int64_t* result) {
    if (r.len == 0) { *result = 0; return 1; }
    if (ix->status < 0) { *result = ix->status; return 1; }
    if (ix->block_size != block_size) { *result = ZXC_ERROR_BAD_BLOCK_SIZE; return 1; }
    if (r.len > max_len || r.len > ~r.base) { *result = ZXC_ERROR_DST_TOO_SMALL; return 1; }
    if (r.base == 0) { *result = ZXC_ERROR_NULL_INPUT; return 1; }
    return zr_range_final_dict(ix, zrv_range(r), src_size, max_len, r.len, block_size, have_dict, have_id, result);
}
/* Block b of a valid range decodes straight to its place base + b bs - offset: all of it is wanted, the place is 16-byte aligned,
 * and the block plus the 32 bytes the decoders may store behind it end inside [base, base + len): place + bs + 32 <= base + len is
 * b bs + bs + 32 <= offset + len. Nothing is promised writable behind a range, so a range's last whole block is staged unless 32
 * more bytes of the range follow it. */
ZC_FN int zrv_direct(zxc_dev_rangev_t r, uint64_t b, uint32_t block_size) {
    const uint64_t lo = b * block_size;
    if (lo < r.offset || lo + block_size + 32u > r.offset + r.len) return 0;
    return ((r.base + (lo - r.offset)) & 15u) == 0;
}
/* Job j of range r (job_index = r J + j), as zr_job_dict: block offset / bs + j while the range reaches it, else an empty job
 * (comp_size 0: the decoder answers with an error status and touches nothing). out_base: the launch's d_out as a number;
 * stage_rel: the staged slots counted from it. A direct job's out_off is its place minus out_base; a staged job's copy record
 * names slot[from, from + n) -> out_base + dst_at, dst_at the wanted part's address minus out_base (both modulo 2^64). */
ZC_FN void zrv_job(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                   uint32_t block_size, uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job,
                   zr_copy_t* cp) {
    const zr_index_t* ix = (const zr_index_t*)index;
    const uint64_t* offs = zr_coffsets(index);
    int64_t res;
    uint32_t from, to;
    job->comp_off = 0; job->out_off = stage_rel + job_index * ((uint64_t)block_size + ZR_SLOT_PAD); job->comp_size = 0; job->out_len = block_size;
    cp->dst_at = 0; cp->from = 0; cp->n = 0;
    if (zrv_range_final(ix, r, src_size, max_len, block_size, have_dict, have_id, &res)) return;
    const uint64_t b = r.offset / block_size + j;
    zr_wanted(zrv_range(r), b, block_size, &from, &to);
    if (to == from) return;
    job->comp_off = offs[b];
    job->comp_size = (uint32_t)(offs[b + 1u] - offs[b]);
    const uint64_t at = r.base + (b * block_size + from - r.offset) - out_base;
    if (zrv_direct(r, b, block_size)) job->out_off = at;
    else { cp->dst_at = at; cp->from = from; cp->n = to - from; }
}
/* The range's result from its J statuses: the first failing covered block in block order, else len (zr_verdict_dict). */
ZC_FN int64_t zrv_verdict(const void* index, zxc_dev_rangev_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                          uint32_t block_size, int have_dict, uint32_t have_id) {
    int64_t res;
    if (zrv_range_final((const zr_index_t*)index, r, src_size, max_len, block_size, have_dict, have_id, &res)) return res;
    return zr_verdict_dict(index, zrv_range(r), J, status, src_size, max_len, r.len, block_size, have_dict, have_id);
}
#endif
