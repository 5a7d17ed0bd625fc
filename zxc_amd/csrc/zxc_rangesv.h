/* zxc_rangesv.h — what zxc_mi355x_decompress_rangesv_device adds to the rules of zxc_ranges.h: ranges whose destinations are
 * absolute device addresses of any alignment (zxc_dev_rangev_t) instead of offsets into one aligned buffer. That is a request
 * builder, and the front end's four functions as thin calls of the family's rules over it: the early verdict, the direct rule
 * (the block's own address decides the alignment, the range's own destination bounds the decoders' spill), job (r, j) with its
 * copy record, and the verdict; the shape is the sibling's. Plain inline C that hipcc and a host C compiler both take.
 *
 * Addresses are counted from one base, the decode launch's d_out (the work area's 256-byte aligned base), modulo 2^64: a
 * destination may lie above or below the work area, and the decode and copy kernels only ever add such an offset to that base in
 * 64 bits (the convention of takev, zxc_take_device.hip). The base is a multiple of 16, so an offset has its address's alignment. */
#ifndef ZXC_RANGESV_H
#define ZXC_RANGESV_H
#include "../../include/zxc_mi355x_rangesv.h"
#include "zxc_ranges.h"

/* out_base: the launch's d_out as a number. The destination checks restated: there is no capacity, so DST_TOO_SMALL is
 * len > max_len or an end base + len that reaches 2^64 (behind it every address of the range is below 2^64 and no sum wraps); a
 * zero base with a length is zav_entry_flags' ZXC_ERROR_NULL_INPUT (zxc_appendv.h), refused and never dereferenced. */
ZC_FN zr_req_t zrv_req(zxc_dev_rangev_t r, uint64_t max_len, uint64_t out_base) {
    zr_req_t q;
    q.offset = r.offset; q.len = r.len; q.place = r.base - out_base;
    q.dst_err = (r.len > max_len || r.len > ~r.base) ? ZXC_ERROR_DST_TOO_SMALL : r.base == 0 ? ZXC_ERROR_NULL_INPUT : 0;
    return q;
}
/* The rangesv front end under the names its kernels and the CPU tests call: the early verdict, the direct rule on the address itself
 * (out_base is a multiple of 16), job (r, j) with its copy record counted from out_base, and the verdict. */
ZC_FN int zrv_range_final(const zr_index_t* ix, zxc_dev_rangev_t r, uint64_t src_size, uint64_t max_len, uint32_t block_size,
                          int have_dict, uint32_t have_id, int64_t* result) {
    return zr_req_final(ix, zrv_req(r, max_len, 0u), src_size, block_size, have_dict, have_id, result);
}
ZC_FN int zrv_direct(zxc_dev_rangev_t r, uint64_t b, uint32_t block_size) { return zr_req_direct(zrv_req(r, r.len, 0u), b, block_size); }
ZC_FN void zrv_job(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                   uint32_t block_size, uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job,
                   zr_copy_t* cp) {
    zr_part_t p;
    zr_req_job(index, zrv_req(r, max_len, out_base), j, job_index, src_size, block_size, stage_rel, 1, have_dict, have_id, job, &p);
    *cp = zr_copy_of(p, 0u);
}
ZC_FN int64_t zrv_verdict(const void* index, zxc_dev_rangev_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                          uint32_t block_size, int have_dict, uint32_t have_id) {
    return zr_req_verdict(index, zrv_req(r, max_len, 0u), J, status, src_size, block_size, 0, have_dict, have_id);
}
#endif
