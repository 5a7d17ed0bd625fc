/* zxc_rangesv_shuffle.h — the rules of zxc_mi355x_decompress_rangesv_shuffle_device on top of zxc_rangesv.h and zxc_shuffle.h:
 * ranges of the PLAIN bytes of an archive that holds byte-shuffled blocks (unit = the block size), each into a destination of its
 * own. The transform keeps sizes and every unit is one block, so plain bytes [offset, offset + len) lie in the blocks the same
 * shuffled bytes lie in: the request (zrv_req), the index, the early verdict, the jobs per range and the slots are rangesv's as
 * they are. What the planes change are two arguments of the family's rules (zxc_ranges.h) and the record: no block can be decoded
 * in place (zrs_job: zr_req_job with may_direct 0), a block's planes are laid out by its length, so the block verdict holds the status against
 * the length the index gives the block (zrs_verdict, zrs_block_verdict: exact 1), and the copy-out becomes a gather across the
 * E planes of a slot, which is what this file has. Plain inline C that hipcc and a host C compiler both take, so that the kernels
 * of zxc_rangesv_shuffle_device.hip and the CPU tests (tests/ranges/rangesv_shuffle_replay.h) run the same lines.
 *
 * The gather plan. A job wants plain bytes [from, from + n) of a block of m bytes, counted from the block's first byte. With
 * q = m / E and Gq = q / 16, whole group g < Gq of the block is plain bytes [16 E g, 16 E (g + 1)) and 16 bytes at
 * slot + k q + 16 g in each plane k (zxc_shuffle.h). A wanted byte p is a VECTOR byte exactly when p < 16 E Gq and its whole group
 * lies inside [from, from + n): a lane moves such a group with E 16-byte loads, zsh_regs_unshuffle and E 16-byte stores. Every
 * other wanted byte is a SINGLE byte, read from slot[(p % E) q + p / E] when p < q E, else from slot[p] (zsh_index inside the
 * block): the two edge groups, the elements behind the last whole group of a ragged block, and its m % E copied bytes, at most
 * 2 (16 E - 1) + 127 per job. An item is (job, chunk): chunk c owns the wanted bytes with p / 8192 == c. 8192 is a multiple of
 * 16 E, so a group never straddles two chunks: every wanted byte has exactly one owner and is written exactly once. */
#ifndef ZXC_RANGESV_SHUFFLE_H
#define ZXC_RANGESV_SHUFFLE_H
#include "../../include/zxc_mi355x_rangesv_shuffle.h"
#include "zxc_rangesv.h"
#include "zxc_shuffle.h"

#define ZRS_CHUNK 8192u   /* plain bytes of a block one wavefront of the gather owns */
#define ZRS_JOB_BYTES 52u /* work area per job besides its slot: zxc_dev_job_t + status + zrs_gather_t */

/* A job's gather: the un-shuffle of slot[0, m) restricted to plain bytes [from, from + n) -> d_out + dst_at, when the block
 * decoded to exactly m bytes. n == 0: nothing to move (an empty job). zr_copy_t's fields and the block's length from the index. */
typedef struct zrs_gather {
    uint64_t dst_at;
    uint32_t from, n, m, rsv;
} zrs_gather_t;

/* Job j of range r (job_index = r J + j): rangesv's job without the direct rule. Every covered block is staged in its slot; the
 * record names what of its plain bytes goes where (dst_at counted from out_base modulo 2^64) and the block's length. */
ZC_FN void zrs_job(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                   uint32_t block_size, uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job,
                   zrs_gather_t* ga) {
    zr_part_t p;
    zr_req_job(index, zrv_req(r, max_len, out_base), j, job_index, src_size, block_size, stage_rel, 0, have_dict, have_id, job, &p);
    ga->dst_at = p.dst_at; ga->from = p.from; ga->n = p.n; ga->rsv = 0;
    ga->m = p.n ? zr_block_len((const zr_index_t*)index, p.b, block_size) : 0;
}
/* the block rule and the verdict with exact statuses: the block must have decoded to the length its planes were laid out by */
ZC_FN int32_t zrs_block_verdict(int32_t status, uint32_t m) { return zr_block_rule(status, m, 1); }
ZC_FN int64_t zrs_verdict(const void* index, zxc_dev_rangev_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                          uint32_t block_size, int have_dict, uint32_t have_id) {
    return zr_req_verdict(index, zrv_req(r, max_len, 0u), J, status, src_size, block_size, 1, have_dict, have_id);
}

/* ---- the gather plan (E: 2, 4 or 8; from + n <= m <= 2 MiB) */
/* the definition: wanted byte p of [from, from + n) moves with its whole group */
ZC_FN int zrs_vector_byte(uint32_t p, uint32_t from, uint32_t n, uint32_t m, uint32_t E) {
    const uint32_t w = ZSH_GROUP * E, g = p / w;
    return g < m / E / ZSH_GROUP && g * w >= from && (g + 1u) * w <= from + n;
}
/* where plain byte p of a block of m bytes lies in its slot */
ZC_FN uint32_t zrs_src(uint32_t p, uint32_t m, uint32_t E) {
    const uint32_t q = m / E;
    return p < q * E ? (p % E) * q + p / E : p;
}
/* What item (job, chunk c) moves: the whole groups [g_lo, g_hi) and the single bytes [head_at, head_at + head_n) in front of them
 * and [tail_at, tail_at + tail_n) behind them (without a whole group: everything it owns is the head). -> 0: it owns nothing. */
typedef struct zrs_item { uint32_t g_lo, g_hi, head_at, head_n, tail_at, tail_n; } zrs_item_t;
ZC_FN int zrs_item(uint32_t from, uint32_t n, uint32_t m, uint32_t E, uint32_t c, zrs_item_t* it) {
    const uint32_t w = ZSH_GROUP * E, end = from + n, c_lo = c * ZRS_CHUNK, c_hi = c_lo + ZRS_CHUNK;
    const uint32_t lo = from > c_lo ? from : c_lo, hi = end < c_hi ? end : c_hi, Gq = m / E / ZSH_GROUP;
    if (hi <= lo) return 0;
    it->g_lo = (lo + w - 1u) / w;
    it->g_hi = hi / w < Gq ? hi / w : Gq;
    it->head_at = lo;
    if (it->g_hi <= it->g_lo) {
        it->g_hi = it->g_lo;
        it->head_n = hi - lo; it->tail_at = hi; it->tail_n = 0;
    } else {
        it->head_n = it->g_lo * w - lo; it->tail_at = it->g_hi * w; it->tail_n = hi - it->tail_at;
    }
    return 1;
}
/* single byte k < head_n + tail_n of an item: its place in the block's plain bytes */
ZC_FN uint32_t zrs_single(const zrs_item_t* it, uint32_t k) { return k < it->head_n ? it->head_at + k : it->tail_at + (k - it->head_n); }

/* ---- the call's shape: rangesv's jobs and slots, a gather record per job in the copy record's place, ZRS_CHUNK chunks per job */
typedef zr_shape_t zrs_shape_t;
ZC_FN int zrs_shape(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, zrs_shape_t* s) {
    return zr_shape_of(n_ranges, max_len, block_size, sizeof(zrs_gather_t), (block_size + ZRS_CHUNK - 1u) / ZRS_CHUNK, s);
}
#endif
