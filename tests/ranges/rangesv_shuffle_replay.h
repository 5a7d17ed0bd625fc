/* Test-only: zxc_mi355x_decompress_rangesv_shuffle_device replayed on the host, stage by stage as the entry point of
 * zxc_rangesv_shuffle_device.hip enqueues them, over the rule functions the kernels call (zxc_amd/csrc/zxc_rangesv_shuffle.h on top
 * of zxc_ranges.h). The stages are the frame of rangesv_replay.h (rvr_stages: plan, the stand-in decode, verdict) with this front
 * end: no block decoded in place, so block b's SHUFFLED bytes (what the archive holds) always go to its slot; exact statuses; and
 *   gather   the gather kernels' arithmetic for every (job, chunk, lane): per whole group E 16-byte loads from the planes,
 *            zsh_regs_unshuffle and E 16-byte stores; the single bytes one at a time
 * The work area is the caller's, of exactly the shape's size, and the destinations are the caller's host addresses above or below
 * it, so that a sanitizer sees every byte written outside either. d_out is the work area's 256-byte aligned base and every address
 * is that base plus a 64-bit offset modulo 2^64, computed in integers as the kernels' pointer arithmetic comes out. Every store
 * into a destination goes through RSR_HIT(address, bytes), which the includer may define to count the writes. */
#ifndef RANGESV_SHUFFLE_REPLAY_H
#define RANGESV_SHUFFLE_REPLAY_H
#include "../../zxc_amd/csrc/zxc_rangesv_shuffle.h"
#include "rangesv_replay.h" /* rvr_blocks_t, rvr_at, RVR_BAD_PLAN, rvr_stages */

#ifndef RSR_HIT
#define RSR_HIT(addr, n) ((void)0)
#endif

static inline void rsr_put(uint64_t out_base, uint64_t off, const void* v, uint32_t n) {
    memcpy(rvr_at(out_base, off), v, n);
    RSR_HIT(out_base + off, n);
}

/* the gather of job i, as the wavefronts of zxc_rangesv_shuffle_gather{2,4,8}_kernel make it with out = d_out */
static inline void rsr_gather_job(const uint8_t* stage, uint32_t slot_stride, const void* gathers, const int32_t* status, uint32_t i,
                                  uint32_t chunks, uint32_t E, uint64_t out_base) {
    const zrs_gather_t ga = ((const zrs_gather_t*)gathers)[i];
    for (uint32_t c = 0; c < chunks; c++) {
        zrs_item_t item;
        if (ga.n == 0 || !zrs_item(ga.from, ga.n, ga.m, E, c, &item)) continue;
        if (zrs_block_verdict(status[i], ga.m) != 0) continue;
        const uint8_t* s = stage + (uint64_t)i * slot_stride;
        const uint32_t q = ga.m / E;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            for (uint32_t turn = 0; turn < 8u / E; turn++) {
                const uint32_t g = item.g_lo + turn * 64u + lane;
                uint32_t e[32], p[32];
                if (g >= item.g_hi) continue;
                for (uint32_t k = 0; k < E; k++) memcpy(p + 4u * k, s + (uint64_t)k * q + 16u * g, 16);
                zsh_regs_unshuffle(p, e, E);
                for (uint32_t j = 0; j < E; j++) rsr_put(out_base, ga.dst_at + (g * (ZSH_GROUP * E) - ga.from) + 16u * j, e + 4u * j, 16);
            }
            for (uint32_t k = lane; k < item.head_n + item.tail_n; k += 64u) {
                const uint32_t at = zrs_single(&item, k);
                rsr_put(out_base, ga.dst_at + (at - ga.from), s + zrs_src(at, ga.m, E), 1);
            }
        }
    }
}

static inline void rsr_job(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t i, uint64_t src_size, uint64_t max_len, uint32_t bs,
                           uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job, void* recs) {
    zrs_job(index, r, j, i, src_size, max_len, bs, out_base, stage_rel, have_dict, have_id, job, (zrs_gather_t*)recs + i);
}
/* The whole call. work: the shape's bytes, of any alignment. -> ZXC_OK, a synchronous error of the entry point's argument checks
 * (the NULL checks excepted), or RVR_BAD_PLAN. */
static inline int rsr_call(uint64_t src_size, const void* index, const zxc_dev_rangev_t* ranges, uint32_t n_ranges, uint64_t max_len,
                           uint32_t E, uint32_t bs, int have_dict, uint32_t have_id, const rvr_blocks_t* blk, uint8_t* work,
                           uint64_t work_size, int64_t* results) {
    zr_shape_t s;
    if (!zsh_elem_ok(E)) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int shape_rc = zrs_shape(n_ranges, max_len, bs, &s);
    if (shape_rc != 0) return shape_rc;
    if (work_size < s.bytes) return ZXC_ERROR_MEMORY;
    if (n_ranges == 0) return ZXC_OK;
    return rvr_stages(0, rsr_job, zrs_verdict, rsr_gather_job, E, src_size, index, ranges, n_ranges, max_len, bs, have_dict, have_id, blk, &s, work, results);
}
#endif
