/* Test-only: zxc_mi355x_decompress_rangesv_device replayed on the host, stage by stage as rangesv_call of zxc_ranges_device.hip
 * enqueues them, over the rule functions the kernels call (zxc_amd/csrc/zxc_rangesv.h on top of zxc_ranges.h):
 *   plan     zrv_job for every job (r, j) into the work area's job and copy tables
 *   decode   a stand-in for the decode launch: block b's expected bytes go to d_out + out_off, 32 more bytes are scribbled behind
 *            them (what the decoders may store), a failing block leaves junk in the front half of its slot, an empty job (comp_size
 *            0) is answered with an error and touches nothing
 *   copy     zxc_ranges_copy_kernel's arithmetic for every (job, chunk, lane, unit): aligned 16-byte stores, bytes at the two ends
 *   verdict  zrv_verdict for every range
 * The work area is one heap block of exactly zr_shape's size and the destinations are the caller's host addresses, so that a
 * sanitizer sees every byte written outside either. d_out is the work area's 256-byte aligned base and every address is that base
 * plus a 64-bit offset modulo 2^64, computed in integers as the kernels' pointer arithmetic comes out. */
#ifndef RANGESV_REPLAY_H
#define RANGESV_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_rangesv.h"

#define RVR_BAD_PLAN (-1000) /* the replay's own checks failed: a job that names no block of the index, a place that is not 16-byte aligned */

typedef struct rvr_blocks { /* what a decoder answers: block b decodes to status[b] bytes at bytes + at[b], or fails with status[b] < 0 */
    const uint8_t* bytes;
    const uint64_t* at;
    const int32_t* status;
    uint32_t n;
} rvr_blocks_t;

static inline uint8_t* rvr_at(uint64_t out_base, uint64_t off) { return (uint8_t*)(uintptr_t)(out_base + off); }

/* the copy-out of job i, as the wavefronts of zxc_ranges_copy_kernel make it with dst = d_out */
static inline void rvr_copy_job(const uint8_t* stage, uint32_t slot_stride, const zr_copy_t* copies, const int32_t* status, uint32_t i,
                                uint32_t chunks, uint64_t out_base) {
    const zr_copy_t cp = copies[i];
    for (uint32_t k = 0; k < chunks; k++) {
        if (cp.n == 0 || (uint64_t)k * ZR_COPY_CHUNK >= (cp.dst_at & 15u) + cp.n) continue;
        const int32_t st = status[i];
        if (st < 0 || (uint32_t)st < cp.from + cp.n) continue;
        const uint8_t* s = stage + (uint64_t)i * slot_stride + cp.from;
        const int64_t n = (int64_t)cp.n;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            int64_t rel = (int64_t)k * ZR_COPY_CHUNK - (int64_t)(cp.dst_at & 15u) + 16 * (int64_t)lane;
            for (uint32_t u = 0; u < ZR_COPY_CHUNK / 1024u; u++, rel += 1024) {
                if (rel >= n) break;
                if (rel >= 0 && rel + 16 <= n) {
                    memcpy(rvr_at(out_base, cp.dst_at + (uint64_t)rel), s + rel, 16);
                } else {
                    const int64_t lo = rel < 0 ? 0 : rel, hi = rel + 16 < n ? rel + 16 : n;
                    for (int64_t b = lo; b < hi; b++) *rvr_at(out_base, cp.dst_at + (uint64_t)b) = s[b];
                }
            }
        }
    }
}

/* The whole call. -> ZXC_OK, a synchronous error of the entry point's argument checks, or RVR_BAD_PLAN. */
static inline int rvr_call(uint64_t src_size, const void* index, const zxc_dev_rangev_t* ranges, uint32_t n_ranges, uint64_t max_len,
                           uint32_t bs, int have_dict, uint32_t have_id, const rvr_blocks_t* blk, int64_t* results) {
    zr_shape_t s;
    const int shape_rc = zr_shape(n_ranges, max_len, bs, &s);
    if (shape_rc != 0) return shape_rc;
    if (n_ranges == 0) return ZXC_OK;
    uint8_t* work = malloc(s.bytes);
    const uint64_t out_base = zc_round_up((uint64_t)(uintptr_t)work, 256u);
    uint8_t* base = work + (out_base - (uint64_t)(uintptr_t)work);
    zxc_dev_job_t* jobs = (zxc_dev_job_t*)(base + s.o_jobs);
    int32_t* status = (int32_t*)(base + s.o_status);
    zr_copy_t* copies = (zr_copy_t*)(base + s.o_copy);
    const uint64_t* offs = zr_coffsets(index);
    int rc = ZXC_OK;

    for (uint32_t i = 0; i < s.n_jobs; i++)
        zrv_job(index, ranges[i / s.J], i % s.J, i, src_size, max_len, bs, out_base, s.o_stage, have_dict, have_id, &jobs[i], &copies[i]);

    for (uint32_t i = 0; i < s.n_jobs && rc == ZXC_OK; i++) {
        status[i] = ZXC_ERROR_SRC_TOO_SMALL;
        if (jobs[i].comp_size == 0) continue;
        const uint64_t b = ranges[i / s.J].offset / bs + i % s.J;
        if (b >= blk->n || offs[b] != jobs[i].comp_off || offs[b + 1u] - offs[b] != jobs[i].comp_size || jobs[i].out_len != bs ||
            (jobs[i].out_off & 15u)) { rc = RVR_BAD_PLAN; break; }
        uint8_t* out = rvr_at(out_base, jobs[i].out_off);
        status[i] = blk->status[b];
        if (status[i] < 0) { memset(out, 0x5A, bs / 2u); continue; }
        const uint32_t n = (uint32_t)status[i] < bs ? (uint32_t)status[i] : bs;
        memcpy(out, blk->bytes + blk->at[b], n);
        memset(out + n, 0xA5, 32);
    }
    if (rc == ZXC_OK) {
        for (uint32_t i = 0; i < s.n_jobs; i++) rvr_copy_job(base + s.o_stage, s.slot_stride, copies, status, i, s.copy_chunks, out_base);
        for (uint32_t r = 0; r < n_ranges; r++)
            results[r] = zrv_verdict(index, ranges[r], s.J, status + (uint64_t)r * s.J, src_size, max_len, bs, have_dict, have_id);
    }
    free(work);
    return rc;
}
#endif
