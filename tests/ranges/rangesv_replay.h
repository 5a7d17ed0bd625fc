/* Test-only: zxc_mi355x_decompress_rangesv_device replayed on the host, stage by stage as rangesv_call of zxc_ranges_device.hip
 * enqueues them, over the rule functions the kernels call (zxc_amd/csrc/zxc_rangesv.h on top of zxc_ranges.h), and the frame of
 * those stages (rvr_stages) that the replay of the shuffled ranges (rangesv_shuffle_replay.h) runs with its own front end:
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
static inline void rvr_copy_job(const uint8_t* stage, uint32_t slot_stride, const void* copies, const int32_t* status, uint32_t i,
                                uint32_t chunks, uint32_t E, uint64_t out_base) {
    const zr_copy_t cp = ((const zr_copy_t*)copies)[i];
    (void)E;
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

typedef void (*rvr_job_fn)(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t i, uint64_t src_size, uint64_t max_len, uint32_t bs,
                           uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job, void* recs);
typedef int64_t (*rvr_verdict_fn)(const void* index, zxc_dev_rangev_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                                  uint32_t bs, int have_dict, uint32_t have_id);
typedef void (*rvr_out_fn)(const uint8_t* stage, uint32_t slot_stride, const void* recs, const int32_t* status, uint32_t i, uint32_t chunks,
                           uint32_t E, uint64_t out_base);
/* The stages behind a front end's argument checks, as zd_ranges_stages enqueues them. The front end: the stand-in's RVR_BAD_PLAN
 * check of a job's place (may_direct 1: 16-byte aligned; 0: always the job's slot), the job and verdict functions its kernels call,
 * its copy-out of job i. work: s->bytes, of any alignment. -> ZXC_OK or RVR_BAD_PLAN. */
static inline int rvr_stages(int may_direct, rvr_job_fn job, rvr_verdict_fn verdict, rvr_out_fn copy_out, uint32_t E, uint64_t src_size,
                             const void* index, const zxc_dev_rangev_t* ranges, uint32_t n_ranges, uint64_t max_len, uint32_t bs, int have_dict,
                             uint32_t have_id, const rvr_blocks_t* blk, const zr_shape_t* s, uint8_t* work, int64_t* results) {
    const uint64_t out_base = zc_round_up((uint64_t)(uintptr_t)work, 256u);
    uint8_t* base = work + (out_base - (uint64_t)(uintptr_t)work);
    zxc_dev_job_t* jobs = (zxc_dev_job_t*)(base + s->o_jobs);
    int32_t* status = (int32_t*)(base + s->o_status);
    void* recs = base + s->o_copy;
    const uint64_t* offs = zr_coffsets(index);

    for (uint32_t i = 0; i < s->n_jobs; i++)
        job(index, ranges[i / s->J], i % s->J, i, src_size, max_len, bs, out_base, s->o_stage, have_dict, have_id, &jobs[i], recs);
    for (uint32_t i = 0; i < s->n_jobs; i++) {
        status[i] = ZXC_ERROR_SRC_TOO_SMALL;
        if (jobs[i].out_len != bs) return RVR_BAD_PLAN;
        if (may_direct ? (jobs[i].out_off & 15u) != 0 : jobs[i].out_off != s->o_stage + (uint64_t)i * s->slot_stride) return RVR_BAD_PLAN;
        if (jobs[i].comp_size == 0) continue;
        const uint64_t b = ranges[i / s->J].offset / bs + i % s->J;
        if (b >= blk->n || offs[b] != jobs[i].comp_off || offs[b + 1u] - offs[b] != jobs[i].comp_size) return RVR_BAD_PLAN;
        uint8_t* out = rvr_at(out_base, jobs[i].out_off);
        status[i] = blk->status[b];
        if (status[i] < 0) { memset(out, 0x5A, bs / 2u); continue; }
        const uint32_t n = (uint32_t)status[i] < bs ? (uint32_t)status[i] : bs;
        memcpy(out, blk->bytes + blk->at[b], n);
        memset(out + n, 0xA5, 32);
    }
    for (uint32_t i = 0; i < s->n_jobs; i++) copy_out(base + s->o_stage, s->slot_stride, recs, status, i, s->copy_chunks, E, out_base);
    for (uint32_t r = 0; r < n_ranges; r++)
        results[r] = verdict(index, ranges[r], s->J, status + (uint64_t)r * s->J, src_size, max_len, bs, have_dict, have_id);
    return ZXC_OK;
}

static inline void rvr_job(const void* index, zxc_dev_rangev_t r, uint32_t j, uint64_t i, uint64_t src_size, uint64_t max_len, uint32_t bs,
                           uint64_t out_base, uint64_t stage_rel, int have_dict, uint32_t have_id, zxc_dev_job_t* job, void* recs) {
    zrv_job(index, r, j, i, src_size, max_len, bs, out_base, stage_rel, have_dict, have_id, job, (zr_copy_t*)recs + i);
}
/* The whole rangesv call. -> ZXC_OK, a synchronous error of the entry point's argument checks, or RVR_BAD_PLAN. */
static inline int rvr_call(uint64_t src_size, const void* index, const zxc_dev_rangev_t* ranges, uint32_t n_ranges, uint64_t max_len,
                           uint32_t bs, int have_dict, uint32_t have_id, const rvr_blocks_t* blk, int64_t* results) {
    zr_shape_t s;
    const int shape_rc = zr_shape(n_ranges, max_len, bs, &s);
    if (shape_rc != 0) return shape_rc;
    if (n_ranges == 0) return ZXC_OK;
    uint8_t* work = malloc(s.bytes);
    const int rc = rvr_stages(1, rvr_job, zrv_verdict, rvr_copy_job, 0u, src_size, index, ranges, n_ranges, max_len, bs, have_dict, have_id, blk, &s, work, results);
    free(work);
    return rc;
}

/* The seeded table of the two stand-alone sanitizer programs: the fixed ranges, random ones, then the three that are refused by
 * their destination: one longer than max_len and two (at most 100 and 50 bytes) that get a zero and a wrapping base. -> n */
static inline uint32_t rvr_san_table(const uint64_t (*fixed)[2], uint32_t n_fixed, uint32_t maxr, uint64_t total, uint32_t bs,
                                     uint32_t (*rnd)(void), uint64_t* off, uint64_t* len, uint64_t* max_len) {
    uint32_t n = 0;
    for (; n < n_fixed; n++) { off[n] = fixed[n][0]; len[n] = fixed[n][1]; }
    while (n < maxr - 3) {
        off[n] = rnd() % total;
        len[n] = 1u + rnd() % (3ull * bs + 40u);
        if (len[n] > total - off[n] && (rnd() & 7u)) len[n] = total - off[n];
        n++;
    }
    *max_len = 1;
    for (uint32_t r = 0; r < n; r++) if (off[r] + len[r] <= total && len[r] > *max_len) *max_len = len[r];
    if (*max_len > 3ull * bs + 40u && total > 8ull * bs) *max_len = 3ull * bs + 40u; /* (the whole archive is then refused: len > max_len) */
    off[n] = 0; len[n] = *max_len + 1u; n++;
    off[n] = 0; len[n] = total < 100u ? total : 100u; n++;
    off[n] = 0; len[n] = total < 50u ? total : 50u; n++;
    return n;
}
/* what the early verdict owes entry r of that table */
static inline int64_t rvr_san_want(const uint64_t* off, const uint64_t* len, uint32_t n, uint32_t r, uint64_t max_len, uint64_t total) {
    if (len[r] == 0) return 0;
    if (len[r] > max_len || r == n - 1u) return ZXC_ERROR_DST_TOO_SMALL;
    if (r == n - 2u) return ZXC_ERROR_NULL_INPUT;
    return off[r] > total || len[r] > total - off[r] ? ZXC_ERROR_SRC_TOO_SMALL : (int64_t)len[r];
}
/* One pass over the table: a valid range's destination is a heap buffer of exactly k[r] + len bytes, its base k[r] bytes in; a refused
 * or empty range gets no buffer at all: its base is never dereferenced. far == 0: the wrapping base's end is at 2^64, else past it. */
static inline void rvr_san_pass(const uint64_t* off, const uint64_t* len, const uint32_t* k, uint32_t n, uint64_t max_len, uint64_t total, int far,
                                zxc_dev_rangev_t* tab, uint8_t** raw) {
    for (uint32_t r = 0; r < n; r++) {
        const int valid = rvr_san_want(off, len, n, r, max_len, total) > 0;
        raw[r] = valid ? malloc(len[r] + k[r]) : NULL;
        tab[r].offset = off[r]; tab[r].len = len[r];
        tab[r].base = valid ? (uint64_t)(uintptr_t)(raw[r] + k[r]) : 0x1000u + k[r];
        if (r == n - 2u) tab[r].base = 0;
        if (r == n - 1u) tab[r].base = ~(uint64_t)0 - (far ? len[r] / 2u : len[r] - 1u);
    }
}
#endif
