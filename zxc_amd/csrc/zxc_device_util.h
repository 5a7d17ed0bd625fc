// zxc_device_util.h — what the device-to-device calls share (zxc_frame_device.hip, zxc_unframe_device.hip, zxc_ranges_device.hip,
// zxc_batch_device.hip, zxc_cbatch_device.hip, zxc_cpack_device.hip, zxc_append_device.hip, zxc_take_device.hip,
// zxc_dict_device.hip, zxc_shuffle_device.hip, zxc_rangesv_shuffle_device.hip, zxc_shufflev_device.hip): the three tile passes every container stage is made of, the 64-bit workgroup scan, the copy out of a staged slot, the gather of a run of blocks, and the host-side plumbing
// of an entry point: the launch check, the work area's base, the dictionary argument, the one reader of zxc_compress_opts_t, and
// the launches the decode-side calls share: the verification tables, the copy grid, the container and the verdict stages, and the
// ranges family's plan and verdict kernel bodies and its four stages (zd_ranges_plan, zd_ranges_verdict, zd_ranges_stages).
// HIP only; the container rules themselves are the plain C of zxc_container.h / zxc_ranges.h / zxc_batch.h / zxc_cbatch.h.
//
// A tile is ZC_TILE_BLOCKS consecutive blocks, handled by one workgroup of ZD_TILE_THREADS threads, ZD_PER_THREAD consecutive
// blocks per thread. Every helper with a barrier in it is called by all threads of the workgroup, outside divergent control flow.
// The wave primitives and the copy are those of zxc_wave.h, the same ones the decode and encode kernels use.
#ifndef ZXC_DEVICE_UTIL_H
#define ZXC_DEVICE_UTIL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zxc_container.h"
#include "zxc_kernels.h"  // the container stages that zd_container_stages and zd_verdict_stages launch
#include "zxc_wave.h"

#define ZD_TILE_THREADS 256u
#define ZD_WAVES (ZD_TILE_THREADS / 64u)
#define ZD_PER_THREAD (ZC_TILE_BLOCKS / ZD_TILE_THREADS)
#define ZD_WORK_ALIGN 256u  // every part of a work area starts on this, counted from the aligned base (zd_work_base)

// ---------------------------------------------------------------- tile passes
struct zd_totals {
    uint64_t sum;
    uint32_t hash, bad;  // the hashes xored, the bad flags (0 / 1) ored
};

// Reduce over the workgroup: every thread hands in the sum, the hash and the bad flag of its own blocks; all threads get the
// totals back. One barrier. A thread's sum is at most 2^24 (four entries of at most ZC_SEEK_ENTRY_MAX, or four block sizes of at
// most 2 MiB + 64), a wave's then at most 2^30: 32 bits hold both, and the waves are added in 64.
__device__ __forceinline__ zd_totals zd_tile_reduce(uint32_t sum, uint32_t hash, uint32_t bad) {
    __shared__ uint32_t w_sum[ZD_WAVES], w_hash[ZD_WAVES], w_bad[ZD_WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    sum = wave_sum(sum);
    hash = wave_xor(hash);
    bad = __any(bad) ? 1u : 0u;
    if (lane == 0) { w_sum[wave] = sum; w_hash[wave] = hash; w_bad[wave] = bad; }
    __syncthreads();
    zd_totals r = {0, 0, 0};
    for (uint32_t w = 0; w < ZD_WAVES; w++) { r.sum += w_sum[w]; r.hash ^= w_hash[w]; r.bad |= w_bad[w]; }
    return r;
}

// Exclusive offsets inside a tile: sum = this thread's entries added up (the bound of zd_tile_reduce holds), base = the offset of
// the tile's first block. -> base + the entries of all lower threads: the offset of this thread's first block. One barrier.
__device__ __forceinline__ uint64_t zd_tile_offset(uint32_t sum, uint64_t base) {
    __shared__ uint32_t w_incl[ZD_WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t incl = wave_scan_add(sum);
    if (lane == 63) w_incl[wave] = incl;
    __syncthreads();
    uint64_t at = base + incl - sum;
    for (uint32_t w = 0; w < wave; w++) at += w_incl[w];
    return at;
}

// One workgroup of 256 threads over the n_tiles words the reduce pass left, one per tile: load(i, hash, bad) returns tile i's sum
// and folds its hash and bad flag into the two references; store(i, v) puts v where tile i's sum was. Thread t owns tiles
// [t * per, (t + 1) * per): a serial sum, a 64-bit scan of the 256 sums (a tile's sum can pass 2^31), a serial write-back. Every
// tile's word becomes base + the sums of the tiles in front of it; all threads get the totals (the sum without base). One barrier,
// behind every thread's loads and in front of every store.
template <class Load, class Store>
__device__ __forceinline__ zd_totals zd_scan_tiles(uint32_t n_tiles, uint64_t base, Load load, Store store) {
    __shared__ uint64_t w_tot[4];
    __shared__ uint32_t w_hash[4], w_bad[4];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t per = (n_tiles + 255u) / 256u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t mine = 0;
    uint32_t hash = 0, bad = 0;
    for (uint32_t i = lo; i < hi; i++) mine += load(i, hash, bad);
    uint64_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(incl, (unsigned)d);
        if ((int)lane >= d) incl += o;
    }
    hash = wave_xor(hash);
    bad = __any(bad) ? 1u : 0u;
    if (lane == 63) w_tot[wave] = incl;
    if (lane == 0) { w_hash[wave] = hash; w_bad[wave] = bad; }
    __syncthreads();
    zd_totals r = {0, 0, 0};
    uint64_t run = base + incl - mine;
    for (uint32_t w = 0; w < 4u; w++) {
        if (w < wave) run += w_tot[w];
        r.sum += w_tot[w];
        r.hash ^= w_hash[w];
        r.bad |= w_bad[w];
    }
    for (uint32_t i = lo; i < hi; i++) {
        uint32_t h = 0, b = 0;
        const uint64_t s = load(i, h, b);
        store(i, run);
        run += s;
    }
    return r;
}

// Exclusive scan of one 64-bit value per thread over the workgroup of 256, adding up saturating at 2^64 - 1 (min(a + b, 2^64 - 1)
// is associative, so the grouping does not show): -> the sum of all lower threads' values; *all gets the workgroup's sum. The
// scan of appendv's table of lengths (zxc_append_device.hip), which may say anything, and of the pack call's extents
// (zxc_cpack_device.hip), which never saturate. zd_sat_add is zav_sat_add of zxc_appendv.h, which the plain C rules keep. One
// barrier; called by all threads outside divergent control flow, once per kernel.
__device__ __forceinline__ uint64_t zd_sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}
__device__ __forceinline__ uint64_t zd_wg_scan64(uint64_t mine, uint64_t* all) {
    __shared__ uint64_t w_tot[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(incl, (unsigned)d);
        if ((int)lane >= d) incl = zd_sat_add(o, incl);
    }
    uint64_t excl = __shfl_up(incl, 1u);
    if (lane == 0) excl = 0;
    if (lane == 63) w_tot[wave] = incl;
    __syncthreads();
    uint64_t run = 0, tot = 0;
    for (uint32_t w = 0; w < 4u; w++) {
        if (w < wave) run = zd_sat_add(run, w_tot[w]);
        tot = zd_sat_add(tot, w_tot[w]);
    }
    *all = tot;
    return zd_sat_add(run, excl);
}

// ---------------------------------------------------------------- staged slot -> destination
#define ZD_COPY_CHUNK 8192u  // destination bytes one wavefront moves (ZB_COPY_CHUNK)

// One wavefront's part of the copy s[0, n) -> d[0, n), d of any alignment: chunk k is the part whose destination addresses lie in
// [A + k CHUNK, A + (k + 1) CHUNK), A = d rounded down to 16. A lane moves 16-byte units of the destination: an aligned 16-byte
// store fed by a 16-byte load of any alignment from the slot, bytes where the unit passes the copy's ends. (The loop of
// zxc_ranges_copy_kernel, which keeps its own copy: that kernel is left exactly as it was.)
__device__ __forceinline__ void zd_copy_chunk(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, int64_t n, uint32_t k, uint32_t lane) {
    // rel: position in the copy of this lane's first unit (negative in front of the head)
    int64_t rel = (int64_t)k * ZD_COPY_CHUNK - (int64_t)((uintptr_t)d & 15u) + 16 * (int64_t)lane;
#pragma unroll 4
    for (uint32_t u = 0; u < ZD_COPY_CHUNK / 1024u; u++, rel += 1024) {
        if (rel >= n) break;
        if (rel >= 0 && rel + 16 <= n) {
            *(v4u*)(d + rel) = ld128(s + rel);
        } else {
            const int64_t lo = rel < 0 ? 0 : rel, hi = rel + 16 < n ? rel + 16 : n;
            for (int64_t b = lo; b < hi; b++) d[b] = s[b];
        }
    }
}

// Compaction, one wave per block: block b's sizes[b] bytes at slots + b x slot_stride -> dst + offsets[b], for b < nb. The body of
// zxc_frame_gather_kernel and zxc_append_gather_kernel, behind their test of the status word.
__device__ __forceinline__ void zd_gather_blocks(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes,
                                                 const uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t nb) {
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    for (uint64_t b = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); b < nb; b += (uint64_t)gridDim.x * waves) {
        copy_bytes(dst + offsets[b], slots + b * slot_stride, sizes[b], lane, 64u);
    }
}

// ---------------------------------------------------------------- the ranges family: plan and verdict
// The bodies of the plan and verdict kernels of ranges, rangesv (zxc_ranges_device.hip) and the shuffled ranges
// (zxc_rangesv_shuffle_device.hip). The rules stand once in zxc_ranges.h; a front end hands in its thin function over them.
// plan: one thread per job, 256 per workgroup; job_of(range, j, job_index, &job, &record) is zr_job_dict, zrv_job or zrs_job.
template <class Range, class Rec, class JobOf>
__device__ __forceinline__ void zd_ranges_plan(const Range* __restrict__ ranges, uint32_t J, uint32_t n_jobs, zxc_dev_job_t* __restrict__ jobs,
                                               Rec* __restrict__ recs, JobOf job_of) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_jobs) return;
    const uint32_t r = i / J, j = i - r * J;
    zxc_dev_job_t job;
    Rec rec;
    job_of(ranges[r], j, i, &job, &rec);
    jobs[i] = job;
    recs[i] = rec;
}
// verdict: one thread per range, 256 per workgroup; verdict_of(range, its J statuses) is zr_verdict_dict, zrv_verdict or zrs_verdict.
template <class Range, class VerdictOf>
__device__ __forceinline__ void zd_ranges_verdict(const Range* __restrict__ ranges, uint32_t n_ranges, uint32_t J, const int32_t* __restrict__ status,
                                                  int64_t* __restrict__ results, VerdictOf verdict_of) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_ranges) return;
    results[r] = verdict_of(ranges[r], status + (uint64_t)r * J);
}

// ---------------------------------------------------------------- a kernel two files launch
// zxc_frame_device.hip defines it; zxc_append_device.hip launches it per piece. Declared once, here, which both include: a
// definition that departs from this is a conflicting redeclaration and does not compile (as zxc_kernels.h).
extern "C" __global__ void zxc_frame_tiles_kernel(const uint8_t* slots, uint32_t slot_stride, const uint32_t* sizes, uint32_t nb,
                                                  uint32_t block_size, uint32_t checksum, uint64_t* tile_sum, uint32_t* tile_hash,
                                                  uint32_t* tile_bad);

// ---------------------------------------------------------------- host side of an entry point
// hidden entry point of zxc_hip_shim.hip (decode_launch)
extern "C" int zxc_hip_decode_blocks(const void* d_comp, const zxc_dev_job_t* d_jobs, uint32_t n_jobs, void* d_out, int32_t* d_status,
                                     uint32_t block_size, int verify_trailer, const void* d_dict, uint32_t dict_size,
                                     const void* d_dict_huf, uint32_t cap_override, void* stream);

static inline bool launched() { return hipGetLastError() == hipSuccess; }
static inline bool have_device() {
    int n_dev = 0, dev = -1;
    return hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0 && hipGetDevice(&dev) == hipSuccess && dev >= 0;
}
// the caller's d_work may have any alignment: the work area starts at the next multiple of ZD_WORK_ALIGN (the *_work_size count it)
static inline uint8_t* zd_work_base(void* d_work) { return (uint8_t*)zc_round_up((uint64_t)(uintptr_t)d_work, ZD_WORK_ALIGN); }
// The dictionary argument of a *_dict_device call. -> ZXC_OK or the error; a dictionary of size 0 is no dictionary (*dict = NULL).
static inline int dict_arg(const zxc_dev_dict_t** dict) {
    const zxc_dev_dict_t* d = *dict;
    if (d && d->size > ZC_DICT_MAX) return ZXC_ERROR_DICT_TOO_LARGE;
    if (d && d->size > 0 && (!d->d_content || !d->d_id)) return ZXC_ERROR_NULL_INPUT;
    if (d && d->size == 0) *dict = NULL;
    return ZXC_OK;
}
// The dictionary as a call's launches take it, behind dict_arg: everything NULL or 0 when there is none.
struct zd_dict_t {
    const void *content, *huf;
    const uint32_t* id;
    uint32_t size;
};
static inline zd_dict_t zd_dict_of(const zxc_dev_dict_t* d) { return d ? zd_dict_t{d->d_content, d->d_huf, d->d_id, d->size} : zd_dict_t{NULL, NULL, NULL, 0u}; }
// ---- the launches the decode-side calls share
// A call that may verify decodes table tb < tables with verify_trailer = tb (whether the blocks carry trailers is known on the
// device only): its n jobs at jobs + tb x job_stride, their statuses at status + tb x status_stride. -> the first rc != ZXC_OK.
static inline int zd_decode_tables(const void* d_src, const zxc_dev_job_t* jobs, uint64_t job_stride, uint32_t n, void* d_out, int32_t* status,
                                   uint64_t status_stride, uint32_t block_size, uint32_t tables, const zd_dict_t& dict, void* stream) {
    int rc = ZXC_OK;
    for (uint32_t tb = 0; tb < tables && rc == ZXC_OK; tb++)
        rc = zxc_hip_decode_blocks(d_src, jobs + tb * job_stride, n, d_out, status + tb * status_stride, block_size, (int)tb, dict.content,
                                   dict.size, dict.huf, 0u, stream);
    return rc;
}
// One decode launch for a call's destination and the staged slots of its work area: job offsets are 64-bit and counted from d_out,
// so d_out is the lower of the two (both are 16-byte aligned, which keeps the out_off of every slot and of every block decoded
// straight a multiple of 16). -> d_out; *dst_rel, *stage_rel: the two areas counted from it (d_dst == NULL: no destination).
static inline uint8_t* zd_out_base(void* d_dst, uint8_t* stage, uint64_t* dst_rel, uint64_t* stage_rel) {
    uint8_t *dst = (uint8_t*)d_dst, *out = (dst && dst < stage) ? dst : stage;
    *dst_rel = dst ? (uint64_t)(dst - out) : 0u;
    *stage_rel = (uint64_t)(stage - out);
    return out;
}
// The grid of a copy launch over `units` (copy, 8 KiB) pairs: a wavefront each, four to a workgroup; past 2^20 workgroups the kernels stride.
static inline dim3 zd_copy_grid(uint64_t units) { return dim3((uint32_t)((units + 3u) / 4u < (1u << 20) ? (units + 3u) / 4u : (1u << 20))); }
// A call of the ranges family (ranges, rangesv, the shuffled ranges) in stream order, behind its entry point's own checks: plan,
// one decode launch over all jobs with d_out = out, the copy-out of the staged slots, verdict. base: the work area's; the jobs, the
// statuses, the front end's records and the slots are carved from the shape. The launches a front end owns are handed in:
// plan(grid, jobs, recs), copy_out(grid, stage, recs, status), verdict(grid, status).
template <class Plan, class CopyOut, class Verdict>
static inline int zd_ranges_stages(const void* d_src, const zr_shape_t& s, uint8_t* base, void* out, uint32_t n_ranges, uint32_t block_size,
                                   const zd_dict_t& dict, void* stream, Plan plan, CopyOut copy_out, Verdict verdict) {
    zxc_dev_job_t* jobs = (zxc_dev_job_t*)(base + s.o_jobs);
    int32_t* status = (int32_t*)(base + s.o_status);
    void* recs = base + s.o_copy;
    plan(dim3((s.n_jobs + 255u) / 256u), jobs, recs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const int rc = zxc_hip_decode_blocks(d_src, jobs, s.n_jobs, out, status, block_size, 0, dict.content, dict.size, dict.huf, 0u, stream);
    if (rc != ZXC_OK) return rc;
    copy_out(zd_copy_grid((uint64_t)s.n_jobs * s.copy_chunks), (const uint8_t*)(base + s.o_stage), (const void*)recs, (const int32_t*)status);
    verdict(dim3((n_ranges + 255u) / 256u), (const int32_t*)status);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
// The container's parts of a work area, from a zc_shape_t or from a zt_shape_t, which keeps zc_shape's offsets up to o_status.
struct zd_cwork_t {
    zc_ctl_t* ctl;
    uint64_t* tile_sum;
    uint32_t *tile_hash, *tile_bad, n_jobs, n_tiles;
    zxc_dev_job_t* jobs;
    int32_t* status;
};
template <class Shape>
static inline zd_cwork_t zd_cwork(uint8_t* base, const Shape& s) {
    return zd_cwork_t{(zc_ctl_t*)base, (uint64_t*)(base + s.o_tile_sum), (uint32_t*)(base + s.o_tile_hash), (uint32_t*)(base + s.o_tile_bad),
                      s.n_jobs, s.n_tiles, (zxc_dev_job_t*)(base + s.o_jobs), (int32_t*)(base + s.o_status)};
}
// The container stages of zxc_unframe_device.hip in stream order: clear, head, tiles, scan, scatter, walk -> the control word and
// the job table the head stage picks. Jobs below k_direct get their block's place in one destination as out_off.
static inline int zd_container_stages(const zd_cwork_t& w, const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size,
                                      uint32_t want_verify, uint32_t k_direct, const uint32_t* dict_id, hipStream_t st) {
    if (hipMemsetAsync(w.jobs, 0, (size_t)(1u + want_verify) * w.n_jobs * sizeof(zxc_dev_job_t), st) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_unframe_head_kernel, dim3(1), dim3(64), 0, st, src, src_size, dst_capacity, block_size, want_verify, w.n_jobs, w.ctl, dict_id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    if (dst_capacity == 0) return ZXC_OK;  // (the empty-frame probe is answered by the head stage alone)
    hipLaunchKernelGGL(zxc_unframe_tiles_kernel, dim3(w.n_tiles), dim3(ZD_TILE_THREADS), 0, st, src, (const zc_ctl_t*)w.ctl, w.tile_sum, w.tile_bad);
    hipLaunchKernelGGL(zxc_unframe_scan_kernel, dim3(1), dim3(256), 0, st, w.tile_sum, (const uint32_t*)w.tile_bad, w.n_tiles, w.ctl);
    hipLaunchKernelGGL(zxc_unframe_scatter_kernel, dim3(w.n_tiles), dim3(ZD_TILE_THREADS), 0, st, src, (const zc_ctl_t*)w.ctl,
                       (const uint64_t*)w.tile_sum, block_size, k_direct, w.n_jobs, w.jobs, w.tile_hash, w.tile_bad);
    hipLaunchKernelGGL(zxc_unframe_walk_kernel, dim3(1), dim3(256), 0, st, src, src_size, block_size, k_direct, w.n_jobs,
                       (const uint32_t*)w.tile_hash, (const uint32_t*)w.tile_bad, w.jobs, w.ctl);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
// ... and the verdict stages behind every decode launch: events over the whole status table, then *d_result, written once.
static inline int zd_verdict_stages(const zd_cwork_t& w, uint32_t block_size, uint64_t dst_capacity, int64_t* d_result, hipStream_t st) {
    if (dst_capacity > 0) {
        hipLaunchKernelGGL(zxc_unframe_events_kernel, dim3(w.n_tiles * 4u < 1024u ? w.n_tiles * 4u : 1024u), dim3(256), 0, st,
                           (const int32_t*)w.status, block_size, w.n_jobs, dst_capacity, w.ctl);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    hipLaunchKernelGGL(zxc_unframe_result_kernel, dim3(1), dim3(64), 0, st, (const zc_ctl_t*)w.ctl, (const int32_t*)w.status, block_size, w.n_jobs, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
// The scan of a table of (base, len) entries (zxc_appendv.h; the kernels of zxc_append_device.hip), in stream order: starts[0 .. n_iov],
// the table's status in *vctl, and its fold into *fold: the session's control word for appendv, a word nobody reads for takev.
static inline int zd_iov_scan(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint32_t n_tiles, uint64_t* tile_sum, uint32_t* tile_flags,
                              uint64_t* starts, zav_ctl_t* vctl, zap_ctl_t* fold, hipStream_t st) {
    hipLaunchKernelGGL(zxc_appendv_reduce_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, iov, n_iov, total, tile_sum, tile_flags);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_appendv_scan_kernel, dim3(1), dim3(256), 0, st, tile_sum, (const uint32_t*)tile_flags, n_tiles, total, starts, n_iov, vctl, fold);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_appendv_starts_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, iov, n_iov, (const uint64_t*)tile_sum, starts);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
// Options as zxc_compress reads them (zxc_host.c): level 3 unless given, at most 7; blocks of 512 KiB unless given. -> ZXC_OK or
// ZXC_ERROR_BAD_BLOCK_SIZE. opts->dict is not looked at: each caller refuses it at its own place in its order of errors.
struct zd_copts_t {
    uint32_t block_size, level, checksum, seekable;
};
static inline int zd_compress_opts(const zxc_compress_opts_t* opts, zd_copts_t* o) {
    const int level = (opts && opts->level > 0) ? opts->level : 3;
    const uint64_t bs = (opts && opts->block_size > 0) ? (uint64_t)opts->block_size : 512u * 1024u;
    if (!zc_block_size_ok(bs)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    o->block_size = (uint32_t)bs;
    o->level = (uint32_t)(level > 7 ? 7 : level);
    o->checksum = (opts && opts->checksum_enabled) ? 1u : 0u;
    o->seekable = (opts && opts->seekable) ? 1u : 0u;
    return ZXC_OK;
}
#endif
