// zxc_hip_shim.hip — the only C <-> HIP crossing of libzxc_mi355x.so.
// extern "C" entry points declared in include/zxc_mi355x.h; host C code
// (zxc_host.c) and external callers use plain pointers and sizes only.
#include "zxc_experiments.h"  // (first: the gate in front of every experiment switch)
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/zxc_error.h"
#include "zxc_encode_levels.h"
#include "zxc_kernels.h"  // every kernel launched here and its workgroup size; zxc_dev.h

#ifdef EXP_ENC_CLOCKS  // (experiment build only, tools/encclk.py)
extern "C" __attribute__((visibility("default"))) int zxc_mi355x_exp_enc_clocks(unsigned long long* out8) {
    unsigned long long* d = NULL;
    if (hipMalloc((void**)&d, 64) != hipSuccess) return -1;
    hipLaunchKernelGGL(zxc_enc_clk_read_kernel, dim3(1), dim3(64), 0, 0, d);
    const hipError_t e = hipMemcpy(out8, d, 64, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}
#endif

// Per-device scratch for expanded literal / token sections: one slot per resident
// workgroup. Grown on demand, never shrunk; freed at process exit by the driver.
#define ZXC_MAX_DEVICES 16
#define ZXC_RLE_LEAN_MAX_JOBS 16384u
#define ZXC_ORDER_STREAMS 16
#define ZXC_POOLS 10 /* block_size_log2 12..21 */
/* One scratch pool per block size: slot stride and count depend on block_size only, so concurrent launches on different streams
 * either share a pool with identical geometry (same busy flag guards the same bytes) or use disjoint pools. */
struct Pool { uint8_t* scratch; uint32_t* busy; uint32_t n_slots; uint32_t stride; };
/* A stream's launch-order slot: launch-order buffer (zxc_dev_ord_layout), helper streams and events, pinned hint page, section /
 * RLE scratch (capacities in bytes). Launches on one stream are ordered: its buffers are free again when its next launch is enqueued. */
struct Ord {
    void* stream; int used; uint32_t* buf; size_t buf_cap; hipStream_t aux, aux2; hipEvent_t fork, join, join2, small_done;
    uint32_t* hint; uint8_t* pscratch; size_t pscratch_cap; uint8_t* rscratch; size_t rscratch_cap;
};
static struct {
    Pool pool[ZXC_POOLS];
    int cus, wg_per_cu, lean_wg_per_cu;
    Ord ord[ZXC_ORDER_STREAMS];
} g_dev[ZXC_MAX_DEVICES];
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;

#ifdef ZXC_EXPERIMENT  // the plan-forcing bits ZXC_DEV_DBG_* (zxc_dev.h) exist only in experiment builds (tools/build_variant.sh)
static uint32_t g_debug_flags = 0;
#else
#define g_debug_flags 0u
#endif

static int current_device(void) {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= ZXC_MAX_DEVICES) return -1;
    return d;
}

extern "C" {

#ifdef ZXC_EXPERIMENT
/* experiment builds only (not in include/): forces decode plans (ZXC_DEV_DBG_NO_ORDER / _NO_TWO_PASS) for tools/kbench.py */
__attribute__((visibility("default"))) void zxc_mi355x__set_debug(uint32_t flags) { g_debug_flags = flags; }
#endif

int zxc_mi355x_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int zxc_mi355x_set_device(int device) {
    return hipSetDevice(device) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int zxc_mi355x_get_device(void) {
    int d = -1;
    return hipGetDevice(&d) == hipSuccess ? d : ZXC_ERROR_GPU_UNAVAILABLE;
}

void* zxc_mi355x_malloc(size_t bytes) {
    void* p = NULL;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return NULL;
    return p;
}

void zxc_mi355x_free(void* d_ptr) {
    if (d_ptr) (void)hipFree(d_ptr);
}

int zxc_mi355x_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
    if (bytes == 0) return ZXC_OK;
    return hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int zxc_mi355x_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return ZXC_OK;
    return hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

/* internal to the library (hidden): a worker thread's own stream and the copies on it (zxc_host.c) */
int zxc_hip_stream_create(void** stream_out) {
    hipStream_t st = NULL;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    *stream_out = (void*)st;
    return ZXC_OK;
}
void zxc_hip_stream_destroy(void* stream) {
    if (!stream) return;
    const int dev = current_device();
    if (dev >= 0) {  // the launch-order buffer (and helper stream) this stream used is free for another one
        pthread_mutex_lock(&g_lock);
        for (int i = 0; i < ZXC_ORDER_STREAMS; i++)
            if (g_dev[dev].ord[i].used && g_dev[dev].ord[i].stream == stream) { g_dev[dev].ord[i].used = 0; g_dev[dev].ord[i].stream = NULL; }
        pthread_mutex_unlock(&g_lock);
    }
    (void)hipStreamDestroy((hipStream_t)stream);
}
int zxc_hip_memcpy_h2d_async(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    if (bytes == 0) return ZXC_OK;
    return hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
int zxc_hip_memcpy_d2h_async(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes == 0) return ZXC_OK;
    return hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

/* internal to the library (hidden): what the host API's piece pipeline needs besides streams (zxc_host.c) — an event behind a
 * piece's launch, and pinned host memory for its block statuses (a stream-ordered copy into it needs no staging and no wait) */
int zxc_hip_event_create(void** ev_out) {
    hipEvent_t e = NULL;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    *ev_out = (void*)e;
    return ZXC_OK;
}
void zxc_hip_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }
int zxc_hip_event_record(void* ev, void* stream) {
    return hipEventRecord((hipEvent_t)ev, (hipStream_t)stream) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
int zxc_hip_event_synchronize(void* ev) {
    return hipEventSynchronize((hipEvent_t)ev) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
void* zxc_hip_host_alloc(size_t bytes) {
    void* p = NULL;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return NULL;
    return p;
}
void zxc_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }

extern "C" void zxc_host_release_arenas(void);
/* Gives back the device memory this library keeps between calls: the host API's staging arenas (those nobody is using)
 * and, on the calling thread's device, the scratch pools of the section decoders and the launch-order buffers. Call it
 * when no launch of this library is in flight on that device (pools and order buffers belong to launches). */
void zxc_mi355x_release_cached(void) {
    zxc_host_release_arenas();
    const int dev = current_device();
    if (dev < 0) return;
    (void)hipDeviceSynchronize();
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < ZXC_POOLS; i++) {
        auto& p = g_dev[dev].pool[i];
        if (p.scratch) (void)hipFree(p.scratch);
        if (p.busy) (void)hipFree(p.busy);
        p.scratch = NULL; p.busy = NULL; p.n_slots = 0; p.stride = 0;
    }
    for (int i = 0; i < ZXC_ORDER_STREAMS; i++) {
        auto& o = g_dev[dev].ord[i];
        if (o.buf) (void)hipFree(o.buf);
        if (o.pscratch) (void)hipFree(o.pscratch);
        if (o.rscratch) (void)hipFree(o.rscratch);
        o.buf = NULL; o.buf_cap = 0;
        o.pscratch = NULL; o.pscratch_cap = 0;
        o.rscratch = NULL; o.rscratch_cap = 0;
    }
    pthread_mutex_unlock(&g_lock);
}

int zxc_mi355x_synchronize(void* stream) {
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

// The full kernel's scratch pool of a block size, made on first use: a slot per resident workgroup, claimed in-kernel by blocks with
// an RLE / PivCo section only (waiters spin, holders never wait), so it may be smaller: capped at 1 GiB of scratch. (under g_lock)
static int setup_pool(int dev, uint32_t block_size, Pool** pool_out, uint32_t* max_slots) {
    auto& d = g_dev[dev];
    if (d.cus == 0 && (hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || d.cus <= 0)) d.cus = 256;
    // one workgroup (one wavefront) per block; how many are resident (LDS / register limited) is asked from the runtime
    if (d.wg_per_cu == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&d.wg_per_cu, zxc_decode_blocks_kernel, 64, 0) != hipSuccess ||
                             d.wg_per_cu <= 0 || d.wg_per_cu > 32))
        d.wg_per_cu = 32;
    *max_slots = (uint32_t)d.cus * (uint32_t)d.wg_per_cu;  // <= 8192
    // the lean kernel's residency, which the launch order is mixed for (zxc_dev_order_mix)
    if (d.lean_wg_per_cu == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&d.lean_wg_per_cu, zxc_decode_blocks_lean_kernel, 64, 0) != hipSuccess ||
                                  d.lean_wg_per_cu <= 0 || d.lean_wg_per_cu > 32))
        d.lean_wg_per_cu = 24;
    Pool& pool = *(*pool_out = &d.pool[__builtin_ctz(block_size) - 12]);
    if (pool.scratch) return ZXC_OK;
    const uint32_t stride = ZXC_DEV_SLOT_STRIDE(block_size);
    uint32_t n = (uint32_t)(((size_t)1 << 30) / stride);
    if (n > *max_slots) n = *max_slots;
    if (n < 64u) n = 64u;
    uint8_t* sc = NULL;
    uint32_t* busy = NULL;
    if (hipMalloc((void**)&sc, (size_t)n * stride) != hipSuccess) return ZXC_ERROR_MEMORY;
    if (hipMalloc((void**)&busy, (size_t)n * 4u) != hipSuccess) { (void)hipFree(sc); return ZXC_ERROR_MEMORY; }
    // slot-busy flags, zero = free (every workgroup releases what it took). The memset runs on the null
    // stream, which a non-blocking user stream does not wait for: finish it before anyone can launch.
    if (hipMemset(busy, 0, (size_t)n * 4u) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(sc), (void)hipFree(busy);
        return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    pool = Pool{sc, busy, n, stride};
    return ZXC_OK;
}

// The stream's launch-order slot: its own, else a free one; NULL with more streams than slots (then one kernel in plain order,
// still correct). A slot that changes owner forgets its previous owner's hints: its first launch plans like any first launch.
static Ord* claim_slot(int dev, void* stream) {
    Ord* ord = g_dev[dev].ord;
    for (int i = 0; i < ZXC_ORDER_STREAMS; i++)
        if (ord[i].used && ord[i].stream == stream) return &ord[i];
    for (int i = 0; i < ZXC_ORDER_STREAMS; i++)
        if (!ord[i].used) {
            ord[i].used = 1, ord[i].stream = stream;
            if (ord[i].hint) { ord[i].hint[0] = 0xFFFFFFFFu; ord[i].hint[1] = 0u; }
            return &ord[i];
        }
    return NULL;
}

// A slot's helper streams, their events and its pinned hint page: created by its first two-pass launch, retried if that fails.
static void make_helpers(Ord& o) {
    if (o.aux) return;
    if (hipStreamCreateWithFlags(&o.aux, hipStreamNonBlocking) != hipSuccess) { o.aux = NULL; return; }
    const unsigned f = hipEventDisableTiming;
    if (hipStreamCreateWithFlags(&o.aux2, hipStreamNonBlocking) != hipSuccess) { (void)hipStreamDestroy(o.aux); o.aux = NULL; return; }
    if (hipEventCreateWithFlags(&o.fork, f) != hipSuccess || hipEventCreateWithFlags(&o.join, f) != hipSuccess ||
        hipEventCreateWithFlags(&o.join2, f) != hipSuccess || hipEventCreateWithFlags(&o.small_done, f) != hipSuccess) {
        (void)hipStreamDestroy(o.aux), (void)hipStreamDestroy(o.aux2);
        o.aux = NULL;
    } else if (!o.hint) {
        if (hipHostMalloc((void**)&o.hint, 64, hipHostMallocDefault) == hipSuccess) { o.hint[0] = 0xFFFFFFFFu; o.hint[1] = 0u; }
        else o.hint = NULL;
    }
}

// Grows one of a slot's buffers to at least `bytes` (never shrinks; the contents are not kept). false: it has none now.
static bool grow(void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return true;
    if (*p) (void)hipFree(*p);
    *cap = 0;
    if (hipMalloc(p, bytes) != hipSuccess) { *p = NULL; return false; }
    *cap = bytes;
    return true;
}

// What the kernels of one decode launch take. The pointers into the launch-order buffer are NULL where the plan has no use for them.
struct Launch {
    const uint8_t* comp; const zxc_dev_job_t* jobs; uint32_t n; uint8_t* out; int32_t* status; uint32_t bs, cap_override;
    zxc_dev_plan_t plan; hipStream_t s0; const Pool* pool; uint32_t max_slots, cus, mix_slots; Ord* o;
    uint32_t *order, *list, *ctl, *pre_entries; zxc_dev_sec_t* secs; zxc_dev_pre_t* pre;
    uint8_t *ck_bad, *pscratch, *rscratch; uint32_t pscratch_cap16, rscratch_cap16;
};

// The launch-order pass: heaviest-first order[] (a launch ends when its slowest block ends); in a two-pass plan also the full
// kernel's list, the block classes, the section kernels' work lists, and the hint words for the next launch on this stream.
static void order_pass(const Launch& L) {
    const uint32_t g = (L.n + 255u) / 256u;
    hipLaunchKernelGGL(zxc_order_hist_kernel, dim3(g), dim3(256), 0, L.s0, L.comp, L.jobs, L.n, L.bs, L.o->buf);
    hipLaunchKernelGGL(zxc_order_scatter_kernel, dim3(g), dim3(256), 0, L.s0, L.comp, L.jobs, L.n, L.bs, L.o->buf, L.order, L.list,
                       L.plan.trailer_bytes & ~ZXC_DEV_TRAILER_ELSEWHERE, L.pre, L.ctl, L.pre_entries, L.secs, L.pscratch_cap16,
                       L.cap_override ? L.cap_override : L.bs + 2112u, L.rscratch_cap16, L.mix_slots);
    if (L.ctl && L.o->hint) {  // (pinned: a stream-ordered copy, read by the next launch without waiting)
        (void)hipMemcpyAsync(L.o->hint, L.ctl + ZXC_DEV_CTL_WANTED, 4, hipMemcpyDeviceToHost, L.s0);
        (void)hipMemcpyAsync(L.o->hint + 1, L.ctl + ZXC_DEV_CTL_RLE_WANTED, 4, hipMemcpyDeviceToHost, L.s0);
    }
}

// The full kernel: over every block (FULL plan), or over its list on a fixed grid that pulls work through counters (two-pass).
static void launch_full(const Launch& L, hipStream_t st, uint32_t grid) {
    hipLaunchKernelGGL(zxc_decode_blocks_kernel, dim3(grid), dim3(64), 0, st, L.comp, L.jobs, L.n, L.out, L.status, L.bs, L.plan.trailer_bytes,
                       L.pool->scratch, L.pool->stride, g_debug_flags, L.pool->busy, L.pool->n_slots, L.order, L.cap_override, L.list);
}

// the LEAN_RLE blocks' literals, in front of the lean kernel on its stream (a small grid: it is over in a few microseconds)
static void launch_rle(const Launch& L, hipStream_t st) {
    if (!L.rscratch_cap16) return;
    hipLaunchKernelGGL(zxc_rle_expand_kernel, dim3(L.n < 8u * L.cus ? L.n : 8u * L.cus), dim3(64), 0, st, L.comp, L.jobs, L.pre,
                       L.rscratch, L.ctl + ZXC_DEV_CTL_RLE_LIST, L.pre_entries + L.n - 1u);
}

// The two-pass plans' streams, s0 = the caller's, aux / aux2 = its slot's helpers:
//   TWO_PASS:      s0: [RLE literals,] lean kernel over every block, [checksum merge] | aux: full kernel over its list
//                  | aux2: [checksum kernel]
//   TWO_PASS_PRE:  s0: section kernels medium, large, [small done], the lean kernel's second entry (PRE blocks)
//                  | aux: [RLE literals,] lean kernel (LEAN class) | aux2: section kernel small, THEN the full kernel
// (the small class first: the lean kernel's second entry waits for small_done, and the full kernel's persistent workgroups
// hold their stream for as long as the slowest one-wave block takes: VERDICT r3 weak #3)
// The helpers wait for the fork event on s0 and are joined back by one event each (capturable, no host synchronisation); one
// whose wait failed is not used. fail() waits for them before an error is reported: the host path frees its arena right after.
// Per-block checksums apart (round 6): hashed by their own kernel, nine blocks per wavefront, beside the decode; the decode
// kernels only skip the trailers, and the merge kernel writes BAD_CHECKSUM over the status of the blocks that failed, behind
// every kernel that writes a status. Inside the decode kernels 57 of 64 lanes idle through the hash: -8.9 % of the launch
// inline against -7.7 % apart (profiles/r6j_checksum_kernel_ab.log).
static bool fork_to(Ord& o, hipStream_t h) { return hipStreamWaitEvent(h, o.fork, 0) == hipSuccess; }
static int fail(Ord& o) { (void)hipStreamSynchronize(o.aux), (void)hipStreamSynchronize(o.aux2); return ZXC_ERROR_GPU_UNAVAILABLE; }
static int join(Ord& o, hipStream_t s0, bool aux, bool aux2) {
    if ((aux && (hipEventRecord(o.join, o.aux) != hipSuccess || hipStreamWaitEvent(s0, o.join, 0) != hipSuccess)) ||
        (aux2 && (hipEventRecord(o.join2, o.aux2) != hipSuccess || hipStreamWaitEvent(s0, o.join2, 0) != hipSuccess)))
        return fail(o);
    return ZXC_OK;
}

static int enqueue_two_pass(const Launch& L) {
    Ord& o = *L.o; const hipStream_t s0 = L.s0;
    const bool aux = hipEventRecord(o.fork, s0) == hipSuccess && fork_to(o, o.aux);
    launch_full(L, aux ? o.aux : s0, L.n < L.max_slots ? L.n : L.max_slots);
    const bool aux2 = L.plan.ck_apart && aux && fork_to(o, o.aux2);
    if (L.plan.ck_apart)
        hipLaunchKernelGGL(zxc_block_checksum_kernel, dim3((L.n + 8u) / 9u), dim3(64), 0, aux2 ? o.aux2 : s0, L.comp, L.jobs, L.n, L.order, L.ck_bad, L.mix_slots);
    launch_rle(L, s0);
    hipLaunchKernelGGL(zxc_decode_blocks_lean_kernel, dim3(L.n), dim3(64), 0, s0, L.comp, L.jobs, L.n, L.out, L.status, L.bs, L.order,
                       L.cap_override, L.plan.trailer_bytes, L.pre, L.rscratch);
    if (const int rc = join(o, s0, aux, aux2)) return rc;
    if (L.plan.ck_apart)
        hipLaunchKernelGGL(zxc_checksum_merge_kernel, dim3((L.n + 255u) / 256u), dim3(256), 0, s0, L.ck_bad, L.status, L.n);
    return ZXC_OK;
}

static int enqueue_two_pass_pre(const Launch& L) {
    Ord& o = *L.o;
    const bool forked = hipEventRecord(o.fork, L.s0) == hipSuccess && fork_to(o, o.aux) && fork_to(o, o.aux2);
    const hipStream_t s0 = L.s0, s1 = forked ? o.aux : s0, s2 = forked ? o.aux2 : s0;
    uint32_t* sec_hdr = L.ctl + ZXC_DEV_CTL_SEC;
    auto grid = [&](uint32_t per_cu) { const uint32_t g = per_cu * L.cus; return dim3(2u * L.n < g ? 2u * L.n : g); };
    launch_rle(L, s1);
    hipLaunchKernelGGL(zxc_decode_blocks_lean_kernel, dim3(L.n), dim3(64), 0, s1, L.comp, L.jobs, L.n, L.out, L.status, L.bs, L.order,
                       L.cap_override, L.plan.trailer_bytes, L.pre, L.rscratch);
    // (the small class runs beside the medium / large ones, on its own stream: +1 % level 7, +4 % level 6)
    hipLaunchKernelGGL(zxc_pivco_sections_small_kernel, grid(10), dim3(PDIR_SMALL_THREADS), 0, s2, L.comp, L.secs, sec_hdr, L.pre, L.pscratch);
    if (forked && hipEventRecord(o.small_done, s2) != hipSuccess) return fail(o);
    launch_full(L, s2, L.n < L.max_slots ? L.n : L.max_slots);
    hipLaunchKernelGGL(zxc_pivco_sections_medium_kernel, grid(3), dim3(PDIR_MEDIUM_THREADS), 0, s0, L.comp, L.secs + 2u * (size_t)L.n, sec_hdr + 2, L.pre, L.pscratch);
    hipLaunchKernelGGL(zxc_pivco_sections_large_kernel, grid(2), dim3(PDIR_LARGE_THREADS), 0, s0, L.comp, L.secs + 4u * (size_t)L.n, sec_hdr + 4, L.pre, L.pscratch);
    if (forked && hipStreamWaitEvent(s0, o.small_done, 0) != hipSuccess) return fail(o);
    hipLaunchKernelGGL(zxc_decode_blocks_lean_pre_kernel, dim3(L.n), dim3(64), 0, s0, L.comp, L.jobs, L.out, L.status, L.bs,
                       L.cap_override, L.plan.trailer_bytes, L.pre, L.pscratch, L.ctl + ZXC_DEV_CTL_PRE, L.pre_entries);
    return join(o, s0, forked, forked);
}

// Steps: validate, pool, claim slot and helpers (if the plan could use them), choose, provision, settle, order pass, enqueue.
static int decode_launch(const void* d_comp, const zxc_dev_job_t* d_jobs, uint32_t n_jobs, void* d_out,
                         int32_t* d_status, uint32_t block_size, int verify_trailer, void* stream, const void* d_dict,
                         uint32_t dict_size, const void* d_dict_huf, uint32_t cap_override = 0) {
    if (n_jobs == 0) return ZXC_OK;
    if (!d_comp || !d_jobs || !d_out || !d_status) return ZXC_ERROR_NULL_INPUT;
    if (block_size < (1u << 12) || block_size > (1u << 21) || (block_size & (block_size - 1u))) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const int dev = current_device();
    if (dev < 0) return ZXC_ERROR_GPU_UNAVAILABLE;
    zxc_dev_plan_in_t in = {(uint32_t)(d_dict || d_dict_huf), cap_override, n_jobs, 0u, g_debug_flags, (uint32_t)(verify_trailer != 0), block_size};
    in.rle_lean_max_jobs = ZXC_RLE_LEAN_MAX_JOBS;
    // switches (A/B and fault isolation), read on every launch
    in.ck_inline = getenv("ZXC_MI355X_CK_INLINE") != NULL, in.no_rle_scratch = getenv("ZXC_MI355X_NO_RLE_SCRATCH") != NULL;
#ifdef EXP_NO_PRE  // (experiment: every coded block to the full kernel)
    in.no_pre = 1;
#endif
    struct Unlock { ~Unlock() { pthread_mutex_unlock(&g_lock); } } unlock_on_return;
    pthread_mutex_lock(&g_lock);
    Pool* pool;
    if (const int rc = setup_pool(dev, block_size, &pool, &in.max_slots)) return rc;
    in.slot = in.helpers = 1;
    const zxc_dev_plan_t could = zxc_dev_plan_choose(&in);
    Ord* o = could.ordered ? claim_slot(dev, stream) : NULL;
    if (o && could.kind >= ZXC_DEV_PLAN_TWO_PASS) make_helpers(*o);
    in.slot = o != NULL; in.helpers = o && o->aux; in.hint = o && o->hint;
    if (in.hint) { in.hint0 = *(volatile uint32_t*)o->hint; in.hint1 = *(volatile uint32_t*)(o->hint + 1); }
    zxc_dev_plan_t plan = zxc_dev_plan_choose(&in);
    const hipStream_t s0 = (hipStream_t)stream; const zxc_dev_ord_layout_t at = zxc_dev_ord_layout(n_jobs);
    if (plan.ordered) in.order_failed = !grow((void**)&o->buf, &o->buf_cap, at.words * 4u);
    if (plan.pscratch_bytes) in.pscratch_failed = !grow((void**)&o->pscratch, &o->pscratch_cap, plan.pscratch_bytes);
    if (plan.rscratch_bytes) in.rscratch_failed = !grow((void**)&o->rscratch, &o->rscratch_cap, plan.rscratch_bytes);
    if (plan.ordered && !in.order_failed)
        in.order_failed = hipMemsetAsync(o->buf, 0, 130u * 4u, s0) != hipSuccess ||
                          hipMemsetAsync(o->buf + at.ctl, 0, ZXC_DEV_CTL_WORDS * 4u, s0) != hipSuccess;
    plan = zxc_dev_plan_choose(&in);  // settle
    Launch L = {(const uint8_t*)d_comp, d_jobs, n_jobs, (uint8_t*)d_out, d_status, block_size, cap_override, plan, s0, pool,
                in.max_slots, (uint32_t)g_dev[dev].cus, (uint32_t)g_dev[dev].cus * (uint32_t)g_dev[dev].lean_wg_per_cu, o};
#ifdef ZXC_EXPERIMENT  // (tools/ordermix.py: 0 = sorted, 0xFFFFFFFF = file order, else the residency the order is mixed for)
    if (const char* e = getenv("ZXC_EXP_ORDER_SLOTS")) L.mix_slots = (uint32_t)strtoul(e, NULL, 0);
#endif
    if (plan.ordered) L.order = o->buf + at.order;
    if (plan.kind >= ZXC_DEV_PLAN_TWO_PASS) {
        L.list = o->buf + at.list; L.ctl = o->buf + at.ctl; L.pre_entries = o->buf + at.pre_ent;
        L.secs = (zxc_dev_sec_t*)(o->buf + at.secs); L.pre = (zxc_dev_pre_t*)(o->buf + at.pre); L.ck_bad = (uint8_t*)(o->buf + at.ck_bad);
        if (plan.pscratch_bytes) { L.pscratch = o->pscratch; L.pscratch_cap16 = (uint32_t)(o->pscratch_cap >> 4); }
        if (plan.rscratch_bytes) { L.rscratch = o->rscratch; L.rscratch_cap16 = (uint32_t)(o->rscratch_cap >> 4); }
    }
    if (plan.ordered) order_pass(L);
    if (plan.kind == ZXC_DEV_PLAN_TWO_PASS || plan.kind == ZXC_DEV_PLAN_TWO_PASS_PRE) {
        if (const int rc = plan.kind == ZXC_DEV_PLAN_TWO_PASS ? enqueue_two_pass(L) : enqueue_two_pass_pre(L)) return rc;
    } else if (plan.kind == ZXC_DEV_PLAN_DICT)
        hipLaunchKernelGGL(zxc_decode_blocks_dict_kernel, dim3(n_jobs), dim3(64), 0, s0, L.comp, d_jobs, n_jobs, L.out, d_status, block_size,
                           plan.trailer_bytes, pool->scratch, pool->stride, g_debug_flags, pool->busy, pool->n_slots, L.order, cap_override,
                           (const uint8_t*)d_dict, dict_size, (const uint8_t*)d_dict_huf);
    else
        launch_full(L, s0, n_jobs);
    return hipGetLastError() == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int zxc_mi355x_decode_blocks_device(const void* d_comp, const zxc_dev_job_t* d_jobs, uint32_t n_jobs, void* d_out,
                                    int32_t* d_status, uint32_t block_size, int verify_trailer, void* stream) {
    return decode_launch(d_comp, d_jobs, n_jobs, d_out, d_status, block_size, verify_trailer, stream, NULL, 0, NULL);
}

int zxc_mi355x_decode_blocks_dict_device(const void* d_comp, const zxc_dev_job_t* d_jobs, uint32_t n_jobs, void* d_out,
                                         int32_t* d_status, uint32_t block_size, int verify_trailer, const void* d_dict,
                                         uint32_t dict_size, const void* d_dict_huf, void* stream) {
    if (dict_size > 65535u || (dict_size && !d_dict)) return ZXC_ERROR_DICT_TOO_LARGE;
    return decode_launch(d_comp, d_jobs, n_jobs, d_out, d_status, block_size, verify_trailer, stream, d_dict, dict_size,
                         d_dict_huf);
}

/* internal to the library (hidden): the host C file's Block API needs the strict capacity of
 * zxc_decompress_block_safe (cap_override != 0: per-block output cap instead of block_size + 2112) and the
 * device the calling thread is on (per-device staging arenas). */
int zxc_hip_decode_blocks(const void* d_comp, const zxc_dev_job_t* d_jobs, uint32_t n_jobs, void* d_out, int32_t* d_status,
                          uint32_t block_size, int verify_trailer, const void* d_dict, uint32_t dict_size,
                          const void* d_dict_huf, uint32_t cap_override, void* stream) {
    if (dict_size > 65535u || (dict_size && !d_dict)) return ZXC_ERROR_DICT_TOO_LARGE;
    return decode_launch(d_comp, d_jobs, n_jobs, d_out, d_status, block_size, verify_trailer, stream, d_dict, dict_size,
                         d_dict_huf, cap_override);
}
int zxc_hip_current_device(void) { return current_device(); }

uint32_t zxc_mi355x_encode_slot_stride(uint32_t block_size) { return 2u * block_size + 512u; }

static int encode_launch(const void* d_src, uint64_t src_size, uint32_t block_size, int level, int with_checksum,
                         const void* d_dict, uint32_t dict_size, void* d_work, void* d_slots, uint32_t* d_sizes, void* stream) {
    // the level picks the kernel entry (table geometry = occupancy, GHI / GLO) and the search effort (zxc_encode_levels.h)
    if (src_size == 0) return ZXC_OK;
    if (!d_src || !d_slots || !d_sizes || (dict_size && (!d_dict || !d_work))) return ZXC_ERROR_NULL_INPUT;
    if (block_size < (1u << 12) || block_size > (1u << 21) || (block_size & (block_size - 1u))) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (dict_size > 65535u) return ZXC_ERROR_DICT_TOO_LARGE;
    if (current_device() < 0) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint64_t nb64 = (src_size + block_size - 1u) / block_size;
    if (nb64 > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint32_t nb = (uint32_t)nb64;
    const uint8_t* in = (const uint8_t*)d_src;
    if (dict_size) {  // [dict | block] image per block: the dictionary seeds every block's tables
        hipLaunchKernelGGL(zxc_prepend_dict_kernel, dim3(nb), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_src, src_size,
                           block_size, (const uint8_t*)d_dict, dict_size, (uint8_t*)d_work, nb);
        if (hipGetLastError() != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;  // (noticed here, not behind the encode launch)
        in = (const uint8_t*)d_work;
    }
    zxc_enc_level_t lp = zxc_enc_level_bs(level, block_size);
    uint8_t* huf_scratch = NULL;
    if (lp.huf) {
        // levels 6-7: level buffers + coded sections of the PivCo encoder, 4 x (block_size + 64) per block. Stream-ordered
        // allocation: it belongs to this launch alone (concurrent launches on other streams get their own) and is given
        // back to the device pool right behind the kernel.
        const size_t need = (size_t)nb * 4u * ((size_t)block_size + 64u);
        if (hipMallocAsync((void**)&huf_scratch, need, (hipStream_t)stream) != hipSuccess || !huf_scratch) return ZXC_ERROR_MEMORY;
    }
    auto kern = lp.entry == 0 ? zxc_encode_blocks_kernel_l1 : lp.entry == 1 ? zxc_encode_blocks_kernel_l2
              : lp.entry == 2 ? zxc_encode_blocks_kernel_l3 : lp.entry == 3 ? zxc_encode_blocks_kernel_l4
              : lp.entry == 4 ? zxc_encode_blocks_kernel_l57 : zxc_encode_blocks_kernel_l67;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(64), 0, (hipStream_t)stream, in, src_size, block_size,
                       (uint8_t*)d_slots, zxc_mi355x_encode_slot_stride(block_size), d_sizes, nb, with_checksum ? 1u : 0u,
                       lp.depth, lp.sufficient, lp.lazy, dict_size, huf_scratch, lp.huf);
    const hipError_t lerr = hipGetLastError();
    if (huf_scratch) (void)hipFreeAsync(huf_scratch, (hipStream_t)stream);
    return lerr == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

/* The encode launch over a job table whose inputs are in place: workgroup i encodes d_jobs[i].len bytes at in + d_jobs[i].src_off
 * (behind dict_size dictionary bytes when there is a dictionary) into slot i and writes d_sizes[i]. Entry and effort come from the
 * level table as in encode_launch. */
static int encode_jobs_launch(const uint8_t* in, const zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level,
                              int with_checksum, uint32_t dict_size, void* d_slots, uint32_t* d_sizes, void* stream) {
    zxc_enc_level_t lp = zxc_enc_level_bs(level, block_size);
    uint8_t* huf_scratch = NULL;
    if (lp.huf) {  // levels 6-7: the PivCo encoder's scratch per job, stream-ordered as in encode_launch
        const size_t need = (size_t)n_jobs * 4u * ((size_t)block_size + 64u);
        if (hipMallocAsync((void**)&huf_scratch, need, (hipStream_t)stream) != hipSuccess || !huf_scratch) return ZXC_ERROR_MEMORY;
    }
    auto kern = lp.entry == 0 ? zxc_encode_jobs_kernel_l1 : lp.entry == 1 ? zxc_encode_jobs_kernel_l2
              : lp.entry == 2 ? zxc_encode_jobs_kernel_l3 : lp.entry == 3 ? zxc_encode_jobs_kernel_l4
              : lp.entry == 4 ? zxc_encode_jobs_kernel_l57 : zxc_encode_jobs_kernel_l67;
    hipLaunchKernelGGL(kern, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, in, d_jobs, block_size,
                       (uint8_t*)d_slots, zxc_mi355x_encode_slot_stride(block_size), d_sizes, n_jobs, with_checksum ? 1u : 0u,
                       lp.depth, lp.sufficient, lp.lazy, dict_size, huf_scratch, lp.huf);
    const hipError_t lerr = hipGetLastError();
    if (huf_scratch) (void)hipFreeAsync(huf_scratch, (hipStream_t)stream);
    return lerr == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

/* internal to the library (hidden): the encode launch over a job table in device memory (zxc_cbatch_device.hip): workgroup i
 * encodes d_jobs[i].len bytes at d_base + d_jobs[i].src_off into slot i and writes d_sizes[i]; a job of len 0 is unused and its
 * d_sizes[i] stays. Entry and effort come from the level table as in encode_launch. With dict_size != 0 the jobs point at
 * [dict | block] images, made in d_images from the jobs' source bytes first (zxc_encode_job_images_kernel, which repoints the
 * jobs): d_base is then the source, d_images holds n_jobs images + 64 bytes. The caller checked the arguments. */
int zxc_hip_encode_jobs(const void* d_base, zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level, int with_checksum,
                        const void* d_dict, uint32_t dict_size, void* d_images, void* d_slots, uint32_t* d_sizes, void* stream) {
    if (n_jobs == 0) return ZXC_OK;
    const uint8_t* in = (const uint8_t*)d_base;
    if (dict_size) {
        hipLaunchKernelGGL(zxc_encode_job_images_kernel, dim3(n_jobs), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_base, d_jobs,
                           n_jobs, block_size, (const uint8_t*)d_dict, dict_size, (uint8_t*)d_images);
        if (hipGetLastError() != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
        in = (const uint8_t*)d_images;
    }
    return encode_jobs_launch(in, d_jobs, n_jobs, block_size, level, with_checksum, dict_size, d_slots, d_sizes, stream);
}

/* internal to the library (hidden): the same launch over images the caller has built (zxc_append_device.hip): job i's src_off is
 * the offset of its [dict | len bytes] image from d_images, behind the last of which ZC_IMAGE_PAD bytes are readable. dict_size
 * != 0. Nothing is written to the jobs or the images. */
int zxc_hip_encode_job_images(const void* d_images, const zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level,
                              int with_checksum, uint32_t dict_size, void* d_slots, uint32_t* d_sizes, void* stream) {
    if (n_jobs == 0) return ZXC_OK;
    return encode_jobs_launch((const uint8_t*)d_images, d_jobs, n_jobs, block_size, level, with_checksum, dict_size, d_slots, d_sizes, stream);
}

int zxc_mi355x_encode_blocks_device(const void* d_src, uint64_t src_size, uint32_t block_size, int level,
                                    int with_checksum, void* d_slots, uint32_t* d_sizes, void* stream) {
    return encode_launch(d_src, src_size, block_size, level, with_checksum, NULL, 0, NULL, d_slots, d_sizes, stream);
}

uint64_t zxc_mi355x_encode_dict_work_size(uint64_t src_size, uint32_t block_size, uint32_t dict_size) {
    const uint64_t nb = block_size ? (src_size + block_size - 1u) / block_size : 0;
    return nb * ((uint64_t)block_size + dict_size) + 64u;
}

int zxc_mi355x_encode_blocks_dict_device(const void* d_src, uint64_t src_size, uint32_t block_size, int level,
                                         int with_checksum, const void* d_dict, uint32_t dict_size, void* d_work,
                                         void* d_slots, uint32_t* d_sizes, void* stream) {
    return encode_launch(d_src, src_size, block_size, level, with_checksum, d_dict, dict_size, d_work, d_slots, d_sizes, stream);
}

int zxc_mi355x_gather_blocks_device(const void* d_slots, uint32_t block_size, const uint32_t* d_sizes,
                                    const uint64_t* d_offsets, void* d_out, uint32_t n_blocks, void* stream) {
    if (n_blocks == 0) return ZXC_OK;
    if (!d_slots || !d_sizes || !d_offsets || !d_out) return ZXC_ERROR_NULL_INPUT;
    hipLaunchKernelGGL(zxc_gather_blocks_kernel, dim3(n_blocks), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_slots,
                       zxc_mi355x_encode_slot_stride(block_size), d_sizes, d_offsets, (uint8_t*)d_out, n_blocks);
    return hipGetLastError() == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

/* internal to the library (hidden): offsets of a piece's blocks in its compacted output, computed where the sizes are (zxc_host.c:
 * the compaction follows the encode on its stream) */
int zxc_hip_block_offsets(uint32_t* d_sizes, uint64_t* d_offsets, uint32_t n_blocks, uint32_t max_size, void* stream) {
    if (n_blocks == 0) return ZXC_OK;
    if (!d_sizes || !d_offsets) return ZXC_ERROR_NULL_INPUT;
    hipLaunchKernelGGL(zxc_block_offsets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_sizes, d_offsets, n_blocks, max_size);
    return hipGetLastError() == hipSuccess ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // extern "C"
