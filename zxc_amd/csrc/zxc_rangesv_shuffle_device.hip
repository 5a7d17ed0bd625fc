// zxc_rangesv_shuffle_device.hip — zxc_mi355x_decompress_rangesv_shuffle_device (include/zxc_mi355x_rangesv_shuffle.h): ranges of
// the plain bytes of a seekable archive of byte-shuffled blocks, each into a destination of its own, device to device. The rules
// are the inline C of zxc_rangesv_shuffle.h on top of zxc_rangesv.h and zxc_shuffle.h, which the CPU tests run as well.
//
// In stream order, as rangesv_call of zxc_ranges_device.hip:
//   plan     one thread per job: validates its range, writes the job (always a staged slot) and the gather record
//   decode   the existing decode launch, once, over all jobs (with the dictionary when there is one)
//   gather   one wavefront per (job, 8 KiB of the block's plain bytes): the slot's planes -> the range's destination
//   verdict  one thread per range: d_results[r]
//
// The gather is the un-shuffle kernel's lane plan (zxc_shuffle_device.hip) restricted to what a range wants of a block: a lane owns
// a whole group of 16 elements, E 16-byte loads from the planes of the slot (contiguous across the wavefront), zsh_regs_unshuffle,
// E 16-byte stores of 16 E contiguous bytes at whatever alignment the range's base gives. A range's two edge groups and the
// leftovers of a ragged last block move a byte at a time. Nothing is stored for a job until its status has been held against the
// block's length. Destinations are counted from the work area's 256-byte aligned base modulo 2^64, rangesv's convention. No LDS.
#include "zxc_device_util.h"  // ld128, the host-side plumbing; the kernels' declarations (zxc_kernels.h)
#include "zxc_rangesv_shuffle.h"

extern "C" __global__ void __launch_bounds__(256)
zxc_rangesv_shuffle_plan_kernel(const void* __restrict__ index, const zxc_dev_rangev_t* __restrict__ ranges, uint32_t J, uint32_t n_jobs,
                                uint64_t src_size, uint64_t max_len, uint32_t block_size, uint64_t out_base, uint64_t stage_rel,
                                zxc_dev_job_t* __restrict__ jobs, zrs_gather_t* __restrict__ gathers, const uint32_t* __restrict__ dict_id) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_jobs) return;
    const uint32_t r = i / J, j = i - r * J;
    zxc_dev_job_t job;
    zrs_gather_t ga;
    zrs_job(index, ranges[r], j, i, src_size, max_len, block_size, out_base, stage_rel, dict_id != nullptr, dict_id ? *dict_id : 0u, &job, &ga);
    jobs[i] = job;
    gathers[i] = ga;
}

namespace {

__device__ __forceinline__ void st128(uint8_t* p, v4u v) { *(v4u_unaligned*)p = v; }

// One wavefront per item = (job, chunk), grid-striding as zxc_ranges_copy_kernel does. Most items are empty (empty jobs, chunks a
// range does not reach) and end at once.
template <uint32_t E>
__device__ __forceinline__ void gather_body(const uint8_t* __restrict__ stage, uint32_t slot_stride, const zrs_gather_t* __restrict__ gathers,
                                            const int32_t* __restrict__ status, uint32_t n_jobs, uint32_t chunks, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t items = (uint64_t)n_jobs * chunks, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < items; it += waves) {
        const uint32_t i = (uint32_t)(it / chunks), c = (uint32_t)(it - (uint64_t)i * chunks);
        const zrs_gather_t ga = gathers[i];
        zrs_item_t item;
        if (ga.n == 0 || !zrs_item(ga.from, ga.n, ga.m, E, c, &item)) continue;
        if (zrs_block_verdict(status[i], ga.m) != 0) continue;  // (the range fails: its bytes are undefined, nothing is moved)
        const uint8_t* s = stage + (uint64_t)i * slot_stride;
        uint8_t* d = out + ga.dst_at;  // plain byte p of the block goes to d[p - from]
        const uint32_t q = ga.m / E;
#pragma unroll
        for (uint32_t turn = 0; turn < 8u / E; turn++) {
            const uint32_t g = item.g_lo + turn * 64u + lane;
            if (g >= item.g_hi) continue;
            uint32_t e[4u * E], p[4u * E];
#pragma unroll
            for (uint32_t k = 0; k < E; k++) {
                const v4u v = ld128(s + (uint64_t)k * q + 16u * g);
                p[4u * k] = v.x; p[4u * k + 1u] = v.y; p[4u * k + 2u] = v.z; p[4u * k + 3u] = v.w;
            }
            zsh_regs_unshuffle(p, e, E);
            uint8_t* to = d + (g * (ZSH_GROUP * E) - ga.from);
#pragma unroll
            for (uint32_t j = 0; j < E; j++) {
                const v4u v = {e[4u * j], e[4u * j + 1u], e[4u * j + 2u], e[4u * j + 3u]};
                st128(to + 16u * j, v);
            }
        }
        for (uint32_t k = lane; k < item.head_n + item.tail_n; k += 64u) {
            const uint32_t p = zrs_single(&item, k);
            d[p - ga.from] = s[zrs_src(p, ga.m, E)];
        }
    }
}

}  // namespace

#define ZRS_KERNEL(name, E)                                                                                                            \
    extern "C" __global__ void __launch_bounds__(256) name(const uint8_t* __restrict__ stage, uint32_t slot_stride,                   \
                                                           const zrs_gather_t* __restrict__ gathers, const int32_t* __restrict__ status, \
                                                           uint32_t n_jobs, uint32_t chunks, uint8_t* __restrict__ out) {              \
        gather_body<E>(stage, slot_stride, gathers, status, n_jobs, chunks, out);                                                     \
    }
ZRS_KERNEL(zxc_rangesv_shuffle_gather2_kernel, 2u)
ZRS_KERNEL(zxc_rangesv_shuffle_gather4_kernel, 4u)
ZRS_KERNEL(zxc_rangesv_shuffle_gather8_kernel, 8u)

extern "C" __global__ void __launch_bounds__(256)
zxc_rangesv_shuffle_verdict_kernel(const void* __restrict__ index, const zxc_dev_rangev_t* __restrict__ ranges, uint32_t n_ranges, uint32_t J,
                                   const int32_t* __restrict__ status, uint64_t src_size, uint64_t max_len, uint32_t block_size,
                                   int64_t* __restrict__ results, const uint32_t* __restrict__ dict_id) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_ranges) return;
    results[r] = zrs_verdict(index, ranges[r], J, status + (uint64_t)r * J, src_size, max_len, block_size, dict_id != nullptr,
                             dict_id ? *dict_id : 0u);
}

extern "C" {

uint64_t zxc_mi355x_decompress_rangesv_shuffle_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size) {
    zrs_shape_t s;
    return zrs_shape(n_ranges, max_len, block_size, &s) != 0 ? 0u : s.bytes;
}

int zxc_mi355x_decompress_rangesv_shuffle_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_rangev_t* d_ranges,
                                                 uint32_t n_ranges, uint64_t max_len, uint32_t elem_size, uint32_t block_size,
                                                 const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_results,
                                                 void* stream) {
    if (!d_src || !d_index || !d_work || !d_results || (!d_ranges && n_ranges > 0)) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    zrs_shape_t s;
    const int shape_rc = zrs_shape(n_ranges, max_len, block_size, &s);
    if (shape_rc == ZXC_ERROR_BAD_BLOCK_SIZE) return shape_rc;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if (shape_rc != 0 || work_size < s.bytes) return ZXC_ERROR_MEMORY;
    if (n_ranges == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const zd_dict_t dc = zd_dict_of(dict);
    uint8_t* base = zd_work_base(d_work);
    zxc_dev_job_t* jobs = (zxc_dev_job_t*)(base + s.o_jobs);
    int32_t* status = (int32_t*)(base + s.o_status);
    zrs_gather_t* gathers = (zrs_gather_t*)(base + s.o_gather);
    const uint8_t* stage = base + s.o_stage;

    hipLaunchKernelGGL(zxc_rangesv_shuffle_plan_kernel, dim3((s.n_jobs + 255u) / 256u), dim3(256), 0, st, d_index, d_ranges, s.J, s.n_jobs,
                       src_size, max_len, block_size, (uint64_t)(uintptr_t)base, s.o_stage, jobs, gathers, dc.id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const int rc = zxc_hip_decode_blocks(d_src, jobs, s.n_jobs, base, status, block_size, 0, dc.content, dc.size, dc.huf, 0u, stream);
    if (rc != ZXC_OK) return rc;
    const dim3 grid = zd_copy_grid((uint64_t)s.n_jobs * s.chunks), block(256);
    if (elem_size == 2u)
        hipLaunchKernelGGL(zxc_rangesv_shuffle_gather2_kernel, grid, block, 0, st, stage, s.slot_stride, (const zrs_gather_t*)gathers,
                           (const int32_t*)status, s.n_jobs, s.chunks, base);
    else if (elem_size == 4u)
        hipLaunchKernelGGL(zxc_rangesv_shuffle_gather4_kernel, grid, block, 0, st, stage, s.slot_stride, (const zrs_gather_t*)gathers,
                           (const int32_t*)status, s.n_jobs, s.chunks, base);
    else
        hipLaunchKernelGGL(zxc_rangesv_shuffle_gather8_kernel, grid, block, 0, st, stage, s.slot_stride, (const zrs_gather_t*)gathers,
                           (const int32_t*)status, s.n_jobs, s.chunks, base);
    hipLaunchKernelGGL(zxc_rangesv_shuffle_verdict_kernel, dim3((n_ranges + 255u) / 256u), dim3(256), 0, st, d_index, d_ranges, n_ranges, s.J,
                       (const int32_t*)status, src_size, max_len, block_size, d_results, dc.id);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // extern "C"
