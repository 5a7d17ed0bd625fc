// zxc_rangesv_shuffle_device.hip — zxc_mi355x_decompress_rangesv_shuffle_device (include/zxc_mi355x_rangesv_shuffle.h): ranges of
// the plain bytes of a seekable archive of byte-shuffled blocks, each into a destination of its own, device to device. The third
// front end of the ranges family (ranges and rangesv are zxc_ranges_device.hip's): rangesv's request over the one rule set of
// zxc_ranges.h with no block decoded in place and a block's status held against its length, and the gather plan of
// zxc_rangesv_shuffle.h on top of zxc_shuffle.h, all of it inline C that the CPU tests run as well.
//
// In stream order, enqueued by zd_ranges_stages (zxc_device_util.h) as for the two siblings:
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
    zd_ranges_plan(ranges, J, n_jobs, jobs, gathers, [=](zxc_dev_rangev_t r, uint32_t j, uint32_t i, zxc_dev_job_t* job, zrs_gather_t* ga) {
        zrs_job(index, r, j, i, src_size, max_len, block_size, out_base, stage_rel, dict_id != nullptr, dict_id ? *dict_id : 0u, job, ga);
    });
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
    zd_ranges_verdict(ranges, n_ranges, J, status, results, [=](zxc_dev_rangev_t r, const int32_t* st) {
        return zrs_verdict(index, r, J, st, src_size, max_len, block_size, dict_id != nullptr, dict_id ? *dict_id : 0u);
    });
}

extern "C" {

uint64_t zxc_mi355x_decompress_rangesv_shuffle_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size) {
    zr_shape_t s;
    return zrs_shape(n_ranges, max_len, block_size, &s) != 0 ? 0u : s.bytes;
}

int zxc_mi355x_decompress_rangesv_shuffle_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_rangev_t* d_ranges,
                                                 uint32_t n_ranges, uint64_t max_len, uint32_t elem_size, uint32_t block_size,
                                                 const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_results,
                                                 void* stream) {
    if (!d_src || !d_index || !d_work || !d_results || (!d_ranges && n_ranges > 0)) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    zr_shape_t s;
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
    return zd_ranges_stages(
        d_src, s, base, base, n_ranges, block_size, dc, stream,
        [&](dim3 grid, zxc_dev_job_t* jobs, void* gathers) {
            hipLaunchKernelGGL(zxc_rangesv_shuffle_plan_kernel, grid, dim3(256), 0, st, d_index, d_ranges, s.J, s.n_jobs, src_size, max_len,
                               block_size, (uint64_t)(uintptr_t)base, s.o_stage, jobs, (zrs_gather_t*)gathers, dc.id);
        },
        [&](dim3 grid, const uint8_t* stage, const void* gathers, const int32_t* status) {
            const auto kernel = elem_size == 2u   ? zxc_rangesv_shuffle_gather2_kernel
                                : elem_size == 4u ? zxc_rangesv_shuffle_gather4_kernel
                                                  : zxc_rangesv_shuffle_gather8_kernel;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, stage, s.slot_stride, (const zrs_gather_t*)gathers, status, s.n_jobs, s.copy_chunks,
                               base);
        },
        [&](dim3 grid, const int32_t* status) {
            hipLaunchKernelGGL(zxc_rangesv_shuffle_verdict_kernel, grid, dim3(256), 0, st, d_index, d_ranges, n_ranges, s.J, status, src_size,
                               max_len, block_size, d_results, dc.id);
        });
}

}  // extern "C"
