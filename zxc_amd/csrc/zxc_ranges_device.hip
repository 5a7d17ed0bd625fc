// zxc_ranges_device.hip — zxc_mi355x_seekable_open_device and zxc_mi355x_decompress_ranges_device: random access into a seekable
// v8 archive that lies in device memory, results into device memory.
//
// The device-resident counterpart of zxc_seekable_open + zxc_seekable_decompress_range (zxc_host.c), batched: one range of a few
// blocks cannot fill the device, a few thousand can. The rules are the inline C of zxc_ranges.h, which the CPU tests run as well.
//
// open, once per archive, in stream order:
//   head     file header, footer, SEK and EOF headers                                      -> index header, status < 0
//   tiles    per tile of 1024 entries: their sum and whether one is implausible, left in comp_offsets[first block of the tile]
//   scan     one workgroup: those words become the tiles' archive offsets; the entries must sum from 16 to the EOF block -> status 0
//   scatter  per tile: comp_offsets[b] for its blocks (the tile's first block is the word the scan left), [nb] behind the last
//
// ranges, per call, in stream order (the ranges are device data: the host only knows n_ranges and max_len, so it launches
// J = (max_len - 1) / block_size + 2 jobs per range, of which a range uses as many as it covers blocks):
//   plan     one thread per job: validates its range, writes the job and the copy descriptor
//   decode   the existing decode launch, once, over all jobs: one d_out base below both d_dst and the staged slots
//   copy     staged slot -> d_dst, one wavefront per 8 KiB of destination
//   verdict  one thread per range: d_results[r]
//
// No workgroup waits for another: every dependency is the stream order between launches, and every stage is predicated on the index
// status and the range's own verdict.
//
// zxc_mi355x_decompress_ranges_dict_device is the ranges call with a dictionary in device memory: plan and verdict compare the
// index's dictionary id with the word zxc_mi355x_dict_prepare_device wrote, and the decode launch gets the dictionary.
//
// zxc_mi355x_decompress_rangesv_device (and _dict) is the ranges call over a table whose entries carry the absolute device address
// of their destination (zxc_rangesv.h). The decode launch's d_out and the copy's destination base are the work area's 256-byte
// aligned base, and every place outside the work area is counted from it modulo 2^64, so the decode kernels and
// zxc_ranges_copy_kernel run as they are.
//
// One rule set, three front ends: ranges and rangesv here, the shuffled ranges in zxc_rangesv_shuffle_device.hip. The rules of
// zxc_ranges.h are written over a normalised request (zr_req_t) that each front end builds of its table entry; the plan and verdict
// kernels are instantiations of zd_ranges_plan / zd_ranges_verdict, and zd_ranges_stages (zxc_device_util.h) enqueues the four
// stages for every entry point, behind that entry point's own synchronous checks.
#include "zxc_device_util.h"  // the tile passes, the ranges family's kernel bodies and stages, the host-side plumbing
#include "zxc_rangesv.h"      // on top of zxc_ranges.h

#define RNG_BAD (1ull << 63)  // in a tile's word: one of its entries is implausible (a tile's sum is <= 2^32)

__device__ __forceinline__ v4u rng_ld128(const uint8_t* p) { v4u v; __builtin_memcpy(&v, p, 16); return v; }  // any alignment

// ---------------------------------------------------------------- open
extern "C" __global__ void __launch_bounds__(64)
zxc_seekidx_head_kernel(const uint8_t* __restrict__ src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, zr_index_t* __restrict__ ix) {
    if (threadIdx.x == 0) zr_open_head(src, src_size, block_size, max_blocks, ix);
}

// Tile t covers entries [t * ZC_TILE_BLOCKS, ...), ZD_PER_THREAD consecutive entries per thread. Every tile of the grid writes its
// word, also those behind the table (t * ZC_TILE_BLOCKS <= max_blocks: inside the index).
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_seekidx_tiles_kernel(const uint8_t* __restrict__ src, const zr_index_t* __restrict__ ix, uint64_t* __restrict__ offs) {
    if (ix->seek != 1u) return;
    const uint32_t t = threadIdx.x, nb = ix->nb;
    const uint8_t* ent = zr_entries(src, ix);
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + t * ZD_PER_THREAD;
    uint32_t sum = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        const uint32_t e = zc_rd32(ent + 4ull * b);
        if (zr_entry_ok(e)) sum += e;
        else bad = 1u;
    }
    const zd_totals tile = zd_tile_reduce(sum, 0u, bad);
    if (t == 0) offs[(uint64_t)blockIdx.x * ZC_TILE_BLOCKS] = tile.sum | (tile.bad ? RNG_BAD : 0ull);
}

// One workgroup. Tile t's word becomes the archive offset of its first block (exclusive prefix + 16, in place); the table is
// accepted only when no entry was implausible and the entries sum exactly to the EOF block the head stage found.
extern "C" __global__ void __launch_bounds__(256)
zxc_seekidx_scan_kernel(uint64_t* __restrict__ offs, uint32_t n_tiles, zr_index_t* __restrict__ ix) {
    if (ix->seek != 1u) return;
    const zd_totals all = zd_scan_tiles(  // (behind its barrier every thread has read ix->seek)
        n_tiles, ZC_FILE_HDR,
        [=](uint32_t i, uint32_t&, uint32_t& bad) {
            const uint64_t w = offs[(uint64_t)i * ZC_TILE_BLOCKS];
            bad |= (uint32_t)(w >> 63);
            return w & ~RNG_BAD;
        },
        [=](uint32_t i, uint64_t off) { offs[(uint64_t)i * ZC_TILE_BLOCKS] = off; });
    if (threadIdx.x == 0) zr_open_judge(ix, (int)all.bad, all.sum);
}

// Per tile: block b's offset is the prefix sum of the entries. Every entry is plausible and the sum was checked, so every offset
// lies in front of the EOF block.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_seekidx_scatter_kernel(const uint8_t* __restrict__ src, const zr_index_t* __restrict__ ix, uint64_t* __restrict__ offs) {
    if (ix->seek != 2u) return;
    const uint32_t t = threadIdx.x, nb = ix->nb;
    if ((uint64_t)blockIdx.x * ZC_TILE_BLOCKS >= nb) return;  // (a tile behind the table; [nb] is written by the last block's thread)
    const uint8_t* ent = zr_entries(src, ix);
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + t * ZD_PER_THREAD;
    uint32_t e[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        e[j] = b0 + j < nb ? zc_rd32(ent + 4ull * (b0 + j)) : 0u;
        sum += e[j];
    }
    // (thread 0 writes its first block's offset over the tile's word: the same value, so a thread reads the right one either way)
    uint64_t run = zd_tile_offset(sum, offs[(uint64_t)blockIdx.x * ZC_TILE_BLOCKS]);
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        offs[b] = run;
        run += e[j];
        if (b + 1u == nb) offs[nb] = run;
    }
}

// ---------------------------------------------------------------- ranges
extern "C" __global__ void __launch_bounds__(256)
zxc_ranges_plan_kernel(const void* __restrict__ index, const zxc_dev_range_t* __restrict__ ranges, uint32_t J, uint32_t n_jobs,
                       uint64_t src_size, uint64_t max_len, uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel,
                       zxc_dev_job_t* __restrict__ jobs, zr_copy_t* __restrict__ copies, const uint32_t* __restrict__ dict_id) {
    zd_ranges_plan(ranges, J, n_jobs, jobs, copies, [=](zxc_dev_range_t r, uint32_t j, uint32_t i, zxc_dev_job_t* job, zr_copy_t* cp) {
        zr_job_dict(index, r, j, i, src_size, max_len, dst_capacity, block_size, dst_rel, stage_rel, dict_id != nullptr, dict_id ? *dict_id : 0u, job, cp);
    });
}

// One wavefront per item = (job, chunk): chunk k of a job is the part of its copy whose destination addresses lie in
// [A + k CHUNK, A + (k + 1) CHUNK), A = the copy's destination rounded down to 16. A lane moves 16-byte units of the destination:
// an aligned 16-byte store fed by a 16-byte load of any alignment from the slot, bytes where the unit passes the copy's ends.
// Most items are empty (direct and empty jobs, chunks behind a short copy) and end at once.
extern "C" __global__ void __launch_bounds__(256)
zxc_ranges_copy_kernel(const uint8_t* __restrict__ stage, uint32_t slot_stride, const zr_copy_t* __restrict__ copies,
                       const int32_t* __restrict__ status, uint32_t n_jobs, uint32_t chunks, uint8_t* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t items = (uint64_t)n_jobs * chunks, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < items; it += waves) {
        const uint32_t i = (uint32_t)(it / chunks), k = (uint32_t)(it - (uint64_t)i * chunks);
        const zr_copy_t cp = copies[i];
        if (cp.n == 0 || (uint64_t)k * ZR_COPY_CHUNK >= (cp.dst_at & 15u) + cp.n) continue;
        const int32_t st = status[i];
        if (st < 0 || (uint32_t)st < cp.from + cp.n) continue;  // (the range fails: its bytes are undefined, nothing is copied)
        const uint8_t* s = stage + (uint64_t)i * slot_stride + cp.from;
        uint8_t* d = dst + cp.dst_at;
        const int64_t n = (int64_t)cp.n;
        // rel: position in the copy of this lane's first unit (negative in front of the head)
        int64_t rel = (int64_t)k * ZR_COPY_CHUNK - (int64_t)(cp.dst_at & 15u) + 16 * (int64_t)lane;
#pragma unroll 4
        for (uint32_t u = 0; u < ZR_COPY_CHUNK / 1024u; u++, rel += 1024) {
            if (rel >= n) break;
            if (rel >= 0 && rel + 16 <= n) {
                *(v4u*)(d + rel) = rng_ld128(s + rel);
            } else {
                const int64_t lo = rel < 0 ? 0 : rel, hi = rel + 16 < n ? rel + 16 : n;
                for (int64_t b = lo; b < hi; b++) d[b] = s[b];
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(256)
zxc_ranges_verdict_kernel(const void* __restrict__ index, const zxc_dev_range_t* __restrict__ ranges, uint32_t n_ranges, uint32_t J,
                          const int32_t* __restrict__ status, uint64_t src_size, uint64_t max_len, uint64_t dst_capacity, uint32_t block_size,
                          int64_t* __restrict__ results, const uint32_t* __restrict__ dict_id) {
    zd_ranges_verdict(ranges, n_ranges, J, status, results, [=](zxc_dev_range_t r, const int32_t* st) {
        return zr_verdict_dict(index, r, J, st, src_size, max_len, dst_capacity, block_size, dict_id != nullptr, dict_id ? *dict_id : 0u);
    });
}

// ---------------------------------------------------------------- rangesv
extern "C" __global__ void __launch_bounds__(256)
zxc_rangesv_plan_kernel(const void* __restrict__ index, const zxc_dev_rangev_t* __restrict__ ranges, uint32_t J, uint32_t n_jobs,
                        uint64_t src_size, uint64_t max_len, uint32_t block_size, uint64_t out_base, uint64_t stage_rel,
                        zxc_dev_job_t* __restrict__ jobs, zr_copy_t* __restrict__ copies, const uint32_t* __restrict__ dict_id) {
    zd_ranges_plan(ranges, J, n_jobs, jobs, copies, [=](zxc_dev_rangev_t r, uint32_t j, uint32_t i, zxc_dev_job_t* job, zr_copy_t* cp) {
        zrv_job(index, r, j, i, src_size, max_len, block_size, out_base, stage_rel, dict_id != nullptr, dict_id ? *dict_id : 0u, job, cp);
    });
}

extern "C" __global__ void __launch_bounds__(256)
zxc_rangesv_verdict_kernel(const void* __restrict__ index, const zxc_dev_rangev_t* __restrict__ ranges, uint32_t n_ranges, uint32_t J,
                           const int32_t* __restrict__ status, uint64_t src_size, uint64_t max_len, uint32_t block_size,
                           int64_t* __restrict__ results, const uint32_t* __restrict__ dict_id) {
    zd_ranges_verdict(ranges, n_ranges, J, status, results, [=](zxc_dev_rangev_t r, const int32_t* st) {
        return zrv_verdict(index, r, J, st, src_size, max_len, block_size, dict_id != nullptr, dict_id ? *dict_id : 0u);
    });
}

// ---------------------------------------------------------------- host side
extern "C" {

uint64_t zxc_mi355x_seekable_index_size(uint32_t max_blocks) { return zr_index_size(max_blocks); }

int zxc_mi355x_seekable_open_device(const void* d_src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* d_index,
                                    uint64_t index_size, void* stream) {
    if (!d_src || !d_index) return ZXC_ERROR_NULL_INPUT;
    if (src_size < ZR_OPEN_MIN) return ZXC_ERROR_SRC_TOO_SMALL;
    if (!zc_block_size_ok(block_size)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if ((uintptr_t)d_index & 15u) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (index_size < zr_index_size(max_blocks)) return ZXC_ERROR_MEMORY;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = (const uint8_t*)d_src;
    zr_index_t* ix = (zr_index_t*)d_index;
    uint64_t* offs = zr_offsets(d_index);
    const uint32_t n_tiles = zr_open_tiles(max_blocks);
    hipLaunchKernelGGL(zxc_seekidx_head_kernel, dim3(1), dim3(64), 0, st, src, src_size, block_size, max_blocks, ix);
    hipLaunchKernelGGL(zxc_seekidx_tiles_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, src, (const zr_index_t*)ix, offs);
    hipLaunchKernelGGL(zxc_seekidx_scan_kernel, dim3(1), dim3(256), 0, st, offs, n_tiles, ix);
    hipLaunchKernelGGL(zxc_seekidx_scatter_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, src, (const zr_index_t*)ix, offs);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

uint64_t zxc_mi355x_decompress_ranges_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size) {
    zr_shape_t s;
    return zr_shape(n_ranges, max_len, block_size, &s) != 0 ? 0u : s.bytes;
}

// The copy-out launch of ranges and rangesv, as zd_ranges_stages takes it: the staged slots -> dst + dst_at.
static auto copy_out(const zr_shape_t& s, uint8_t* dst, hipStream_t st) {
    return [&s, dst, st](dim3 grid, const uint8_t* stage, const void* copies, const int32_t* status) {
        hipLaunchKernelGGL(zxc_ranges_copy_kernel, grid, dim3(256), 0, st, stage, s.slot_stride, (const zr_copy_t*)copies, status, s.n_jobs,
                           s.copy_chunks, dst);
    };
}

// Both calls. dict == NULL: the call that takes no dictionary.
static int ranges_call(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_range_t* d_ranges, uint32_t n_ranges,
                       uint64_t max_len, void* d_dst, uint64_t dst_capacity, uint32_t block_size, const zxc_dev_dict_t* dict, void* d_work,
                       uint64_t work_size, int64_t* d_results, void* stream) {
    if (!d_src || !d_index || !d_work || !d_results || (!d_ranges && n_ranges > 0) || (!d_dst && dst_capacity > 0)) return ZXC_ERROR_NULL_INPUT;
    zr_shape_t s;
    const int shape_rc = zr_shape(n_ranges, max_len, block_size, &s);
    if (shape_rc == ZXC_ERROR_BAD_BLOCK_SIZE) return shape_rc;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if ((uintptr_t)d_dst & 15u) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (shape_rc != 0 || work_size < s.bytes) return ZXC_ERROR_MEMORY;
    if (n_ranges == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const zd_dict_t dc = zd_dict_of(dict);
    uint8_t* base = zd_work_base(d_work);
    uint64_t dst_rel, stage_rel;
    uint8_t* out = zd_out_base(d_dst, base + s.o_stage, &dst_rel, &stage_rel);
    return zd_ranges_stages(
        d_src, s, base, out, n_ranges, block_size, dc, stream,
        [&](dim3 grid, zxc_dev_job_t* jobs, void* copies) {
            hipLaunchKernelGGL(zxc_ranges_plan_kernel, grid, dim3(256), 0, st, d_index, d_ranges, s.J, s.n_jobs, src_size, max_len, dst_capacity,
                               block_size, dst_rel, stage_rel, jobs, (zr_copy_t*)copies, dc.id);
        },
        copy_out(s, (uint8_t*)d_dst, st),
        [&](dim3 grid, const int32_t* status) {
            hipLaunchKernelGGL(zxc_ranges_verdict_kernel, grid, dim3(256), 0, st, d_index, d_ranges, n_ranges, s.J, status, src_size, max_len,
                               dst_capacity, block_size, d_results, dc.id);
        });
}

int zxc_mi355x_decompress_ranges_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_range_t* d_ranges,
                                        uint32_t n_ranges, uint64_t max_len, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                        void* d_work, uint64_t work_size, int64_t* d_results, void* stream) {
    return ranges_call(d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity, block_size, NULL, d_work, work_size, d_results,
                       stream);
}

int zxc_mi355x_decompress_ranges_dict_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_range_t* d_ranges,
                                             uint32_t n_ranges, uint64_t max_len, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                             const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_results, void* stream) {
    return ranges_call(d_src, src_size, d_index, d_ranges, n_ranges, max_len, d_dst, dst_capacity, block_size, dict, d_work, work_size, d_results,
                       stream);
}

uint64_t zxc_mi355x_decompress_rangesv_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size) {
    return zxc_mi355x_decompress_ranges_device_work_size(n_ranges, max_len, block_size);
}

// Both rangesv calls. dict == NULL: the call that takes no dictionary. The copy's destinations are counted from the work area's
// base, as the jobs' places are: zxc_ranges_copy_kernel adds cp.dst_at to the pointer it is given in 64 bits, and the base being a
// multiple of 16 keeps dst_at & 15 the address's alignment.
static int rangesv_call(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_rangev_t* d_ranges, uint32_t n_ranges,
                        uint64_t max_len, uint32_t block_size, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_results,
                        void* stream) {
    if (!d_src || !d_index || !d_work || !d_results || (!d_ranges && n_ranges > 0)) return ZXC_ERROR_NULL_INPUT;
    zr_shape_t s;
    const int shape_rc = zr_shape(n_ranges, max_len, block_size, &s);
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
        [&](dim3 grid, zxc_dev_job_t* jobs, void* copies) {
            hipLaunchKernelGGL(zxc_rangesv_plan_kernel, grid, dim3(256), 0, st, d_index, d_ranges, s.J, s.n_jobs, src_size, max_len, block_size,
                               (uint64_t)(uintptr_t)base, s.o_stage, jobs, (zr_copy_t*)copies, dc.id);
        },
        copy_out(s, base, st),
        [&](dim3 grid, const int32_t* status) {
            hipLaunchKernelGGL(zxc_rangesv_verdict_kernel, grid, dim3(256), 0, st, d_index, d_ranges, n_ranges, s.J, status, src_size, max_len,
                               block_size, d_results, dc.id);
        });
}

int zxc_mi355x_decompress_rangesv_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_rangev_t* d_ranges,
                                         uint32_t n_ranges, uint64_t max_len, uint32_t block_size, void* d_work, uint64_t work_size,
                                         int64_t* d_results, void* stream) {
    return rangesv_call(d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size, NULL, d_work, work_size, d_results, stream);
}

int zxc_mi355x_decompress_rangesv_dict_device(const void* d_src, uint64_t src_size, const void* d_index, const zxc_dev_rangev_t* d_ranges,
                                              uint32_t n_ranges, uint64_t max_len, uint32_t block_size, const zxc_dev_dict_t* dict, void* d_work,
                                              uint64_t work_size, int64_t* d_results, void* stream) {
    return rangesv_call(d_src, src_size, d_index, d_ranges, n_ranges, max_len, block_size, dict, d_work, work_size, d_results, stream);
}

}  // extern "C"
