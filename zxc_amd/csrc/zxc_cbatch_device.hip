// zxc_cbatch_device.hip — zxc_mi355x_compress_batch_device: many independent buffers that lie in device memory compressed into
// many v8 archives in device memory by one call. The write side of zxc_batch_device.hip.
//
// zxc_mi355x_compress_device (zxc_frame_device.hip) enqueues about eight launches for one source; a source of one to sixteen
// blocks fills a sliver of the device, and a thousand of them through a thousand calls keep the host launching and planning.
// Here the host knows only n_items and the promise max_size, the item table is device data, and every item gets
// J = max(1, ceil(max_size / block_size)) jobs, of which it uses as many as it has blocks; every job has a slot of its own. The
// by-value encode entries take a contiguous source in which only the last block is short; in a batch every item ends in a short
// block, so the blocks go through the job-table entries (zxc_encode_jobs_kernel_*, zxc_encode_kernel.hip), which take each
// block's offset and length from a table. The rules are the inline C of zxc_cbatch.h on top of zxc_container.h, which the CPU tests
// run as well. The stream order of one call:
//
//   clear    jobs and sizes = 0 (a job of len 0 is unused: its wave exits at once and its size stays 0)
//   plan     one thread per item: capacity, source bounds, max_size, the known part of the archive, jobs  -> the item's record
//   images   dictionary call only, per chunk of jobs: [dict | block] images in the one image area, the jobs repointed at them
//   encode   the job-table entry of the level, once over all n_items x J jobs (dictionary call: once per chunk, behind its images)
//   finish   one thread per item: size check, archive size, capacity, block offsets, header / EOF / seek table / footer
//   gather   one wave per job: slot -> d_dst + dst_off + offset, only for an item that succeeded
//   results  d_results[r] = the item's archive size or its error
//
// No workgroup waits for another: every dependency is the stream order between launches, and every stage is predicated on the
// item's record.
//
// zxc_mi355x_compress_pack_device (rules: zxc_cpack.h) is the same call without destinations: the archives go back to back, each
// at the end of the one in front of it rounded up to `align`, so an item's place is known only behind the encoder. Clear, images,
// encode and gather are the ones above; the plan has no capacity to check, and between encode and gather stand
//
//   size     one workgroup per tile of 1024 items, four per thread: size check and archive size -> the record; the tile's extents
//            (size rounded up to align; none for an item without a size) added up -> the tile's word
//   scan     one workgroup: the tiles' words become the place of each tile's first item
//   place    one workgroup per tile: exclusive 64-bit prefix of the extents -> the record's place and the room d_dst has behind it;
//            the largest end of a sized item -> the end word (one atomic max per wavefront)
//   finish   the kernel above at that place: container bytes and block offsets, or ZXC_ERROR_DST_TOO_SMALL
//   results  d_results, d_packed (which may be d_items: nothing reads the item table behind the plan) and *d_total
//
// Here too no workgroup waits for another.
#include "zxc_device_util.h"  // copy_bytes (zxc_wave.h), zd_wg_scan64, the host-side plumbing
#include "zxc_cpack.h"        // ... and zxc_cbatch.h

static_assert(sizeof(zcb_rec_t) == ZCB_REC_BYTES && sizeof(zxc_dev_item_t) == 32, "the documented work size and item layout");
static_assert(sizeof(zxc_enc_job_t) == 16 && sizeof(zxc_enc_job_t) + 4 + 8 == ZCB_JOB_BYTES, "the documented work size per job");

// hidden entry point of zxc_hip_shim.hip (the encode launch over a job table)
extern "C" int zxc_hip_encode_jobs(const void* d_base, zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level,
                                   int with_checksum, const void* d_dict, uint32_t dict_size, void* d_images, void* d_slots,
                                   uint32_t* d_sizes, void* stream);

// ---------------------------------------------------------------- kernels
extern "C" __global__ void __launch_bounds__(256)
zxc_cbatch_plan_kernel(const zxc_dev_item_t* __restrict__ items, uint32_t n_items, uint32_t J, uint64_t src_capacity, uint64_t max_size,
                       uint64_t dst_capacity, uint32_t block_size, uint32_t checksum, uint32_t seekable, zcb_rec_t* __restrict__ recs,
                       zxc_enc_job_t* __restrict__ jobs) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    zcb_rec_t rec;
    zcb_plan_item(items[r], r, J, src_capacity, max_size, dst_capacity, block_size, (int)checksum, (int)seekable, &rec, jobs);
    recs[r] = rec;
}

extern "C" __global__ void __launch_bounds__(256)
zxc_cbatch_finish_kernel(zcb_rec_t* __restrict__ recs, uint32_t n_items, uint32_t J, const uint32_t* __restrict__ sizes,
                         uint64_t* __restrict__ offsets, const uint8_t* __restrict__ slots, uint32_t slot_stride, uint8_t* __restrict__ dst,
                         uint32_t block_size, uint32_t checksum, uint32_t seekable, const uint32_t* __restrict__ dict_id) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    const uint64_t first = (uint64_t)r * J;
    zcb_finish_item(recs + r, sizes + first, offsets + first, slots + first * slot_stride, slot_stride, dst, block_size, (int)checksum,
                    (int)seekable, dict_id != nullptr, dict_id ? *dict_id : 0u);
}

// Compaction, one wave per job: job i = r J + b is block b of item r, and its sizes[i] bytes go from its slot to the item's
// archive at offsets[i]. Only for an item whose finish succeeded: its sizes were checked (each in [8, block_size + 64]) and
// its archive fits its capacity, so nothing is written outside [dst_off, dst_off + archive size). Jobs behind an item's blocks
// and all jobs of a refused item end at once.
extern "C" __global__ void __launch_bounds__(256)
zxc_cbatch_gather_kernel(const zcb_rec_t* __restrict__ recs, uint32_t J, uint32_t n_jobs, const uint32_t* __restrict__ sizes,
                         const uint64_t* __restrict__ offsets, const uint8_t* __restrict__ slots, uint32_t slot_stride,
                         uint8_t* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    for (uint64_t i = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); i < n_jobs; i += (uint64_t)gridDim.x * waves) {
        const uint32_t r = (uint32_t)(i / J), b = (uint32_t)(i - (uint64_t)r * J);
        const zcb_rec_t* rec = recs + r;
        if (!zcb_gathers(rec, b)) continue;
        copy_bytes(dst + rec->dst_off + offsets[i], slots + i * slot_stride, sizes[i], lane, 64u);
    }
}

extern "C" __global__ void __launch_bounds__(256)
zxc_cbatch_results_kernel(const zcb_rec_t* __restrict__ recs, uint32_t n_items, int64_t* __restrict__ results) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n_items) results[r] = recs[r].result;
}

// ---------------------------------------------------------------- kernels of the pack call
extern "C" __global__ void __launch_bounds__(256)
zxc_cpack_plan_kernel(const zxc_dev_item_t* items, uint32_t n_items, uint32_t J, uint64_t src_capacity, uint64_t max_size,
                      uint32_t block_size, uint32_t checksum, uint32_t seekable, zcb_rec_t* __restrict__ recs,
                      zxc_enc_job_t* __restrict__ jobs) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    zcb_rec_t rec;
    zcp_plan_item(items[r], r, J, src_capacity, max_size, block_size, (int)checksum, (int)seekable, &rec, jobs);
    recs[r] = rec;
}

// Size and reduce, per tile: thread t sizes items r0 .. r0 + 3 of the tile and adds their extents up; tile_sum[tile] = the tile's.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_cpack_size_kernel(zcb_rec_t* __restrict__ recs, uint32_t n_items, uint32_t J, const uint32_t* __restrict__ sizes, uint32_t block_size,
                      uint32_t checksum, uint32_t seekable, uint32_t align, uint64_t* __restrict__ tile_sum) {
    const uint64_t r0 = (uint64_t)blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        if (r0 + j >= n_items) break;
        zcb_rec_t* rec = recs + r0 + j;
        zcp_size_item(rec, sizes + (r0 + j) * J, block_size, (int)checksum, (int)seekable);
        sum += zcp_extent(rec, align);
    }
    uint64_t all;
    (void)zd_wg_scan64(sum, &all);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// One workgroup: tile_sum[t] becomes the place of tile t's first item. The end word is cleared here, in front of the place pass.
extern "C" __global__ void __launch_bounds__(256)
zxc_cpack_scan_kernel(uint64_t* __restrict__ tile_sum, uint32_t n_tiles, uint64_t* __restrict__ end) {
    const uint32_t t = threadIdx.x, per = (n_tiles + 255u) / 256u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t mine = 0;
    for (uint32_t i = lo; i < hi; i++) mine += tile_sum[i];
    uint64_t all;
    uint64_t run = zd_wg_scan64(mine, &all);
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t s = tile_sum[i];
        tile_sum[i] = run;
        run += s;
    }
    if (t == 0) *end = 0;
}

// Place, per tile: the record of item r gets its place, the extents of all items in front of it added up. Ends grow with the
// place, so the largest is the last sized item's: a wavefront's largest goes into the end word with one atomic max.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_cpack_place_kernel(zcb_rec_t* __restrict__ recs, uint32_t n_items, uint32_t align, uint64_t dst_capacity,
                       const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ end) {
    const uint64_t r0 = (uint64_t)blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint64_t ext[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        ext[j] = r0 + j < n_items ? zcp_extent(recs + r0 + j, align) : 0u;
        sum += ext[j];
    }
    uint64_t all;
    uint64_t run = tile_off[blockIdx.x] + zd_wg_scan64(sum, &all);
    uint64_t last = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        if (r0 + j >= n_items) break;
        const uint64_t e = zcp_place_item(recs + r0 + j, run, dst_capacity);
        last = e > last ? e : last;
        run += ext[j];
    }
    last = wave_all(last, [](uint64_t a, uint64_t b) { return b > a ? b : a; });
    if ((threadIdx.x & 63u) == 0 && last) atomicMax((unsigned long long*)end, (unsigned long long)last);
}

// d_packed may be d_items: neither is restrict, and nothing reads the item table behind the plan.
extern "C" __global__ void __launch_bounds__(256)
zxc_cpack_results_kernel(const zcb_rec_t* __restrict__ recs, uint32_t n_items, const uint64_t* __restrict__ end, zxc_dev_item_t* packed,
                         int64_t* __restrict__ results, uint64_t* __restrict__ total) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    const zcb_rec_t rec = recs[r];
    results[r] = rec.result;
    packed[r] = zcp_packed_item(&rec);
    if (r == 0) *total = *end;
}

// ---------------------------------------------------------------- host side
namespace {

uint64_t cb_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts, uint32_t dict_size) {
    zd_copts_t o;
    zcb_shape_t s;
    if (zd_compress_opts(opts, &o) != ZXC_OK || (opts && opts->dict) || dict_size > ZC_DICT_MAX) return 0u;
    return zcb_shape(n_items, max_size, o.block_size, zxc_mi355x_encode_slot_stride(o.block_size), dict_size, &s) != 0 ? 0u : s.bytes;
}

// The encode launch over all jobs of a call; with a dictionary once per chunk, behind its images.
int cb_encode(const void* d_src, const zcb_shape_t* s, const zd_copts_t* o, const zxc_dev_dict_t* dict, zxc_enc_job_t* jobs, uint8_t* images,
              uint8_t* slots, uint32_t* sizes, void* stream) {
    if (!dict)
        return zxc_hip_encode_jobs(d_src, jobs, s->n_jobs, o->block_size, (int)o->level, (int)o->checksum, NULL, 0u, NULL, slots, sizes, stream);
    // Jobs are independent, so chunk by chunk gives the bytes of one launch over all of them. A chunk's images are built and
    // consumed in stream order before the next chunk overwrites them.
    for (uint32_t c0 = 0; c0 < s->n_jobs; c0 += s->chunk_jobs) {
        const int rc = zxc_hip_encode_jobs(d_src, jobs + c0, zcb_chunk_len(s, c0), o->block_size, (int)o->level, (int)o->checksum,
                                           dict->d_content, dict->size, images, slots + (uint64_t)c0 * s->slot_stride, sizes + c0, stream);
        if (rc != ZXC_OK) return rc;
    }
    return ZXC_OK;
}

// Both calls. dict == NULL: the call that takes no dictionary.
int cb_call(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items, uint64_t max_size, void* d_dst,
            uint64_t dst_capacity, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size,
            int64_t* d_results, void* stream) {
    if (!d_src || !d_work || !d_results || (!d_items && n_items > 0) || (!d_dst && dst_capacity > 0)) return ZXC_ERROR_NULL_INPUT;
    zd_copts_t o;
    const int orc = zd_compress_opts(opts, &o);
    if (orc != ZXC_OK) return orc;
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;  // (behind the block size, unlike the frame and append calls)
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    const uint32_t dict_size = zd_dict_of(dict).size;
    zcb_shape_t s;
    if (zcb_shape(n_items, max_size, o.block_size, zxc_mi355x_encode_slot_stride(o.block_size), dict_size, &s) != 0 || work_size < s.bytes)
        return ZXC_ERROR_MEMORY;
    if (n_items == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    uint8_t* base = zd_work_base(d_work);
    zcb_rec_t* recs = (zcb_rec_t*)(base + s.o_rec);
    zxc_enc_job_t* jobs = (zxc_enc_job_t*)(base + s.o_jobs);
    uint32_t* sizes = (uint32_t*)(base + s.o_sizes);
    uint64_t* offsets = (uint64_t*)(base + s.o_offsets);
    uint8_t* slots = base + s.o_slots;
    uint8_t* images = base + s.o_images;
    const dim3 per_item((n_items + 255u) / 256u);

    // jobs and sizes are neighbours in the work area: one clear for both
    if (hipMemsetAsync(jobs, 0, (size_t)(s.o_offsets - s.o_jobs), st) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cbatch_plan_kernel, per_item, dim3(256), 0, st, d_items, n_items, s.J, src_capacity, max_size, dst_capacity,
                       o.block_size, o.checksum, o.seekable, recs, jobs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const int erc = cb_encode(d_src, &s, &o, dict, jobs, images, slots, sizes, stream);
    if (erc != ZXC_OK) return erc;
    hipLaunchKernelGGL(zxc_cbatch_finish_kernel, per_item, dim3(256), 0, st, recs, n_items, s.J, (const uint32_t*)sizes, offsets,
                       (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst, o.block_size, o.checksum, o.seekable,
                       zd_dict_of(dict).id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint32_t groups = (s.n_jobs + 3u) / 4u < 65536u ? (s.n_jobs + 3u) / 4u : 65536u;
    hipLaunchKernelGGL(zxc_cbatch_gather_kernel, dim3(groups), dim3(256), 0, st, (const zcb_rec_t*)recs, s.J, s.n_jobs, (const uint32_t*)sizes,
                       (const uint64_t*)offsets, (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cbatch_results_kernel, per_item, dim3(256), 0, st, (const zcb_rec_t*)recs, n_items, d_results);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

uint64_t cp_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts, uint32_t dict_size) {
    zd_copts_t o;
    zcp_shape_t s;
    if (zd_compress_opts(opts, &o) != ZXC_OK || (opts && opts->dict) || dict_size > ZC_DICT_MAX) return 0u;
    return zcp_shape(n_items, max_size, o.block_size, zxc_mi355x_encode_slot_stride(o.block_size), dict_size, &s) != 0 ? 0u : s.bytes;
}

// Both pack calls. dict == NULL: the call that takes no dictionary.
int cp_call(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items, uint64_t max_size, void* d_dst,
            uint64_t dst_capacity, uint32_t align, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
            uint64_t work_size, zxc_dev_item_t* d_packed, int64_t* d_results, uint64_t* d_total, void* stream) {
    if (!d_src || !d_work || !d_results || !d_packed || !d_total || (!d_items && n_items > 0) || (!d_dst && dst_capacity > 0))
        return ZXC_ERROR_NULL_INPUT;
    zd_copts_t o;
    const int orc = zd_compress_opts(opts, &o);
    if (orc != ZXC_OK) return orc;
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if (!zcp_align_ok(align)) return ZXC_ERROR_GPU_UNSUPPORTED;
    zcp_shape_t p;
    if (zcp_shape(n_items, max_size, o.block_size, zxc_mi355x_encode_slot_stride(o.block_size), zd_dict_of(dict).size, &p) != 0 ||
        work_size < p.bytes)
        return ZXC_ERROR_MEMORY;
    if (n_items == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const zcb_shape_t& s = p.b;
    uint8_t* base = zd_work_base(d_work);
    zcb_rec_t* recs = (zcb_rec_t*)(base + s.o_rec);
    zxc_enc_job_t* jobs = (zxc_enc_job_t*)(base + s.o_jobs);
    uint32_t* sizes = (uint32_t*)(base + s.o_sizes);
    uint64_t* offsets = (uint64_t*)(base + s.o_offsets);
    uint8_t* slots = base + s.o_slots;
    uint8_t* images = base + s.o_images;
    uint64_t* tiles = (uint64_t*)(base + p.o_tiles);
    uint64_t* end = (uint64_t*)(base + p.o_end);
    const dim3 per_item((n_items + 255u) / 256u), per_tile(p.n_tiles);

    if (hipMemsetAsync(jobs, 0, (size_t)(s.o_offsets - s.o_jobs), st) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cpack_plan_kernel, per_item, dim3(256), 0, st, d_items, n_items, s.J, src_capacity, max_size, o.block_size,
                       o.checksum, o.seekable, recs, jobs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const int erc = cb_encode(d_src, &s, &o, dict, jobs, images, slots, sizes, stream);
    if (erc != ZXC_OK) return erc;
    hipLaunchKernelGGL(zxc_cpack_size_kernel, per_tile, dim3(ZD_TILE_THREADS), 0, st, recs, n_items, s.J, (const uint32_t*)sizes, o.block_size,
                       o.checksum, o.seekable, align, tiles);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cpack_scan_kernel, dim3(1), dim3(256), 0, st, tiles, p.n_tiles, end);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cpack_place_kernel, per_tile, dim3(ZD_TILE_THREADS), 0, st, recs, n_items, align, dst_capacity,
                       (const uint64_t*)tiles, end);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cbatch_finish_kernel, per_item, dim3(256), 0, st, recs, n_items, s.J, (const uint32_t*)sizes, offsets,
                       (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst, o.block_size, o.checksum, o.seekable,
                       zd_dict_of(dict).id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint32_t groups = (s.n_jobs + 3u) / 4u < 65536u ? (s.n_jobs + 3u) / 4u : 65536u;
    hipLaunchKernelGGL(zxc_cbatch_gather_kernel, dim3(groups), dim3(256), 0, st, (const zcb_rec_t*)recs, s.J, s.n_jobs, (const uint32_t*)sizes,
                       (const uint64_t*)offsets, (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cpack_results_kernel, per_item, dim3(256), 0, st, (const zcb_rec_t*)recs, n_items, (const uint64_t*)end, d_packed,
                       d_results, d_total);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_compress_batch_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts) {
    return cb_work_size(n_items, max_size, opts, 0u);
}

int zxc_mi355x_compress_batch_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                     uint64_t max_size, void* d_dst, uint64_t dst_capacity, const zxc_compress_opts_t* opts, void* d_work,
                                     uint64_t work_size, int64_t* d_results, void* stream) {
    return cb_call(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, opts, NULL, d_work, work_size, d_results, stream);
}

uint64_t zxc_mi355x_compress_batch_dict_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts,
                                                         uint32_t dict_size) {
    return cb_work_size(n_items, max_size, opts, dict_size);
}

int zxc_mi355x_compress_batch_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                          uint64_t max_size, void* d_dst, uint64_t dst_capacity, const zxc_compress_opts_t* opts,
                                          const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_results, void* stream) {
    return cb_call(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, opts, dict, d_work, work_size, d_results, stream);
}

uint64_t zxc_mi355x_compress_pack_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts) {
    return cp_work_size(n_items, max_size, opts, 0u);
}

int zxc_mi355x_compress_pack_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                    uint64_t max_size, void* d_dst, uint64_t dst_capacity, uint32_t align, const zxc_compress_opts_t* opts,
                                    void* d_work, uint64_t work_size, zxc_dev_item_t* d_packed, int64_t* d_results, uint64_t* d_total,
                                    void* stream) {
    return cp_call(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align, opts, NULL, d_work, work_size, d_packed,
                   d_results, d_total, stream);
}

uint64_t zxc_mi355x_compress_pack_dict_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts,
                                                        uint32_t dict_size) {
    return cp_work_size(n_items, max_size, opts, dict_size);
}

int zxc_mi355x_compress_pack_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                         uint64_t max_size, void* d_dst, uint64_t dst_capacity, uint32_t align,
                                         const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size,
                                         zxc_dev_item_t* d_packed, int64_t* d_results, uint64_t* d_total, void* stream) {
    return cp_call(d_src, src_capacity, d_items, n_items, max_size, d_dst, dst_capacity, align, opts, dict, d_work, work_size, d_packed,
                   d_results, d_total, stream);
}

}  // extern "C"
