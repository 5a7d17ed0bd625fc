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
#include "zxc_device_util.h"  // copy_bytes (zxc_wave.h), the host-side plumbing
#include "zxc_cbatch.h"

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

// ---------------------------------------------------------------- host side
namespace {

uint64_t cb_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts, uint32_t dict_size) {
    zd_copts_t o;
    zcb_shape_t s;
    if (zd_compress_opts(opts, &o) != ZXC_OK || (opts && opts->dict) || dict_size > ZC_DICT_MAX) return 0u;
    return zcb_shape(n_items, max_size, o.block_size, zxc_mi355x_encode_slot_stride(o.block_size), dict_size, &s) != 0 ? 0u : s.bytes;
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
    const uint32_t dict_size = dict ? dict->size : 0u;
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
    if (dict) {
        // Jobs are independent, so chunk by chunk gives the bytes of one launch over all of them. A chunk's images are built and
        // consumed in stream order before the next chunk overwrites them.
        for (uint32_t c0 = 0; c0 < s.n_jobs; c0 += s.chunk_jobs) {
            const int rc = zxc_hip_encode_jobs(d_src, jobs + c0, zcb_chunk_len(&s, c0), o.block_size, (int)o.level, (int)o.checksum,
                                               dict->d_content, dict_size, images, slots + (uint64_t)c0 * s.slot_stride, sizes + c0, stream);
            if (rc != ZXC_OK) return rc;
        }
    } else {
        const int rc = zxc_hip_encode_jobs(d_src, jobs, s.n_jobs, o.block_size, (int)o.level, (int)o.checksum, NULL, 0u, NULL, slots, sizes,
                                           stream);
        if (rc != ZXC_OK) return rc;
    }
    hipLaunchKernelGGL(zxc_cbatch_finish_kernel, per_item, dim3(256), 0, st, recs, n_items, s.J, (const uint32_t*)sizes, offsets,
                       (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst, o.block_size, o.checksum, o.seekable,
                       dict ? dict->d_id : (const uint32_t*)NULL);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint32_t groups = (s.n_jobs + 3u) / 4u < 65536u ? (s.n_jobs + 3u) / 4u : 65536u;
    hipLaunchKernelGGL(zxc_cbatch_gather_kernel, dim3(groups), dim3(256), 0, st, (const zcb_rec_t*)recs, s.J, s.n_jobs, (const uint32_t*)sizes,
                       (const uint64_t*)offsets, (const uint8_t*)slots, s.slot_stride, (uint8_t*)d_dst);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_cbatch_results_kernel, per_item, dim3(256), 0, st, (const zcb_rec_t*)recs, n_items, d_results);
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

}  // extern "C"
