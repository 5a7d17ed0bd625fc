// zxc_batch_device.hip — zxc_mi355x_decompress_batch_device: many independent v8 archives that lie in device memory decoded into
// device memory by one call.
//
// zxc_mi355x_decompress_device (zxc_unframe_device.hip) enqueues about ten launches of a few workgroups for one archive; an archive
// of one to sixteen blocks cannot fill the device, and a thousand of them through a thousand calls keep the host launching. Here
// the host knows only n_items and the promise max_capacity, the item table is device data, and the call has the shape of
// zxc_mi355x_decompress_ranges_device: J = ceil(max_capacity / block_size) + 1 jobs per item, of which an item uses as many as
// it has blocks, and every job has a staged slot of its own. The rules are the inline C of zxc_batch.h on top of zxc_container.h,
// which the CPU tests run as well. The stream order of one call:
//
//   clear    both job tables = 0 (a job of size 0 is answered with an error status, nothing is read or written for it)
//   plan     one thread per item: capacity, source bounds, head, header walk, jobs, global hash            -> the item's record
//   decode   the existing decode launch once per table over all n_items x J jobs: one d_out base below both d_dst and the slots
//   copy     staged slot -> d_dst, one wavefront per 8 KiB of destination
//   verdict  one thread per item: d_results[r]
//
// No workgroup waits for another: every dependency is the stream order between launches, and every stage is predicated on the
// item's record. Whether an item's blocks carry checksum trailers is known on the device only, and the decode launch takes it by
// value: a call that asks for verification decodes two job tables, one with verify_trailer = 1 and one without, and the plan
// puts an item's jobs into the one its header picks (rec.c.sel); its entries of the other stay empty.
//
// zxc_mi355x_decompress_batch_dict_device is the same call with one dictionary in device memory for the whole batch: the plan
// compares each header's dictionary id with the word zxc_mi355x_dict_prepare_device wrote, and the decode launches get the
// dictionary.
#include "zxc_device_util.h"  // the copy, the host-side plumbing
#include "zxc_batch.h"

static_assert(ZB_COPY_CHUNK == ZD_COPY_CHUNK, "the shape counts the chunks zd_copy_chunk moves");
static_assert(sizeof(zb_rec_t) == ZB_REC_BYTES && sizeof(zxc_dev_item_t) == 32, "the documented work size and item layout");

// ---------------------------------------------------------------- kernels
extern "C" __global__ void __launch_bounds__(256)
zxc_batch_plan_kernel(const uint8_t* __restrict__ src, uint64_t src_capacity, const zxc_dev_item_t* __restrict__ items, uint32_t n_items,
                      uint32_t J, uint32_t n_jobs, uint64_t max_capacity, uint64_t dst_capacity, uint32_t block_size, uint32_t want_verify,
                      uint64_t dst_rel, uint64_t stage_rel, zb_rec_t* __restrict__ recs, zxc_dev_job_t* __restrict__ jobs,
                      const uint32_t* __restrict__ dict_id) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    zb_rec_t rec;
    zb_plan_item(src, src_capacity, items[r], r, J, n_jobs, max_capacity, dst_capacity, block_size, (int)want_verify, dst_rel, stage_rel,
                 dict_id != nullptr, dict_id ? *dict_id : 0u, &rec, jobs);
    recs[r] = rec;
}

// One wavefront per (job, chunk), as in zxc_ranges_copy_kernel: job i = r J + b is block b of item r, and its copy is
// min(decoded size, capacity left) bytes from its slot to d_dst + dst_off + b block_size. Most are empty (jobs behind an item's
// blocks, blocks decoded straight into d_dst, chunks behind a short copy) and end at once.
extern "C" __global__ void __launch_bounds__(256)
zxc_batch_copy_kernel(const uint8_t* __restrict__ stage, uint32_t slot_stride, const zb_rec_t* __restrict__ recs,
                      const int32_t* __restrict__ status, uint32_t J, uint32_t n_jobs, uint32_t chunks, uint32_t block_size,
                      uint8_t* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t units = (uint64_t)n_jobs * chunks, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < units; it += waves) {
        const uint32_t i = (uint32_t)(it / chunks), k = (uint32_t)(it - (uint64_t)i * chunks);
        const uint32_t r = i / J, b = i - r * J;
        const zb_rec_t* rec = recs + r;
        if (rec->c.final || b >= rec->c.found) continue;
        const uint32_t n = zb_copy_bytes(rec, b, status[(uint64_t)rec->c.sel * n_jobs + i], block_size);
        const uint64_t dst_at = rec->dst_off + (uint64_t)b * block_size;
        if (n == 0 || (uint64_t)k * ZB_COPY_CHUNK >= (dst_at & 15u) + n) continue;
        zd_copy_chunk(dst + dst_at, stage + (uint64_t)i * slot_stride, (int64_t)n, k, lane);
    }
}

extern "C" __global__ void __launch_bounds__(256)
zxc_batch_verdict_kernel(const zb_rec_t* __restrict__ recs, uint32_t n_items, uint32_t J, uint32_t n_jobs,
                         const int32_t* __restrict__ status, uint32_t block_size, int64_t* __restrict__ results) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_items) return;
    const zb_rec_t* rec = recs + r;
    results[r] = zb_verdict_item(rec, status + (uint64_t)rec->c.sel * n_jobs + (uint64_t)r * J, block_size);
}

// ---------------------------------------------------------------- host side
extern "C" {

uint64_t zxc_mi355x_decompress_batch_device_work_size(uint32_t n_items, uint64_t max_capacity, uint32_t block_size) {
    zb_shape_t s;
    return zb_shape(n_items, max_capacity, block_size, &s) != 0 ? 0u : s.bytes;
}

// Both calls. dict == NULL: the call that takes no dictionary.
static int batch_call(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items, uint64_t max_capacity,
                      void* d_dst, uint64_t dst_capacity, uint32_t block_size, const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict,
                      void* d_work, uint64_t work_size, int64_t* d_results, void* stream) {
    if (!d_src || !d_work || !d_results || (!d_items && n_items > 0) || (!d_dst && dst_capacity > 0)) return ZXC_ERROR_NULL_INPUT;
    zb_shape_t s;
    const int shape_rc = zb_shape(n_items, max_capacity, block_size, &s);
    if (shape_rc == ZXC_ERROR_BAD_BLOCK_SIZE) return shape_rc;
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if ((uintptr_t)d_dst & 15u) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (shape_rc != 0 || work_size < s.bytes) return ZXC_ERROR_MEMORY;
    if (n_items == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    const uint32_t want_verify = (opts && opts->checksum_enabled) ? 1u : 0u, tables = 1u + want_verify;
    uint8_t* base = zd_work_base(d_work);
    zb_rec_t* recs = (zb_rec_t*)(base + s.o_rec);
    zxc_dev_job_t* jobs = (zxc_dev_job_t*)(base + s.o_jobs);
    int32_t* status = (int32_t*)(base + s.o_status);
    uint8_t* stage = base + s.o_stage;
    uint64_t dst_rel, stage_rel;
    uint8_t* out = zd_out_base(d_dst, stage, &dst_rel, &stage_rel);
    const zd_dict_t dc = zd_dict_of(dict);

    if (hipMemsetAsync(jobs, 0, 2u * (size_t)s.n_jobs * sizeof(zxc_dev_job_t), st) != hipSuccess) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_batch_plan_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, st, (const uint8_t*)d_src, src_capacity, d_items,
                       n_items, s.J, s.n_jobs, max_capacity, dst_capacity, block_size, want_verify, dst_rel, stage_rel, recs, jobs, dc.id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const int rc = zd_decode_tables(d_src, jobs, s.n_jobs, s.n_jobs, out, status, s.n_jobs, block_size, tables, dc, stream);
    if (rc != ZXC_OK) return rc;
    hipLaunchKernelGGL(zxc_batch_copy_kernel, zd_copy_grid((uint64_t)s.n_jobs * s.copy_chunks), dim3(256), 0, st, (const uint8_t*)stage,
                       s.slot_stride, (const zb_rec_t*)recs, (const int32_t*)status, s.J, s.n_jobs, s.copy_chunks, block_size, (uint8_t*)d_dst);
    hipLaunchKernelGGL(zxc_batch_verdict_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, st, (const zb_rec_t*)recs, n_items, s.J,
                       s.n_jobs, (const int32_t*)status, block_size, d_results);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int zxc_mi355x_decompress_batch_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                       uint64_t max_capacity, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                       const zxc_decompress_opts_t* opts, void* d_work, uint64_t work_size, int64_t* d_results,
                                       void* stream) {
    return batch_call(d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity, block_size, opts, NULL, d_work, work_size,
                      d_results, stream);
}

int zxc_mi355x_decompress_batch_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items, uint32_t n_items,
                                            uint64_t max_capacity, void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                            const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size,
                                            int64_t* d_results, void* stream) {
    return batch_call(d_src, src_capacity, d_items, n_items, max_capacity, d_dst, dst_capacity, block_size, opts, dict, d_work, work_size,
                      d_results, stream);
}

}  // extern "C"
