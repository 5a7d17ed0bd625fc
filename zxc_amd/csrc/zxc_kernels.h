// zxc_kernels.h — every kernel that is launched from another translation unit, declared once. HIP only. Included by
// zxc_hip_shim.hip, which launches them, AND by the files that define them (zxc_decode_kernel.hip with zxc_pivco_dir.inc,
// zxc_encode_kernel.hip, zxc_rangesv_shuffle_device.hip, which launches its own): the names are extern "C", so a definition whose argument list departs from the declaration here is a
// conflicting redeclaration and does not compile, where two hand-kept copies would link and launch with a shifted argument
// block. __launch_bounds__ stay on the definitions; the workgroup sizes the shim launches with are the ones below.
#ifndef ZXC_KERNELS_H
#define ZXC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zxc_appendv.h"    // zav_ctl_t, zap_ctl_t
#include "zxc_container.h"  // zc_ctl_t
#include "zxc_dev.h"
#include "zxc_rangesv_shuffle.h"  // zrs_gather_t, zxc_dev_rangev_t; zsh_plan_t (zxc_shuffle.h)

// threads of the three builds of the section decoder (zxc_pivco_dir.inc): launch bounds, loop strides and the shim's launches
#define PDIR_SMALL_THREADS 128
#define PDIR_MEDIUM_THREADS 256
#define PDIR_LARGE_THREADS 512

// ---------------------------------------------------------------- zxc_decode_kernel.hip
extern "C" __global__ void zxc_decode_blocks_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs,
                                                    uint8_t* out, int32_t* status, uint32_t block_size,
                                                    uint32_t trailer_bytes, uint8_t* scratch, uint32_t scratch_stride, uint32_t dbg,
                                                    uint32_t* slot_busy, uint32_t n_slots, const uint32_t* order,
                                                    uint32_t cap_override, uint32_t* list);
extern "C" __global__ void zxc_decode_blocks_dict_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs,
                                                         uint8_t* out, int32_t* status, uint32_t block_size,
                                                         uint32_t trailer_bytes, uint8_t* scratch, uint32_t scratch_stride,
                                                         uint32_t dbg, uint32_t* slot_busy, uint32_t n_slots,
                                                         const uint32_t* order, uint32_t cap_override, const uint8_t* dict,
                                                         uint32_t dict_size, const uint8_t* dict_huf);
extern "C" __global__ void zxc_decode_blocks_lean_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs,
                                                         uint8_t* out, int32_t* status, uint32_t block_size,
                                                         const uint32_t* order, uint32_t cap_override, uint32_t trailer_bytes,
                                                         const zxc_dev_pre_t* pre, const uint8_t* rscratch);
extern "C" __global__ void zxc_decode_blocks_lean_pre_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint8_t* out, int32_t* status,
                                                             uint32_t block_size, uint32_t cap_override, uint32_t trailer_bytes,
                                                             const zxc_dev_pre_t* pre, const uint8_t* pscratch, const uint32_t* hdr,
                                                             const uint32_t* entries);
extern "C" __global__ void zxc_rle_expand_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, zxc_dev_pre_t* pre, uint8_t* rscratch,
                                                 const uint32_t* hdr, const uint32_t* entries_last);
extern "C" __global__ void zxc_order_hist_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs,
                                                 uint32_t block_size, uint32_t* hist);
extern "C" __global__ void zxc_order_scatter_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs,
                                                    uint32_t block_size, uint32_t* hist, uint32_t* order, uint32_t* list, uint32_t trailer_bytes,
                                                    zxc_dev_pre_t* pre, uint32_t* ctl, uint32_t* pre_entries, zxc_dev_sec_t* secs,
                                                    uint32_t pscratch_cap16, uint32_t cap, uint32_t rscratch_cap16, uint32_t mix_slots = 0u);
// (mix_slots, here and below: the residency zxc_dev_order_mix mixes a long launch for. The shim always passes it; left out, as by
// the emulator harness of the plan tests, the launch stays heaviest first. The two kernels of one launch must get the same value.)
#define ZXC_SECTIONS_KERNEL(name)                                                                                              \
    extern "C" __global__ void name(const uint8_t* comp, const zxc_dev_sec_t* secs, uint32_t* hdr, zxc_dev_pre_t* pre, uint8_t* pscratch)
ZXC_SECTIONS_KERNEL(zxc_pivco_sections_small_kernel);
ZXC_SECTIONS_KERNEL(zxc_pivco_sections_medium_kernel);
ZXC_SECTIONS_KERNEL(zxc_pivco_sections_large_kernel);
#undef ZXC_SECTIONS_KERNEL
extern "C" __global__ void zxc_block_checksum_kernel(const uint8_t* comp, const zxc_dev_job_t* jobs, uint32_t n_jobs, const uint32_t* order, uint8_t* ck_bad,
                                                     uint32_t mix_slots = 0u);
extern "C" __global__ void zxc_checksum_merge_kernel(const uint8_t* ck_bad, int32_t* status, uint32_t n_jobs);

// ---------------------------------------------------------------- zxc_encode_kernel.hip
#define ZXC_ENCODE_DECL(name)                                                                                          \
    extern "C" __global__ void name(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint8_t* slots,        \
                                    uint32_t slot_stride, uint32_t* sizes, uint32_t n_blocks, uint32_t with_checksum,  \
                                    uint32_t depth, uint32_t sufficient, uint32_t lazy, uint32_t dict_size,        \
                                    uint8_t* huf_scratch, uint32_t huf)
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l1);
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l2);
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l3);
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l4);
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l57);
ZXC_ENCODE_DECL(zxc_encode_blocks_kernel_l67);
#undef ZXC_ENCODE_DECL
// ... and the job-table entries beside them: one zxc_enc_job_t per workgroup instead of a contiguous source
#define ZXC_ENCODE_JOBS_DECL(name)                                                                                     \
    extern "C" __global__ void name(const uint8_t* src, const zxc_enc_job_t* jobs, uint32_t block_size, uint8_t* slots, \
                                    uint32_t slot_stride, uint32_t* sizes, uint32_t n_jobs, uint32_t with_checksum,    \
                                    uint32_t depth, uint32_t sufficient, uint32_t lazy, uint32_t dict_size,            \
                                    uint8_t* huf_scratch, uint32_t huf)
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l1);
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l2);
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l3);
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l4);
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l57);
ZXC_ENCODE_JOBS_DECL(zxc_encode_jobs_kernel_l67);
#undef ZXC_ENCODE_JOBS_DECL
extern "C" __global__ void zxc_prepend_dict_kernel(const uint8_t* src, uint64_t src_size, uint32_t block_size, const uint8_t* dict,
                                                   uint32_t dict_size, uint8_t* work, uint32_t n_blocks);
extern "C" __global__ void zxc_encode_job_images_kernel(const uint8_t* src, zxc_enc_job_t* jobs, uint32_t n, uint32_t block_size,
                                                        const uint8_t* dict, uint32_t dict_size, uint8_t* work);
extern "C" __global__ void zxc_block_offsets_kernel(uint32_t* sizes, uint64_t* offsets, uint32_t n_blocks, uint32_t max_size);
extern "C" __global__ void zxc_gather_blocks_kernel(const uint8_t* slots, uint32_t slot_stride, const uint32_t* sizes,
                                                    const uint64_t* offsets, uint8_t* out, uint32_t n_blocks);

// ---------------------------------------------------------------- zxc_unframe_device.hip
// The container stages of zxc_mi355x_decompress_device and of the take session: zd_container_stages, zd_verdict_stages (zxc_device_util.h).
extern "C" __global__ void zxc_unframe_head_kernel(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size,
                                                   uint32_t want_verify, uint32_t n_jobs, zc_ctl_t* ctl, const uint32_t* dict_id);
extern "C" __global__ void zxc_unframe_tiles_kernel(const uint8_t* src, const zc_ctl_t* ctl, uint64_t* tile_sum, uint32_t* tile_bad);
extern "C" __global__ void zxc_unframe_scan_kernel(uint64_t* tile_sum, const uint32_t* tile_bad, uint32_t n_tiles, zc_ctl_t* ctl);
extern "C" __global__ void zxc_unframe_scatter_kernel(const uint8_t* src, const zc_ctl_t* ctl, const uint64_t* tile_off, uint32_t block_size,
                                                      uint32_t k_direct, uint32_t n_jobs, zxc_dev_job_t* jobs, uint32_t* tile_hash,
                                                      uint32_t* tile_bad);
extern "C" __global__ void zxc_unframe_walk_kernel(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t k_direct,
                                                   uint32_t n_jobs, const uint32_t* tile_hash, const uint32_t* tile_bad, zxc_dev_job_t* jobs,
                                                   zc_ctl_t* ctl);
extern "C" __global__ void zxc_unframe_events_kernel(const int32_t* status, uint32_t block_size, uint32_t n_jobs, uint64_t dst_capacity,
                                                     zc_ctl_t* ctl);
extern "C" __global__ void zxc_unframe_result_kernel(const zc_ctl_t* ctl, const int32_t* status, uint32_t block_size, uint32_t n_jobs,
                                                     int64_t* result);

// ---------------------------------------------------------------- zxc_append_device.hip
// The scan of a table of (base, len) entries (zxc_appendv.h): zxc_mi355x_compress_appendv_device's, which the take session's takev
// (zxc_take_device.hip) launches as it is, with a zap_ctl_t of its own that nobody reads.
extern "C" __global__ void zxc_appendv_reduce_kernel(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint64_t* tile_sum,
                                                     uint32_t* tile_flags);
extern "C" __global__ void zxc_appendv_scan_kernel(uint64_t* tile_sum, const uint32_t* tile_flags, uint32_t n_tiles, uint64_t total,
                                                   uint64_t* starts, uint32_t n_iov, zav_ctl_t* vctl, zap_ctl_t* ctl);
extern "C" __global__ void zxc_appendv_starts_kernel(const zxc_dev_iov_t* iov, uint32_t n_iov, const uint64_t* tile_off, uint64_t* starts);

// ---------------------------------------------------------------- zxc_rangesv_shuffle_device.hip
// zxc_mi355x_decompress_rangesv_shuffle_device: plan, the gather out of a slot's planes per element size, verdict.
extern "C" __global__ void zxc_rangesv_shuffle_plan_kernel(const void* index, const zxc_dev_rangev_t* ranges, uint32_t J, uint32_t n_jobs,
                                                           uint64_t src_size, uint64_t max_len, uint32_t block_size, uint64_t out_base,
                                                           uint64_t stage_rel, zxc_dev_job_t* jobs, zrs_gather_t* gathers, const uint32_t* dict_id);
#define ZXC_RANGESV_SHUFFLE_GATHER_DECL(name)                                                                                      \
    extern "C" __global__ void name(const uint8_t* stage, uint32_t slot_stride, const zrs_gather_t* gathers, const int32_t* status, \
                                    uint32_t n_jobs, uint32_t chunks, uint8_t* out)
ZXC_RANGESV_SHUFFLE_GATHER_DECL(zxc_rangesv_shuffle_gather2_kernel);
ZXC_RANGESV_SHUFFLE_GATHER_DECL(zxc_rangesv_shuffle_gather4_kernel);
ZXC_RANGESV_SHUFFLE_GATHER_DECL(zxc_rangesv_shuffle_gather8_kernel);
#undef ZXC_RANGESV_SHUFFLE_GATHER_DECL
extern "C" __global__ void zxc_rangesv_shuffle_verdict_kernel(const void* index, const zxc_dev_rangev_t* ranges, uint32_t n_ranges, uint32_t J,
                                                              const int32_t* status, uint64_t src_size, uint64_t max_len, uint32_t block_size,
                                                              int64_t* results, const uint32_t* dict_id);

// ---------------------------------------------------------------- zxc_shufflev_device.hip
// zxc_mi355x_shufflev_device / _compress_shufflev_device: the gather-shuffle of a chunk of a table's concatenation per element
// size, and the kernel that writes the call's status or result word.
#define ZXC_SHUFFLEV_DECL(name)                                                                                                     \
    extern "C" __global__ void name(const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, const zav_ctl_t* vctl, uint64_t v, \
                                    uint8_t* dst, zsh_plan_t pl, uint64_t n)
ZXC_SHUFFLEV_DECL(zxc_shufflev2_kernel);
ZXC_SHUFFLEV_DECL(zxc_shufflev4_kernel);
ZXC_SHUFFLEV_DECL(zxc_shufflev8_kernel);
#undef ZXC_SHUFFLEV_DECL
extern "C" __global__ void zxc_shufflev_result_kernel(const zav_ctl_t* vctl, const int64_t* word, int64_t* d_result);

// ---------------------------------------------------------------- zxc_unshufflev_device.hip
// zxc_mi355x_unshufflev_device / _decompress_shufflev_device: the un-shuffle of a contiguous chunk scattered into a chunk of a
// table's concatenation per element size, and the kernel that writes the call's status or result word.
#define ZXC_UNSHUFFLEV_DECL(name)                                                                                                  \
    extern "C" __global__ void name(const uint8_t* src, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov,          \
                                    const zav_ctl_t* vctl, uint64_t v, zsh_plan_t pl, uint64_t n)
ZXC_UNSHUFFLEV_DECL(zxc_unshufflev2_kernel);
ZXC_UNSHUFFLEV_DECL(zxc_unshufflev4_kernel);
ZXC_UNSHUFFLEV_DECL(zxc_unshufflev8_kernel);
#undef ZXC_UNSHUFFLEV_DECL
extern "C" __global__ void zxc_unshufflev_result_kernel(const zav_ctl_t* vctl, const int64_t* word, uint64_t total, int64_t* d_result);
#ifdef EXP_ENC_CLOCKS  // (experiment build only, tools/encclk.py)
extern "C" __global__ void zxc_enc_clk_read_kernel(unsigned long long* out);
#endif
#endif
