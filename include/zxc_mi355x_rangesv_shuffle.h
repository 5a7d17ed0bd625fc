/* zxc_mi355x_rangesv_shuffle.h — random access into a pointer table for archives of byte-shuffled typed tensors, device to device
 * (zxc_amd/csrc/zxc_rangesv_shuffle_device.hip, rules in zxc_amd/csrc/zxc_rangesv_shuffle.h on top of zxc_rangesv.h and
 * zxc_shuffle.h).
 *
 * zxc_mi355x_compress_shuffle_device (zxc_mi355x_shuffle.h) writes a seekable archive whose blocks hold the byte planes of the
 * tensor's elements; zxc_mi355x_decompress_rangesv_device (zxc_mi355x_rangesv.h) fetches any subset of a seekable archive straight
 * into tensors with allocations of their own, but delivers the archive's bytes as they are: the shuffled ones. The call below
 * composes the two. Its ranges count bytes of the PLAIN tensor, at any offset and of any length, and each destination receives
 * plain bytes: every covered block is decoded into a slot of d_work, and the copy-out gathers across the elem_size planes of the
 * slot. The transform keeps sizes and each of its units is one block, so a plain range lies in the same blocks as the shuffled
 * one: index, jobs per range, slots and result words are the sibling's. */
#ifndef ZXC_MI355X_RANGESV_SHUFFLE_H
#define ZXC_MI355X_RANGESV_SHUFFLE_H
#include "zxc_mi355x_rangesv.h" /* zxc_dev_rangev_t */
#include "zxc_mi355x_shuffle.h" /* the transform */
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch the call below needs; 0 for arguments it would refuse. With J = (max_len - 1) / block_size + 2 jobs per
 * range (1 when max_len == 0), N = n_ranges x J and up(x) = x rounded up to a multiple of 256:
 *     up(up(up(24 N) + 4 N) + 24 N) + N x (block_size + 64) + 256,
 * rangesv's layout (a zxc_dev_job_t, a status word and a slot of block_size + 64 bytes per job) with a gather record of 24 bytes
 * per job where that call keeps a copy record of 16; at most N x (block_size + 64) + 52 N + 1024. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_rangesv_shuffle_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size);

/* For r in [0, n_ranges): [base_r, base_r + len_r) receives bytes [offset_r, offset_r + len_r) of the un-shuffle (elem_size,
 * unit = block_size, zxc_mi355x_shuffle.h) of what the archive d_src[0, src_size) decodes to. Offsets and lengths count plain bytes
 * and need not be multiples of elem_size. The archive does not record the filter: the caller keeps elem_size.
 * Everything else is zxc_mi355x_decompress_rangesv_device's: d_index is the one zxc_mi355x_seekable_open_device wrote with the same
 * block_size; d_ranges (zxc_dev_rangev_t) lies in device memory and is read on the stream, so a kernel enqueued before the call may
 * write it; one result word per range in d_results (device memory), written once; asynchronous on `stream`, no host
 * synchronisation, no device allocation; block checksum trailers are skipped. dict may be NULL or have size == 0: no dictionary;
 * else the blocks are decoded by the dictionary kernel, as in zxc_mi355x_decompress_rangesv_dict_device.
 * d_results[r], in that call's order: len == 0 -> 0 (whatever else is wrong); a failed index -> its status; an index opened with
 * another block_size -> ZXC_ERROR_BAD_BLOCK_SIZE; len > max_len, or base + len reaching 2^64 -> ZXC_ERROR_DST_TOO_SMALL; base == 0
 * -> ZXC_ERROR_NULL_INPUT; offset > total or len > total - offset -> ZXC_ERROR_SRC_TOO_SMALL; a dictionary id in the file header
 * and no dictionary -> ZXC_ERROR_DICT_REQUIRED, another dictionary -> ZXC_ERROR_DICT_MISMATCH; a src_size below the archive that was
 * opened -> ZXC_ERROR_SRC_TOO_SMALL; the first failing covered block's status in block order; else len.
 * One departure: the planes of a block are laid out by its length, so a covered block whose decoded length is not the length the
 * index gives it, min(block_size, total - b x block_size) for block b, counts as ZXC_ERROR_CORRUPT_DATA in that block's turn, and
 * nothing is moved for it. (This contains the sibling's "decoded to fewer bytes than the range needs of it".)
 * Placement: no block is decoded in place. A lane of the gather kernel moves a whole group of 16 elements that lies inside the
 * range with elem_size 16-byte loads from the planes, a transposition in registers and elem_size 16-byte stores at whatever
 * alignment base gives; the bytes of a range's two edge groups and the leftovers of a ragged last block move a byte at a time.
 * Synchronous errors, in this order: NULL d_src / d_index / d_work / d_results, NULL d_ranges with n_ranges > 0 ->
 * ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 -> ZXC_ERROR_GPU_UNSUPPORTED; block_size not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0 ->
 * ZXC_ERROR_NULL_INPUT; n_ranges x J above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_ranges == 0 is ZXC_OK here and
 * enqueues nothing; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * Guarantees: nothing is written outside [base_r, base_r + len_r) of the valid ranges and d_work. A range that fails leaves its own
 * destination bytes undefined and every other range untouched; a range refused before its blocks are looked at leaves its
 * destination untouched too. Ranges may overlap in the archive (a shared block is decoded once per range); ranges whose
 * destinations overlap are the caller's error: undefined bytes, no fault. d_src is never written and must be READABLE up to
 * src_size + 64. d_work: any alignment, owned by the call until the last result is written. Calls on different streams with
 * different work areas may overlap and may share one index. */
ZXC_EXPORT int zxc_mi355x_decompress_rangesv_shuffle_device(const void* d_src, uint64_t src_size, const void* d_index,
                                                            const zxc_dev_rangev_t* d_ranges, uint32_t n_ranges, uint64_t max_len,
                                                            uint32_t elem_size, uint32_t block_size, const zxc_dev_dict_t* dict,
                                                            void* d_work, uint64_t work_size, int64_t* d_results, void* stream);

#ifdef __cplusplus
}
#endif
#endif
