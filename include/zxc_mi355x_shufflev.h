/* zxc_mi355x_shufflev.h — the byte-shuffle pre-filter over a table of typed tensors, device to device
 * (zxc_amd/csrc/zxc_shufflev_device.hip, rules in zxc_amd/csrc/zxc_shufflev.h): the write side that matches
 * zxc_mi355x_decompress_rangesv_shuffle_device (zxc_mi355x_rangesv_shuffle.h).
 *
 * A checkpoint is a table of tensors. zxc_mi355x_compress_shuffle_device (zxc_mi355x_shuffle.h) takes one contiguous source, and
 * zxc_mi355x_compress_appendv_device takes a table but does not shuffle: to write the archive the shuffled ranges call reads, a
 * caller had to concatenate the state dict first, a second copy of the source in device memory and one more pass over it. The
 * calls below take the table itself, n_iov entries of zxc_dev_iov_t {base, len} IN DEVICE MEMORY, as appendv does. X is the
 * concatenation of the entries in table order, `total` bytes; an entry with len == 0 is allowed anywhere and its base is never
 * looked at. The host never holds a pointer, a length or a concatenated copy: it knows n_iov and total.
 *   save   a table of {base, len}           -> one seekable archive of byte planes          (zxc_mi355x_compress_shufflev_device)
 *   load   a table of {offset, len, base}   -> any subset of the tensors, each in its own allocation   (rangesv_shuffle)
 * Tensor r is read back with zxc_mi355x_decompress_rangesv_shuffle_device at offset = starts[r] = the lengths of the entries in
 * front of it added up, len = its length; for whole tensors that wants every len to be a multiple of elem_size (a range of the
 * plain bytes may start anywhere, but elements that straddle two tensors belong to neither).
 *
 * There is ONE elem_size per call, and the archive does not record the filter (zxc_mi355x_shuffle.h): a checkpoint of mixed dtypes
 * is one archive per dtype.
 *
 * The transform, its units and elem_size (2, 4 or 8) are zxc_mi355x_shuffle.h's. The table is checked on the device, as appendv
 * checks it: an entry with len > 0 and base == NULL -> ZXC_ERROR_NULL_INPUT; an entry longer than total, or lengths that add up
 * (saturating) to more than total -> ZXC_ERROR_OVERFLOW; to less -> ZXC_ERROR_SRC_TOO_SMALL; in that precedence. */
#ifndef ZXC_MI355X_SHUFFLEV_H
#define ZXC_MI355X_SHUFFLEV_H
#include "zxc_mi355x_shuffle.h" /* the transform, zxc_dev_iov_t, zxc_dev_dict_t, the options, the error codes */
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch zxc_mi355x_shufflev_device needs for a table of n_iov entries: the scan's control word, starts[0 ..
 * n_iov] and per tile of 1024 entries a sum and the flags of the check (the scratch of zxc_mi355x_compress_appendv_dict_device
 * with a dictionary: no images), and 256 bytes for a word the scan writes and nobody reads. With t = ceil(n_iov / 1024) and up256
 * rounding up to a multiple of 256:
 *     768 + up256(8 x (n_iov + 1)) + up256(8 x t) + up256(4 x t)      <=  8 x (n_iov + 1) + 16 x t + 4096 + 256.
 * Never 0. */
ZXC_EXPORT uint64_t zxc_mi355x_shufflev_device_scratch_size(uint32_t n_iov);

/* d_dst[0, total) = shuffle of X (elem_size, unit) exactly as zxc_mi355x_shuffle_device writes it for the concatenation, with no
 * concatenated copy: the scan of the table (three launches: starts[], the table's status), then one kernel that gathers and
 * transposes. A lane owns groups of 16 elements as in the sibling's kernel; a 16-byte run of the element side that lies inside one
 * entry is one 16-byte load at whatever alignment base + off has, a run that crosses an entry boundary is assembled in registers a
 * byte at a time from consecutive entries. Reads exactly the bytes of the entries (nothing is promised readable behind one) and
 * writes exactly d_dst[0, total), of any alignment; d_scratch may have any alignment. A destination that overlaps an entry is the
 * caller's error. *d_status (device memory) is written once, by the call's last kernel: 0, or the table's error (above); after a
 * table error no kernel reads an entry and d_dst is not written. Asynchronous on `stream`, no host synchronisation, no device
 * allocation, capturable; the table may be uploaded on the stream right before the call.
 * Synchronous errors, in this order: NULL d_iov with n_iov > 0, NULL d_dst with total > 0, NULL d_scratch, NULL d_status ->
 * ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 -> ZXC_ERROR_GPU_UNSUPPORTED; unit not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; n_iov == 0 with total > 0 -> ZXC_ERROR_SRC_TOO_SMALL; scratch_size below
 * zxc_mi355x_shufflev_device_scratch_size(n_iov) -> ZXC_ERROR_MEMORY. What is left is valid (total == 0 with n_iov == 0 is ZXC_OK
 * and enqueues only the store of *d_status = 0) and needs a device: without one, ZXC_ERROR_GPU_UNAVAILABLE. */
ZXC_EXPORT int zxc_mi355x_shufflev_device(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_dst, uint32_t elem_size,
                                          uint32_t unit, void* d_scratch, uint64_t scratch_size, int64_t* d_status, void* stream);

/* Bytes of device scratch zxc_mi355x_compress_shufflev_device needs:
 *     up256(zxc_mi355x_compress_shuffle_device_work_size(total, max_piece, opts, dict_size))
 *         + zxc_mi355x_shufflev_device_scratch_size(n_iov) + 256,
 * that is [session | stage | table scratch | 256 bytes: the session's result word]. 0 whenever the sibling's size is 0 (options,
 * max_piece, dict_size > 65535, too many blocks). */
ZXC_EXPORT uint64_t zxc_mi355x_compress_shufflev_device_work_size(uint32_t n_iov, uint64_t total, uint64_t max_piece,
                                                                  const zxc_compress_opts_t* opts, uint32_t dict_size);

/* zxc_mi355x_compress_shuffle_device with X in place of d_src: the shuffle of X (elem_size, unit = the block size) compressed into
 * a complete v8 archive at d_dst[0, dst_capacity). The piece size, the stage, the append session in d_work (_begin_dict_device when
 * there is a dictionary) and the host loop are the sibling's; the table is scanned once, in front of the first chunk, and per chunk
 * the gather kernel of zxc_mi355x_shufflev_device writes the shuffle of X[at, at + n) into the stage where the sibling's kernel
 * reads d_src + at. So the extra device memory is one chunk and the table's scratch, not one source. The session's end writes into
 * a word of d_work, and one last one-thread kernel writes *d_result (device memory), once: the table's error if it has one (the
 * bytes of d_dst[0, dst_capacity) are then undefined, and no kernel has read an entry), else the session's word. With a valid table
 * the archive and *d_result are byte for byte what zxc_mi355x_compress_shuffle_device writes for the concatenation with the same
 * elem_size, options, dictionary, max_piece and capacity. Nothing is written outside d_dst[0, dst_capacity) and d_work[0,
 * work_size); both may have any alignment. Asynchronous on `stream`, no host synchronisation, no device allocation beyond the
 * encoder's stream-ordered scratch at levels 6-7.
 * Synchronous errors, in this order: NULL d_iov with n_iov > 0, NULL d_result -> ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 ->
 * ZXC_ERROR_GPU_UNSUPPORTED; n_iov == 0 with total > 0 -> ZXC_ERROR_SRC_TOO_SMALL; then those of the sibling's begin in its order
 * (NULL d_dst / d_work, opts->dict, the dictionary, block size and max_piece, work_size too small -> ZXC_ERROR_MEMORY,
 * dst_capacity below the empty archive: see zxc_mi355x_shuffle.h); then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. A launch
 * failure later leaves part of the work enqueued and *d_result unwritten. */
ZXC_EXPORT int zxc_mi355x_compress_shufflev_device(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, uint32_t elem_size,
                                                   void* d_dst, uint64_t dst_capacity, uint64_t max_piece,
                                                   const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                                   uint64_t work_size, int64_t* d_result, void* stream);

#ifdef __cplusplus
}
#endif
#endif
