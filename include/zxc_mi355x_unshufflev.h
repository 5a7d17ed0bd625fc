/* zxc_mi355x_unshufflev.h — the inverse byte-shuffle into a table of typed tensors, device to device
 * (zxc_amd/csrc/zxc_unshufflev_device.hip, rules in zxc_amd/csrc/zxc_unshufflev.h): the load side that mirrors
 * zxc_mi355x_compress_shufflev_device (zxc_mi355x_shufflev.h).
 *
 * A checkpoint is restored into the tensors' own allocations. zxc_mi355x_decompress_shuffle_device (zxc_mi355x_shuffle.h) writes
 * one contiguous destination, a second copy of the checkpoint and one device copy per tensor behind it;
 * zxc_mi355x_decompress_rangesv_shuffle_device decodes every covered block into a slot of its own, wants a seekable archive with
 * an opened index and offsets the host added up. The calls below take the table itself, n_iov entries of zxc_dev_iov_t {base, len}
 * IN DEVICE MEMORY, as zxc_mi355x_decompress_takev_device does. Y is the concatenation of the entries' destinations in table order,
 * `total` bytes; an entry with len == 0 is allowed anywhere and its base is never looked at. The host never holds a pointer or a
 * length: it knows n_iov and total. The archive is decoded chunk by chunk into one stage, so the extra device memory is one chunk
 * and about 8 bytes per entry whatever the checkpoint's size, and the archive need not be seekable.
 *   save   a table of {base, len}   -> one archive of byte planes              (zxc_mi355x_compress_shufflev_device)
 *   load   one archive              -> the same table of {base, len}, whole    (zxc_mi355x_decompress_shufflev_device)
 *
 * There is ONE elem_size per call, and the archive does not record the filter (zxc_mi355x_shuffle.h).
 *
 * The transform, its units and elem_size (2, 4 or 8) are zxc_mi355x_shuffle.h's. The table is checked on the device, as takev
 * checks it: an entry with len > 0 and base == NULL -> ZXC_ERROR_NULL_INPUT; an entry longer than total, or lengths that add up
 * (saturating) to more than total -> ZXC_ERROR_OVERFLOW; to less -> ZXC_ERROR_DST_TOO_SMALL; in that precedence. */
#ifndef ZXC_MI355X_UNSHUFFLEV_H
#define ZXC_MI355X_UNSHUFFLEV_H
#include "zxc_mi355x_shufflev.h" /* the transform, zxc_dev_iov_t, zxc_dev_dict_t, the options, the error codes, the scratch's form */
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch zxc_mi355x_unshufflev_device needs for a table of n_iov entries: exactly
 * zxc_mi355x_shufflev_device_scratch_size(n_iov) (the same scan, the same shape, the same 256 bytes nobody reads). Never 0. */
ZXC_EXPORT uint64_t zxc_mi355x_unshufflev_device_scratch_size(uint32_t n_iov);

/* Y = the un-shuffle (elem_size, unit) of d_src[0, total), byte for byte what zxc_mi355x_unshuffle_device writes for a contiguous
 * destination, with no contiguous copy: the scan of the table (three launches: starts[], the table's status), one kernel that
 * transposes and scatters, one one-thread kernel that stores *d_status. A lane owns groups of 16 elements as in the sibling's
 * kernel; a 16-byte run of the element side that lies inside one entry is one 16-byte store at whatever alignment base + off has,
 * a run that crosses an entry boundary is stored a byte at a time into consecutive entries. Reads exactly d_src[0, total), of any
 * alignment, and writes exactly the bytes of the entries (nothing is promised writable behind one); d_scratch may have any
 * alignment. Entries that overlap each other or d_src are the caller's error: undefined bytes, no fault. *d_status (device
 * memory) is written once, by the call's last kernel: 0, or the table's error (above); after a table error no byte of any entry
 * is written. Asynchronous on `stream`, no host synchronisation, no device allocation, capturable; the table may be uploaded on
 * the stream right before the call.
 * Synchronous errors, in this order: NULL d_iov with n_iov > 0, NULL d_src with total > 0, NULL d_scratch, NULL d_status ->
 * ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 -> ZXC_ERROR_GPU_UNSUPPORTED; unit not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; n_iov == 0 with total > 0 -> ZXC_ERROR_DST_TOO_SMALL; scratch_size below
 * zxc_mi355x_unshufflev_device_scratch_size(n_iov) -> ZXC_ERROR_MEMORY. What is left is valid (total == 0 with n_iov == 0 is ZXC_OK
 * and enqueues only the store of *d_status = 0) and needs a device: without one, ZXC_ERROR_GPU_UNAVAILABLE. */
ZXC_EXPORT int zxc_mi355x_unshufflev_device(const void* d_src, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total,
                                            uint32_t elem_size, uint32_t unit, void* d_scratch, uint64_t scratch_size,
                                            int64_t* d_status, void* stream);

/* Bytes of device scratch zxc_mi355x_decompress_shufflev_device needs:
 *     up256(zxc_mi355x_decompress_shuffle_device_work_size(src_size, total, max_piece, block_size))
 *         + zxc_mi355x_unshufflev_device_scratch_size(n_iov),
 * that is [session | the session's result word | stage | table scratch]: one chunk, the take session and about 8 bytes per
 * entry. 0 whenever the sibling's size is 0 (block size, max_piece, too many blocks). */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_shufflev_device_work_size(uint32_t n_iov, uint64_t src_size, uint64_t total,
                                                                    uint64_t max_piece, uint32_t block_size);

/* zxc_mi355x_decompress_shuffle_device with Y in place of d_dst and total in place of dst_size: the archive d_src[0, src_size) is
 * decoded and un-shuffled (elem_size, unit = block_size) into the entries. total must be the decoded size exactly. The piece, the
 * take session in d_work (_begin_dict_device), the take into the 16-byte aligned stage per chunk and the session's end into a word
 * of d_work are the sibling's; the table is scanned once, in front of the first chunk, and per chunk the scatter kernel of
 * zxc_mi355x_unshufflev_device writes the un-shuffle of the stage into Y[at, at + n) where the sibling's kernel writes d_dst + at.
 * One last one-thread kernel writes *d_result (device memory), once: the table's error if it has one (no byte of any entry has
 * been written), else exactly the sibling's word: a non-negative size other than total becomes ZXC_ERROR_CORRUPT_DATA, and with
 * total == 0 it is the empty-frame probe's answer. With a valid table the entries' bytes and *d_result are what
 * zxc_mi355x_decompress_shuffle_device produces for the same archive, options, dictionary, max_piece and dst_size = total, cut by
 * the table. After a decode error the entries' bytes are undefined, but nothing outside the entries and d_work[0, work_size) is
 * ever written. d_src is never written and must be READABLE up to src_size + 64, as for the sibling; it need not be seekable.
 * Asynchronous on `stream`, no host synchronisation, no device allocation of its own. opts may be NULL; only checksum_enabled and
 * dict are read.
 * Synchronous errors, in this order: NULL d_iov with n_iov > 0, NULL d_result -> ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 ->
 * ZXC_ERROR_GPU_UNSUPPORTED; n_iov == 0 with total > 0 -> ZXC_ERROR_DST_TOO_SMALL; then those of the sibling's begin in its order
 * (NULL d_src / d_work, src_size < 28, block size and max_piece, opts->dict, the dictionary, work_size too small ->
 * ZXC_ERROR_MEMORY: see zxc_mi355x_shuffle.h); then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. No launch is made before begin
 * has accepted the arguments. A launch failure later leaves part of the work enqueued and *d_result unwritten. */
ZXC_EXPORT int zxc_mi355x_decompress_shufflev_device(const void* d_src, uint64_t src_size, const zxc_dev_iov_t* d_iov, uint32_t n_iov,
                                                     uint64_t total, uint32_t elem_size, uint64_t max_piece, uint32_t block_size,
                                                     const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                                     uint64_t work_size, int64_t* d_result, void* stream);

#ifdef __cplusplus
}
#endif
#endif
