/* zxc_mi355x_rangesv.h — random access into a pointer table, device to device (zxc_amd/csrc/zxc_ranges_device.hip, rules in
 * zxc_amd/csrc/zxc_rangesv.h on top of zxc_ranges.h).
 *
 * zxc_mi355x_decompress_ranges_device (zxc_mi355x.h) fetches any subset of a seekable archive in any order, but into ONE
 * destination buffer: a range names dst_off into a single 16-byte aligned d_dst of one capacity. The calls below are to it what
 * zxc_mi355x_decompress_takev_device is to zxc_mi355x_decompress_take_device: every range carries the absolute device address of
 * its own destination, of any alignment, so that "load this layer", "load these experts", "restore these pages" decode straight
 * into tensors with allocations of their own, without a scratch buffer and a second copy per tensor. Everything else is the
 * sibling's: the index is the one zxc_mi355x_seekable_open_device writes (there is no new open call), the range table lies in
 * device memory and is read on the stream, there is one result word per range, no host synchronisation and no device allocation
 * (the decode launch keeps its per-stream buffers as it does for zxc_mi355x_decode_blocks_device), d_src is never written, block
 * checksum trailers are skipped, and a dictionary variant exists. */
#ifndef ZXC_MI355X_RANGESV_H
#define ZXC_MI355X_RANGESV_H
#include "zxc_mi355x.h" /* zxc_dev_dict_t, the error codes */
#ifdef __cplusplus
extern "C" {
#endif

/* One range to fetch (24 bytes, device-visible layout). */
typedef struct zxc_dev_rangev {
    uint64_t offset; /* first decoded byte wanted */
    uint64_t len;    /* bytes wanted */
    uint64_t base;   /* device address of the destination: [base, base + len), any alignment */
} zxc_dev_rangev_t;

/* Bytes of device scratch the calls below need; 0 for arguments they would refuse. For equal arguments it is the value
 * zxc_mi355x_decompress_ranges_device_work_size returns (J = (max_len - 1) / block_size + 2 jobs per range, a slot per job), so
 * that call's bound holds: at most n_ranges x J x (block_size + 64) + 44 x n_ranges x J + 1536. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_rangesv_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size);

/* For r in [0, n_ranges): decoded bytes [offset_r, offset_r + len_r) of the archive d_src[0, src_size), opened into d_index with
 * the same block_size, go to [base_r, base_r + len_r); d_results[r] (device memory) receives, once, after that range's last byte,
 * what zxc_seekable_decompress_range returns for the same archive, offset, len and a destination of exactly len bytes, in this
 * order: len == 0 -> 0 (whatever else is wrong); a failed index -> its status; an index opened with another block_size ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; len > max_len, or base + len reaching 2^64 -> ZXC_ERROR_DST_TOO_SMALL; base == 0 ->
 * ZXC_ERROR_NULL_INPUT (the table check of zxc_mi355x_compress_appendv_device: a zero base with a length is refused by status and
 * never dereferenced); then the sibling's checks, unchanged and in its order: offset > total or len > total - offset ->
 * ZXC_ERROR_SRC_TOO_SMALL; a dictionary id in the file header -> ZXC_ERROR_DICT_REQUIRED (the _dict call: that without a
 * dictionary, ZXC_ERROR_DICT_MISMATCH when *d_id is not the index's id); a src_size below the archive that was opened ->
 * ZXC_ERROR_SRC_TOO_SMALL; the first failing covered block's status in block order, a covered block that decoded to fewer bytes
 * than the range needs of it being ZXC_ERROR_CORRUPT_DATA; else len.
 * d_ranges lies in device memory and is read on the stream: a kernel enqueued before the call may write it (a routing kernel
 * writes (offset, len, base) for whatever it picked), a replayed graph may fetch other tensors into other places each time.
 * Placement: a block is decoded straight into its destination exactly when all of it is wanted, its address
 * base + (b x block_size - offset) is 16-byte aligned, and the block plus the 32 bytes the decoders may store behind it end inside
 * [base, base + len). Every other covered block is decoded into a slot of d_work and the wanted part is copied out. The range's own
 * destination bounds the spill, not a shared capacity: nothing is promised writable behind a range. With base = offset (mod 16)
 * every block that lies inside a range, its last one or two excepted, is decoded in place.
 * Synchronous errors, in this order: NULL d_src / d_index / d_work / d_results, NULL d_ranges with n_ranges > 0 ->
 * ZXC_ERROR_NULL_INPUT; block_size not a power of two in [4 KiB, 2 MiB] -> ZXC_ERROR_BAD_BLOCK_SIZE; in the _dict call,
 * dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT; n_ranges x J
 * above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_ranges == 0 is ZXC_OK here and enqueues nothing; then, without a
 * device, ZXC_ERROR_GPU_UNAVAILABLE. There is no destination alignment check: there is no d_dst.
 * Guarantees: nothing is written outside [base_r, base_r + len_r) of the valid ranges and d_work. A range that fails leaves its own
 * destination bytes undefined and every other range untouched; a range refused before its blocks are looked at (every status
 * above the covered blocks') leaves its destination untouched too. Ranges may overlap in the archive (a shared block is decoded
 * once per range). Ranges whose destinations overlap are the caller's error: undefined bytes, no fault. d_src must be READABLE up
 * to src_size + 64 (as d_comp of zxc_mi355x_decode_blocks_device). d_work: any alignment, owned by the call until the last result
 * is written. Calls on different streams with different work areas may overlap and may share one index. */
ZXC_EXPORT int zxc_mi355x_decompress_rangesv_device(const void* d_src, uint64_t src_size, const void* d_index,
                                                    const zxc_dev_rangev_t* d_ranges, uint32_t n_ranges, uint64_t max_len,
                                                    uint32_t block_size, void* d_work, uint64_t work_size, int64_t* d_results,
                                                    void* stream);

/* The same with a dictionary in device memory (zxc_dev_dict_t, zxc_mi355x.h), as zxc_mi355x_decompress_ranges_dict_device is to
 * its sibling: same contract, index and work size; the blocks are decoded by the dictionary kernel. A NULL dict, or one with
 * size == 0, makes the call behave exactly as the one above. */
ZXC_EXPORT int zxc_mi355x_decompress_rangesv_dict_device(const void* d_src, uint64_t src_size, const void* d_index,
                                                         const zxc_dev_rangev_t* d_ranges, uint32_t n_ranges, uint64_t max_len,
                                                         uint32_t block_size, const zxc_dev_dict_t* dict, void* d_work,
                                                         uint64_t work_size, int64_t* d_results, void* stream);

#ifdef __cplusplus
}
#endif
#endif
