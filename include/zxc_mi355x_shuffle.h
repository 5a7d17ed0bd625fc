/* zxc_mi355x_shuffle.h — the byte-shuffle pre-filter for typed tensors, device to device (zxc_amd/csrc/zxc_shuffle_device.hip, rules
 * in zxc_amd/csrc/zxc_shuffle.h).
 *
 * ZXC is a byte codec: on arrays of 2-, 4- or 8-byte numbers (bf16 / fp32 weights, optimizer moments, int64 ids) it finds little,
 * because the bytes that repeat (signs and exponents, the zero high bytes of small integers) are interleaved with bytes that do
 * not. Regrouping each block's bytes into byte planes, all first bytes, then all second bytes, ..., puts them side by side. The
 * calls below are the device counterpart of the host recipe  data -> byte-shuffle -> zxc_compress,  zxc_decompress -> un-shuffle:
 * the two transposition kernels on their own, and a compress and a decompress call that run them chunk by chunk in front of an
 * append session and behind a take session, so that the extra device memory is one chunk and not one source.
 *
 * THE ARCHIVE DOES NOT RECORD THE FILTER. It is an ordinary v8 archive of the shuffled bytes: any ZXC reader decodes it, to the
 * shuffled bytes. The caller keeps elem_size (and the block size, which is in the file header) and un-shuffles. A block-aligned
 * range fetched with zxc_mi355x_decompress_ranges_device / _rangesv_device is un-shuffled on its own by
 * zxc_mi355x_unshuffle_device with unit = block_size (the range that reaches the end of the archive included: its last unit is
 * the archive's ragged last block). Ranges of the plain bytes at any offset, each into a destination of its own, are
 * zxc_mi355x_decompress_rangesv_shuffle_device's (zxc_mi355x_rangesv_shuffle.h): one call, no second pass.
 *
 * The transform works per unit, a power of two in [4 KiB, 2 MiB]; the archive calls use unit = the block size, so every block holds
 * its own planes. Unit u covers bytes [u unit, min((u + 1) unit, n)); with m its length, E = elem_size, q = m / E and r = m % E:
 *     out[u unit + k q + i] = in[u unit + i E + k]     for k < E, i < q
 * and the last r bytes of the unit are copied unchanged (only the final unit can have r != 0). Un-shuffle is the inverse.
 * elem_size is 2, 4 or 8. */
#ifndef ZXC_MI355X_SHUFFLE_H
#define ZXC_MI355X_SHUFFLE_H
#include "zxc_mi355x.h" /* zxc_dev_dict_t, the options, the error codes */
#ifdef __cplusplus
extern "C" {
#endif

/* d_dst[0, n) = shuffle (un-shuffle) of d_src[0, n), asynchronously on `stream`: one kernel launch, no allocation, no host
 * synchronisation, capturable. Reads exactly d_src[0, n) and writes exactly d_dst[0, n); both pointers may have any alignment;
 * buffers that overlap are the caller's error. Synchronous errors, in this order: NULL d_src or d_dst with n > 0 ->
 * ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 -> ZXC_ERROR_GPU_UNSUPPORTED; unit not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; then n == 0 is ZXC_OK and enqueues nothing; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * The kernels move 16 bytes per lane and access on both sides and transpose in registers; see zxc_shuffle.h for the plan. */
ZXC_EXPORT int zxc_mi355x_shuffle_device(const void* d_src, void* d_dst, uint64_t n, uint32_t elem_size, uint32_t unit, void* stream);
ZXC_EXPORT int zxc_mi355x_unshuffle_device(const void* d_src, void* d_dst, uint64_t n, uint32_t elem_size, uint32_t unit, void* stream);

/* Both archive calls work in chunks of `piece` bytes, a multiple of the block size: with B = the block size (opts->block_size, 512
 * KiB when opts is NULL or says 0; block_size in the decompress call), T = the size of the plain data (src_size / dst_size),
 *     piece = min(floor((max_piece ? max_piece : 64 MiB) / B) x B,  max(1, ceil(T / B)) x B).
 * max_piece == 0 stands for 64 MiB (128 blocks of 512 KiB per encode or decode launch); 0 < max_piece < B is refused as the
 * sessions refuse it (ZXC_ERROR_BAD_BLOCK_SIZE). */

/* Bytes of device scratch zxc_mi355x_compress_shuffle_device needs:
 *     zxc_mi355x_compress_append_dict_device_work_size(src_size, piece, opts, dict_size) + 256 + piece,
 * the session's work area and behind it, on the next multiple of 256, one stage of a chunk. 0 for arguments the call or the session
 * would refuse (options, max_piece, dict_size > 65535, too many blocks). */
ZXC_EXPORT uint64_t zxc_mi355x_compress_shuffle_device_work_size(uint64_t src_size, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                                 uint32_t dict_size);

/* Compress the shuffle of d_src[0, src_size) (elem_size, unit = the block size) into a complete v8 archive at d_dst[0, dst_capacity).
 * The archive and *d_result are byte for byte what zxc_mi355x_compress_device writes for the shuffled source with the same options
 * and capacity; with a dictionary (dict != NULL and dict->size > 0) what zxc_mi355x_compress_dict_device writes for it. (One
 * departure, the session's: where those calls refuse a capacity below the part of the archive known before encoding synchronously,
 * *d_result receives ZXC_ERROR_DST_TOO_SMALL.)
 * It is an append session in d_work (zxc_mi355x_compress_begin_device, or _begin_dict_device when there is a dictionary, with
 * max_total = src_size and max_piece = piece): per chunk of at most piece bytes the shuffle kernel writes from d_src into the stage,
 * zxc_mi355x_compress_append_device takes the stage, and the next chunk reuses it in stream order; then end. Chunks are cut on block
 * boundaries, so each block's planes are its own. Asynchronous on `stream`, no host synchronisation, no device allocation beyond
 * the encoder's stream-ordered scratch at levels 6-7. Reads exactly d_src[0, src_size), of any alignment; d_dst and d_work may have
 * any alignment; nothing is written at or past d_dst + dst_capacity.
 * Synchronous errors, in this order: NULL d_src with src_size > 0, NULL d_result -> ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 ->
 * ZXC_ERROR_GPU_UNSUPPORTED; then those of the session's begin in its order: NULL d_dst / d_work -> ZXC_ERROR_NULL_INPUT;
 * opts->dict -> ZXC_ERROR_GPU_UNSUPPORTED; dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE; NULL d_content or d_id with size > 0 ->
 * ZXC_ERROR_NULL_INPUT; block size, 0 < max_piece < block size, more than 2^31 - 1 blocks -> ZXC_ERROR_BAD_BLOCK_SIZE; work_size
 * too small -> ZXC_ERROR_MEMORY; dst_capacity below the empty archive -> ZXC_ERROR_DST_TOO_SMALL; then, without a device,
 * ZXC_ERROR_GPU_UNAVAILABLE. A launch failure later leaves part of the work enqueued and *d_result unwritten. */
ZXC_EXPORT int zxc_mi355x_compress_shuffle_device(const void* d_src, uint64_t src_size, uint32_t elem_size, void* d_dst,
                                                  uint64_t dst_capacity, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                  const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result,
                                                  void* stream);

/* Bytes of device scratch zxc_mi355x_decompress_shuffle_device needs:
 *     zxc_mi355x_decompress_take_device_work_size(src_size, dst_size, piece, block_size) + 512 + piece,
 * the session's work area and behind it, on the next multiple of 256, the session's result word (256 bytes) and one stage of a
 * chunk. 0 for arguments the call or the session would refuse. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_shuffle_device_work_size(uint64_t src_size, uint64_t dst_size, uint64_t max_piece,
                                                                   uint32_t block_size);

/* Decode the archive d_src[0, src_size) and un-shuffle it (elem_size, unit = block_size) into d_dst[0, dst_size).
 * dst_size must be the decoded size exactly: the last unit's layout depends on it and the host plans with it (the writer knows it;
 * zxc_mi355x_frame_info_device tells it). It is a take session in d_work (zxc_mi355x_decompress_begin_device, or _begin_dict_device
 * when there is a dictionary, with dst_capacity = dst_size and max_piece = piece): per chunk zxc_mi355x_decompress_take_device
 * delivers into the 16-byte aligned stage, where whole blocks decode in place, and the un-shuffle kernel writes the chunk to d_dst,
 * which may have any alignment; the stage is reused in stream order. The session's end writes its verdict into a word of d_work and
 * one last one-thread kernel writes *d_result (device memory), once: the session's word as it is, except that a non-negative
 * size other than dst_size becomes ZXC_ERROR_CORRUPT_DATA (the archive is not the one the caller described); with dst_size == 0 the
 * word is the empty-frame probe's answer, as it is. Negative results are those of zxc_mi355x_decompress_device (with a dictionary:
 * _dict_device) for the same archive, dst_capacity = dst_size, block_size, options and dictionary. After any error the bytes of
 * d_dst are undefined. Nothing is written outside d_dst[0, dst_size) and d_work; d_src is never written and must be READABLE up to
 * src_size + 64, as for zxc_mi355x_decompress_device. Asynchronous on `stream`, no host synchronisation, no device allocation of
 * its own. opts may be NULL; only checksum_enabled and dict are read.
 * Synchronous errors, in this order: NULL d_dst with dst_size > 0, NULL d_result -> ZXC_ERROR_NULL_INPUT; elem_size not 2, 4 or 8 ->
 * ZXC_ERROR_GPU_UNSUPPORTED; then those of the session's begin in its order: NULL d_src / d_work -> ZXC_ERROR_NULL_INPUT;
 * src_size < 28 -> ZXC_ERROR_SRC_TOO_SMALL; block_size, 0 < max_piece < block_size, more than 2^31 - 2 blocks ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict -> ZXC_ERROR_GPU_UNSUPPORTED; dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE; NULL d_content
 * or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT; work_size too small -> ZXC_ERROR_MEMORY; then, without a device,
 * ZXC_ERROR_GPU_UNAVAILABLE. */
ZXC_EXPORT int zxc_mi355x_decompress_shuffle_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_size,
                                                    uint32_t elem_size, uint64_t max_piece, uint32_t block_size,
                                                    const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                                    uint64_t work_size, int64_t* d_result, void* stream);

#ifdef __cplusplus
}
#endif
#endif
