/* zxc_mi355x.h — device-resident C-ABI of libzxc_mi355x.so (plain pointers and
 * sizes; no C++/torch types). This is the boundary the reference's own block loops
 * would bind to run on an MI355X:
 *
 *   zxc_mi355x_decode_blocks_device  replaces the per-block calls to the internal
 *       zxc_decompress_chunk_wrapper (src/lib/zxc_dispatch.c:279-283, :479-493) made
 *       by zxc_decompress_frame (:912-1001), the seekable ST loop
 *       (src/lib/zxc_seekable.c:742-781) and the seekable MT worker (:943-976):
 *       instead of one 64 KiB block per call on a CPU thread, one launch decodes a
 *       whole table of independent blocks, one wavefront per block.
 *   zxc_mi355x_plan_seekable  produces that table from a seekable handle
 *       (the job planning of src/lib/zxc_seekable.c:1033-1056).
 *
 * All d_* arguments are device pointers on the current HIP device. Return values
 * follow the zxc convention: >= 0 success, < 0 zxc_error_t (zxc_error.h). */
#ifndef ZXC_MI355X_H
#define ZXC_MI355X_H
#include <stddef.h>
#include <stdint.h>
#include "zxc_export.h"
#include "zxc_opts.h"
#include "zxc_seekable.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One block to decode (24 bytes, device- and host-visible layout). */
typedef struct zxc_dev_job {
    uint64_t comp_off;  /* byte offset of the block's 8-byte header inside d_comp */
    uint64_t out_off;   /* byte offset inside d_out; MUST be a multiple of 16 */
    uint32_t comp_size; /* physical block size: header + payload (+ 4-byte checksum trailer) */
    uint32_t out_len;   /* decoded bytes to keep: block_size, or the archive's tail remainder */
} zxc_dev_job_t;

/* Number of usable HIP devices (0 when there is none / no driver). */
ZXC_EXPORT int zxc_mi355x_device_count(void);
/* Select the device used by the calling thread (hipSetDevice). */
ZXC_EXPORT int zxc_mi355x_set_device(int device);
/* The device the calling thread uses (hipGetDevice), or a negative zxc_error_t. */
ZXC_EXPORT int zxc_mi355x_get_device(void);

/* Device memory helpers so a C caller needs no HIP headers. */
ZXC_EXPORT void* zxc_mi355x_malloc(size_t bytes);
ZXC_EXPORT void zxc_mi355x_free(void* d_ptr);
ZXC_EXPORT int zxc_mi355x_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
ZXC_EXPORT int zxc_mi355x_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
ZXC_EXPORT int zxc_mi355x_synchronize(void* stream);
/* Gives back the device memory the library keeps between calls (staging arenas of the host API that nobody is using;
 * on the calling thread's device also the section decoders' scratch pools and the launch-order buffers). Call it when
 * no launch of this library is in flight on that device. Arenas are bounded anyway: every host entry point works in
 * batches of 256 MiB of output, and a buffer that grew past 768 MiB is freed when its call ends. */
ZXC_EXPORT void zxc_mi355x_release_cached(void);

/* Fill jobs[0..n_blocks) for blocks [first_block, first_block + n_blocks) of an open
 * seekable archive. Block i's compressed bytes are expected at
 * d_comp + (archive_offset(i) - comp_rebase) and its output at
 * d_out + (i - first_block) * block_size (16-byte aligned by construction).
 * Pass comp_rebase = 0 when the whole archive was uploaded. Returns n_blocks. */
ZXC_EXPORT int64_t zxc_mi355x_plan_seekable(const zxc_seekable* s, uint32_t first_block,
                                            uint32_t n_blocks, uint64_t comp_rebase,
                                            zxc_dev_job_t* jobs);

/* Decode n_jobs independent blocks, asynchronously on `stream` (a hipStream_t, or
 * NULL for the default stream). d_status[i] receives block i's decoded size or a
 * negative zxc_error_t. Requirements: d_out + job.out_off 16-byte aligned; d_out
 * readable/writable up to round_up(out_off + out_len, 16) + 16. block_size is the
 * archive's block size (bounds scratch and the per-block output cap
 * block_size + 2112, like the reference). verify_trailer = 1 means every block
 * carries its 4-byte checksum trailer and it is verified on device (rapidhash of the
 * payload, ZXC_ERROR_BAD_CHECKSUM on mismatch). */
ZXC_EXPORT int zxc_mi355x_decode_blocks_device(const void* d_comp, const zxc_dev_job_t* d_jobs,
                                               uint32_t n_jobs, void* d_out, int32_t* d_status,
                                               uint32_t block_size, int verify_trailer, void* stream);

/* Same, for archives compressed with a dictionary: d_dict[0..dict_size) is logically prepended to
 * every block (reference d_floor = dst - dict_size, src/lib/zxc_decompress.c:1028); d_dict_huf is
 * the dictionary's 128-byte shared literal table (enc_lit = 3 sections) or NULL. */
ZXC_EXPORT int zxc_mi355x_decode_blocks_dict_device(const void* d_comp, const zxc_dev_job_t* d_jobs,
                                                    uint32_t n_jobs, void* d_out, int32_t* d_status,
                                                    uint32_t block_size, int verify_trailer,
                                                    const void* d_dict, uint32_t dict_size,
                                                    const void* d_dict_huf, void* stream);

/* ---- encode side (LZ77 match finder + GLO serialiser, zxc_amd/csrc/zxc_encode_kernel.hip) ----
 * Replaces the per-block calls to zxc_compress_chunk_wrapper (src/lib/zxc_compress.c:2041-2074)
 * made by zxc_compress (src/lib/zxc_dispatch.c:734-780). Block i of the source
 * (d_src + i*block_size) becomes one complete v8 block (8-byte header + payload, GLO or RAW) at
 * d_slots + i*zxc_mi355x_encode_slot_stride(block_size); its size lands in d_sizes[i]
 * (= the seek-table entry; with_checksum appends the 4-byte rapidhash trailer). Asynchronous on `stream`.
 * d_src must be READABLE up to src_size + 32 (the match finder compares 16 bytes at a time and clamps lengths to the
 * block afterwards; the bytes themselves are never used). */
ZXC_EXPORT uint32_t zxc_mi355x_encode_slot_stride(uint32_t block_size);
ZXC_EXPORT int zxc_mi355x_encode_blocks_device(const void* d_src, uint64_t src_size, uint32_t block_size,
                                               int level, int with_checksum, void* d_slots,
                                               uint32_t* d_sizes, void* stream);
/* Same with a dictionary (reference: opts.dict of zxc_compress, src/lib/zxc_dispatch.c:700-733, and the [dict | block]
 * buffer of zxc_compress_block :1688-1697): every block's tables are seeded with d_dict[0..dict_size), matches may reach
 * into it. d_work is scratch of zxc_mi355x_encode_dict_work_size() bytes (one [dict | block] image per block). */
ZXC_EXPORT uint64_t zxc_mi355x_encode_dict_work_size(uint64_t src_size, uint32_t block_size, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_encode_blocks_dict_device(const void* d_src, uint64_t src_size, uint32_t block_size,
                                                    int level, int with_checksum, const void* d_dict,
                                                    uint32_t dict_size, void* d_work, void* d_slots,
                                                    uint32_t* d_sizes, void* stream);
/* Compaction: block i's d_sizes[i] bytes go to d_out + d_offsets[i] (prefix sums computed by the
 * caller, like seek_comp[] in src/lib/zxc_dispatch.c:761-776). */
ZXC_EXPORT int zxc_mi355x_gather_blocks_device(const void* d_slots, uint32_t block_size,
                                               const uint32_t* d_sizes, const uint64_t* d_offsets,
                                               void* d_out, uint32_t n_blocks, void* stream);

/* ---- whole archive, device to device (zxc_amd/csrc/zxc_frame_device.hip) ----
 * zxc_compress for a source that already lives in device memory: the blocks are encoded, the container (file header, EOF
 * block, seek table, footer, global hash) is written and the blocks are compacted, all on the device. The archive is byte for
 * byte the one zxc_compress writes for the same source, level, block_size, checksum_enabled and seekable.
 * Options are read like zxc_compress reads them (opts may be NULL); n_threads, progress_cb and user_data are ignored, and
 * opts->dict != NULL gives ZXC_ERROR_GPU_UNSUPPORTED (a dictionary in device memory: zxc_mi355x_compress_dict_device below).
 * Reads exactly d_src[0, src_size) (the encoder's over-read is served from a staged copy of the last block or two), writes
 * nothing at or past d_dst + dst_capacity; d_dst may have any alignment. d_work is scratch of at least
 * zxc_mi355x_compress_device_work_size() bytes, any alignment, owned by the call until *d_result is written. */

/* Bytes of device scratch zxc_mi355x_compress_device needs for src_size bytes under opts (0 when opts are invalid). */
ZXC_EXPORT uint64_t zxc_mi355x_compress_device_work_size(uint64_t src_size, const zxc_compress_opts_t* opts);

/* Compress d_src[0..src_size) into a complete v8 archive at d_dst[0..dst_capacity), asynchronously on `stream`.
 * Returns ZXC_OK once everything is enqueued, or a negative zxc_error_t for arguments / launch failures (synchronous):
 * NULL d_dst / d_work / d_result (or d_src with src_size > 0) -> ZXC_ERROR_NULL_INPUT, bad options as above,
 * work_size too small -> ZXC_ERROR_MEMORY, dst_capacity below the part of the archive known before encoding (header,
 * 8 (+4 with checksums) bytes per block, EOF block, seek table, footer) -> ZXC_ERROR_DST_TOO_SMALL; then, without a
 * device, ZXC_ERROR_GPU_UNAVAILABLE. No device allocation (beyond the encoder's stream-ordered scratch at levels 6-7)
 * and no host synchronisation. Calls on different streams with different work areas may run concurrently.
 * *d_result (device memory) receives the archive size or a negative zxc_error_t, written once, after the archive:
 * ZXC_ERROR_DST_TOO_SMALL when the encoded archive does not fit (nothing is compacted then), ZXC_ERROR_CORRUPT_DATA when
 * the encoder reported a block size outside [8 (+4), block_size + 64]. After an error the bytes of d_dst are undefined. */
ZXC_EXPORT int zxc_mi355x_compress_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity,
                                          const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size,
                                          int64_t* d_result, void* stream);

/* ---- and back (zxc_amd/csrc/zxc_unframe_device.hip, container rules in zxc_amd/csrc/zxc_container.h) ----
 * zxc_decompress for an archive that already lives in device memory: the container (file header, block headers, seek table, EOF
 * block, footer size, global hash) is parsed, validated and judged on the device, the blocks are decoded by the launch behind
 * zxc_mi355x_decode_blocks_device, and one 8-byte word says what zxc_decompress would have returned.
 * block_size is the archive's block size: the host sizes the grids and the work area with it and never reads the archive. The
 * writer of the archive knows it; anyone else asks zxc_mi355x_frame_info_device. The call launches
 * n_max + 1 jobs, n_max = ceil(dst_capacity / block_size): an archive with more blocks cannot fit, and the extra job lets a
 * failing block behind a full destination keep its precedence over ZXC_ERROR_DST_TOO_SMALL. */

/* Bytes of device scratch the call below needs (0 for arguments it would refuse: src_size < 28, block_size not a power of two in
 * [4 KiB, 2 MiB], more than 2^31 - 2 blocks of capacity). Does not depend on opts. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_device_work_size(uint64_t src_size, uint64_t dst_capacity, uint32_t block_size);

/* Decode the complete v8 archive d_src[0, src_size) into d_dst[0, dst_capacity), asynchronously on `stream`.
 * Returns ZXC_OK once everything is enqueued, or synchronously, in this order and before any device is touched: NULL d_src /
 * d_work / d_result, or NULL d_dst with dst_capacity > 0 -> ZXC_ERROR_NULL_INPUT; src_size < 28 -> ZXC_ERROR_SRC_TOO_SMALL;
 * block_size as above -> ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict != NULL -> ZXC_ERROR_GPU_UNSUPPORTED; d_dst not 16-byte aligned
 * -> ZXC_ERROR_GPU_UNSUPPORTED; work_size too small -> ZXC_ERROR_MEMORY; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * opts may be NULL; only checksum_enabled and dict are read.
 * No host synchronisation and no device allocation of its own (the decode launch keeps its per-stream buffers as it does for
 * zxc_mi355x_decode_blocks_device), capturable like that call; calls on different streams with different work areas may overlap.
 * Writes nothing at or past d_dst + dst_capacity: the decoders store 16 bytes at a time, so the blocks whose slot
 * [i * block_size, (i + 1) * block_size + 32) does not lie inside the capacity (at most three jobs) are decoded into the work
 * area and copied out, min(decoded size, capacity left) bytes each. d_src must be READABLE up to src_size + 64 (as d_comp of
 * zxc_mi355x_decode_blocks_device; the bytes are never used) and is never written. d_work is scratch of at least
 * zxc_mi355x_decompress_device_work_size() bytes, any alignment, owned by the call until *d_result is written.
 * opts->checksum_enabled with an archive that carries checksums: every block's trailer is verified by the decode launch and the
 * footer's global hash on the device; otherwise nothing is hashed. (The host cannot know whether the archive carries them, and
 * the decode launch takes that by value: such a call enqueues the decode launch over two job tables, of which the device fills
 * one; the jobs of the other are empty and cost a wavefront that exits at once.)
 * *d_result (device memory) receives, once, after the last byte of d_dst: the decoded size, or the negative zxc_error_t that
 * zxc_decompress returns for the same bytes, capacity and options, with the same precedence: file header (BAD_MAGIC, BAD_VERSION,
 * BAD_HEADER, BAD_BLOCK_SIZE; a dictionary id -> DICT_REQUIRED), no block decoded then; the first failing block in archive order;
 * a bad block header found at block k only if blocks 0..k-1 decode; DST_TOO_SMALL when block i's decoded size passes the capacity
 * left; footer size -> CORRUPT_DATA; global hash -> BAD_CHECKSUM. dst_capacity == 0 is the empty-frame probe: 0 for an empty
 * archive, else DST_TOO_SMALL. Two departures: a header block size other than the argument is ZXC_ERROR_BAD_BLOCK_SIZE; an
 * irregular frame (a block that is not the last decodes to something other than block_size: legal, written neither by the
 * reference encoder nor by this library) is ZXC_ERROR_GPU_UNSUPPORTED, because its blocks do not sit back to back in d_dst and
 * there is no host to fall back to. A seek table is used only when it provably describes the chain a header walk follows;
 * otherwise one workgroup walks the headers, a serial chain of loads: write archives for this call with seekable = 1.
 * After an error the bytes of d_dst[0, dst_capacity) are undefined. */
ZXC_EXPORT int zxc_mi355x_decompress_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity,
                                            uint32_t block_size, const zxc_decompress_opts_t* opts, void* d_work,
                                            uint64_t work_size, int64_t* d_result, void* stream);

/* The one call here that synchronises: copies the 16-byte file header and the 12-byte footer to the host, waits for `stream`, and
 * reports what a caller who did not write the archive needs to size the call above (any of the three outputs may be NULL).
 * decompressed_size is what zxc_get_decompressed_size gives for the archive (0 when the footer's size is implausible).
 * -> ZXC_OK, ZXC_ERROR_NULL_INPUT, ZXC_ERROR_SRC_TOO_SMALL, ZXC_ERROR_GPU_UNAVAILABLE, or the file header's error. */
ZXC_EXPORT int zxc_mi355x_frame_info_device(const void* d_src, uint64_t src_size, uint32_t* block_size,
                                            uint64_t* decompressed_size, int* has_checksum, void* stream);

/* ---- random access, device to device (zxc_amd/csrc/zxc_ranges_device.hip, rules in zxc_amd/csrc/zxc_ranges.h) ----
 * zxc_seekable_open and zxc_seekable_decompress_range for a seekable archive that already lives in device memory: the seek table
 * is read and judged on the device once (open), and then any number of calls fetch many ranges each, the ranges themselves lying
 * in device memory. Both calls return ZXC_OK once everything is enqueued, are asynchronous on `stream`, do not synchronise with
 * the host, allocate no device memory of their own (the decode launch keeps its per-stream buffers as it does for
 * zxc_mi355x_decode_blocks_device) and never write d_src. These calls take no dictionary: an archive written with one gives every
 * range ZXC_ERROR_DICT_REQUIRED (zxc_mi355x_decompress_ranges_dict_device below takes one). Block checksum trailers are skipped,
 * not verified, as in zxc_seekable_decompress_range. */

/* One range to fetch (24 bytes, device-visible layout). */
typedef struct zxc_dev_range {
    uint64_t offset;  /* first decoded byte wanted */
    uint64_t len;     /* bytes wanted */
    uint64_t dst_off; /* where they go: d_dst + dst_off */
} zxc_dev_range_t;

/* Bytes of the index of an archive of at most max_blocks blocks: a 64-byte header (status, block count, decoded size, checksum
 * flag, dictionary id) and one uint64_t archive offset per block plus one behind the last. */
ZXC_EXPORT uint64_t zxc_mi355x_seekable_index_size(uint32_t max_blocks);

/* zxc_seekable_open on the device, once per archive: d_index (16-byte aligned, caller-owned, read-only afterwards) receives the
 * index. max_blocks = ceil(decompressed_size / block_size), which the writer knows and zxc_mi355x_frame_info_device tells.
 * Synchronous errors, in this order, before any device is touched: NULL d_src / d_index -> ZXC_ERROR_NULL_INPUT; src_size < 44
 * -> ZXC_ERROR_SRC_TOO_SMALL; block_size not a power of two in [4 KiB, 2 MiB] -> ZXC_ERROR_BAD_BLOCK_SIZE; d_index not 16-byte
 * aligned -> ZXC_ERROR_GPU_UNSUPPORTED; index_size < zxc_mi355x_seekable_index_size(max_blocks) -> ZXC_ERROR_MEMORY; then, without
 * a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * The index's status word is ZXC_OK under exactly the conditions of zxc_seekable_open (file header, non-zero footer size, a SEK
 * block header with a valid check byte and length 4 nb where the footer says it is, every entry >= 8, the entries summing from
 * offset 16 to a valid EOF block header right in front of the SEK block), plus: the header's block size is the argument (else
 * ZXC_ERROR_BAD_BLOCK_SIZE), nb <= max_blocks (else ZXC_ERROR_MEMORY) and, a departure, no entry above 4 MiB (no legal block is
 * that large). A failed open stores the file header's own error where that is what failed, else ZXC_ERROR_CORRUPT_DATA, and every
 * non-empty range read through that index gets that status. Like the host's open it does not look at the block headers; the
 * decoder does when a block is used. */
ZXC_EXPORT int zxc_mi355x_seekable_open_device(const void* d_src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks,
                                               void* d_index, uint64_t index_size, void* stream);

/* Bytes of device scratch the call below needs; 0 for arguments it would refuse (block_size, n_ranges x J > 2^31 - 2). The host
 * never sees the ranges, only the promise that none is longer than max_len: a range of that length touches at most
 * J = (max_len - 1) / block_size + 2 blocks, the call launches n_ranges x J jobs, and every job has a slot of its own. The size is
 * at most n_ranges x J x (block_size + 64) + 44 x n_ranges x J + 1536. That is the price of not knowing the ranges on the host;
 * keep it down with a tight max_len, and keep the slots unused with dst_off = offset (mod 16), which lets every block that lies
 * inside a range decode straight into d_dst. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_ranges_device_work_size(uint32_t n_ranges, uint64_t max_len, uint32_t block_size);

/* For r in [0, n_ranges): decoded bytes [offset_r, offset_r + len_r) of the archive d_src[0, src_size), opened into d_index with
 * the same block_size, go to d_dst + dst_off_r; d_results[r] (device memory) receives, once, after that range's last byte, what
 * zxc_seekable_decompress_range returns for the same archive, offset, len and a destination of dst_capacity - dst_off_r bytes:
 * len == 0 -> 0 (whatever else is wrong); a failed index -> its status; len > max_len, or dst_off + len > dst_capacity ->
 * ZXC_ERROR_DST_TOO_SMALL; offset > total or len > total - offset -> ZXC_ERROR_SRC_TOO_SMALL; a dictionary id in the file header ->
 * ZXC_ERROR_DICT_REQUIRED; then the first failing covered block's status in block order, a covered block that decoded to fewer
 * bytes than the range needs of it being ZXC_ERROR_CORRUPT_DATA; else len. (An index opened with another block_size gives
 * ZXC_ERROR_BAD_BLOCK_SIZE, a src_size below the archive that was opened ZXC_ERROR_SRC_TOO_SMALL.)
 * d_ranges lies in device memory and is read on the stream: a kernel enqueued before the call may write it, a replayed graph may
 * see other ranges each time.
 * Synchronous errors, in this order: NULL d_src / d_index / d_work / d_results, NULL d_ranges with n_ranges > 0, NULL d_dst with
 * dst_capacity > 0 -> ZXC_ERROR_NULL_INPUT; block_size -> ZXC_ERROR_BAD_BLOCK_SIZE; d_dst not 16-byte aligned ->
 * ZXC_ERROR_GPU_UNSUPPORTED; n_ranges x J above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_ranges == 0 is ZXC_OK
 * here and enqueues nothing; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * Guarantees: nothing is written outside the destinations [dst_off_r, dst_off_r + len_r) of the valid ranges and d_work (a block
 * is decoded straight into d_dst only when all of it is wanted, its place is 16-byte aligned and its slot plus the 32 bytes the
 * decoders may store behind it end inside that range's destination; every other block goes through a slot of d_work and a copy).
 * A range that fails leaves its own destination bytes undefined and every other range untouched. Ranges may overlap in the
 * archive (a shared block is decoded once per range). Ranges whose destinations overlap are the caller's error: undefined bytes,
 * no fault. d_src must be READABLE up to src_size + 64 (as d_comp of zxc_mi355x_decode_blocks_device). d_work: any alignment, owned
 * by the call until the last result is written. Calls on different streams with different work areas may overlap and may share
 * one index. */
ZXC_EXPORT int zxc_mi355x_decompress_ranges_device(const void* d_src, uint64_t src_size, const void* d_index,
                                                   const zxc_dev_range_t* d_ranges, uint32_t n_ranges, uint64_t max_len,
                                                   void* d_dst, uint64_t dst_capacity, uint32_t block_size, void* d_work,
                                                   uint64_t work_size, int64_t* d_results, void* stream);

/* ---- the same three calls with a dictionary that lies in device memory (zxc_amd/csrc/zxc_dict_device.hip and the three files
 * above) ----
 * opts->dict of zxc_compress / zxc_decompress and zxc_seekable_set_dict, for callers whose dictionary, like their data, is in
 * device memory. A dictionary is described by a small host struct that every call reads when it is made and does not keep; what it
 * points to must stay valid and unchanged until the call's result is written. */
typedef struct zxc_dev_dict {          /* host struct; read at call time, not kept */
    const void*     d_content;         /* dictionary content in device memory, 1..65535 bytes */
    const void*     d_huf;             /* its 128-byte shared literal table in device memory, or NULL */
    const uint32_t* d_id;              /* one word in device memory, written by zxc_mi355x_dict_prepare_device */
    uint32_t        size;
} zxc_dev_dict_t;
/* No call reads d_content past `size` or d_huf past 128 bytes: the id pass loads inside the bytes it hashes, the encoder works on
 * [dict | block] images that a byte-wise copy makes, and the dictionary decode kernel fetches dictionary bytes one at a time after
 * checking the offset against `size`. (The host API allocates size + 128 + 64 for its own copy; nothing here needs that margin.
 * This rests on reading the three kernels: a test cannot see an over-read inside an allocator's rounding.)
 * A NULL zxc_dev_dict_t*, or one with size == 0, makes each call below behave exactly as its sibling without _dict. A host
 * dictionary has no meaning here: opts->dict != NULL stays ZXC_ERROR_GPU_UNSUPPORTED. */

/* *d_id = zxc_dict_id(content, size, huf), computed by one wavefront, asynchronously on `stream`, without synchronising with the
 * host: once per dictionary, before the first call that uses it on that stream (or behind an event). d_huf may be NULL.
 * Synchronous errors, in this order: NULL d_content or d_id -> ZXC_ERROR_NULL_INPUT; size == 0 -> ZXC_ERROR_NULL_INPUT;
 * size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. */
ZXC_EXPORT int zxc_mi355x_dict_prepare_device(const void* d_content, uint32_t size, const void* d_huf, uint32_t* d_id, void* stream);

/* zxc_mi355x_compress_device with a dictionary: the archive is byte for byte the one zxc_compress writes for the same source,
 * options, dictionary and table. The file header carries the dictionary flag and *d_id, so its bytes 6..15 (flags, id, check
 * bytes) are assembled on the device; as in zxc_compress the encoder is given the content only, the table enters the id alone.
 * The blocks go through the [dict | block] images of zxc_mi355x_encode_blocks_dict_device in chunks of
 * C = max(4096, 256 MiB / (block_size + dict_size)) blocks: one image area of min(nb, C) images is reused from chunk to chunk in
 * stream order, a loop of enqueues without synchronisation. The work size is at most the sibling's plus
 * min(nb, C) x (block_size + dict_size) + 4096. Reads exactly d_src[0, src_size): the images are copies already and their padding
 * serves the encoder's over-read, so they take the place of the sibling's staged copy of the last blocks.
 * Synchronous errors: the sibling's, in its order, with two additions behind the option checks: dict->size > 65535 ->
 * ZXC_ERROR_DICT_TOO_LARGE; NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_dict_device_work_size(uint64_t src_size, const zxc_compress_opts_t* opts, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_compress_dict_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity,
                                               const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                               uint64_t work_size, int64_t* d_result, void* stream);

/* zxc_mi355x_decompress_device with a dictionary: same contract, same work size (zxc_mi355x_decompress_device_work_size), and
 * *d_result is what zxc_decompress returns for the same bytes, capacity, options and dictionary. File-header errors and the
 * block-size departure come first, as in the sibling; then a header with a dictionary id gives ZXC_ERROR_DICT_REQUIRED without a
 * dictionary and ZXC_ERROR_DICT_MISMATCH with one whose *d_id differs, and no block is decoded in either case. A dictionary given
 * for an archive written without one is handed to the decoder all the same, as the host does. The blocks are decoded by the
 * dictionary kernel behind zxc_mi355x_decode_blocks_dict_device (one wavefront per block).
 * Synchronous errors: the sibling's, with dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0
 * -> ZXC_ERROR_NULL_INPUT behind the opts->dict check. */
ZXC_EXPORT int zxc_mi355x_decompress_dict_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity,
                                                 uint32_t block_size, const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict,
                                                 void* d_work, uint64_t work_size, int64_t* d_result, void* stream);

/* zxc_mi355x_decompress_ranges_device with a dictionary: same contract, index (zxc_mi355x_seekable_open_device stores the header's
 * dictionary id) and work size. Where the sibling answers ZXC_ERROR_DICT_REQUIRED: that without a dictionary,
 * ZXC_ERROR_DICT_MISMATCH when *d_id is not the index's id (every non-empty range, their destinations untouched), else the range is
 * decoded with the dictionary. Synchronous errors: the sibling's, with dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL
 * d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT behind the block_size check, as in the two calls above. */
ZXC_EXPORT int zxc_mi355x_decompress_ranges_dict_device(const void* d_src, uint64_t src_size, const void* d_index,
                                                        const zxc_dev_range_t* d_ranges, uint32_t n_ranges, uint64_t max_len,
                                                        void* d_dst, uint64_t dst_capacity, uint32_t block_size,
                                                        const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size,
                                                        int64_t* d_results, void* stream);
/* (The same two calls over ranges that carry the absolute device address of their own destination: zxc_mi355x_rangesv.h.) */

/* ---- many archives per call, device to device (zxc_amd/csrc/zxc_batch_device.hip, rules in zxc_amd/csrc/zxc_batch.h) ----
 * zxc_mi355x_decompress_device for many small, independent archives that already live in device memory (cache pages, shards,
 * column chunks, records compressed against one dictionary): one archive of a few blocks cannot fill the device and costs about
 * ten launches, a few thousand in one call cost four passes. The archives lie in one source area, the decoded bytes go to one
 * destination area, and a table in device memory says where each one lies and goes. */

/* One archive to decode (32 bytes, device-visible layout). */
typedef struct zxc_dev_item {
    uint64_t src_off;      /* the archive is d_src[src_off, src_off + src_size) */
    uint64_t src_size;
    uint64_t dst_off;      /* decoded bytes go to d_dst + dst_off, any alignment */
    uint64_t dst_capacity; /* at most this many */
} zxc_dev_item_t;

/* Bytes of device scratch the call below needs; 0 for arguments it would refuse (block_size, n_items x J > 2^31 - 2). Does not
 * depend on opts. The host never sees the items, only the promise that none decodes to more than max_capacity bytes: the call
 * launches J = ceil(max_capacity / block_size) + 1 jobs per item (the n_max + 1 of zxc_mi355x_decompress_device, for the same
 * reason), and every job has a slot of its own. The size is at most
 * n_items x J x (block_size + 64) + 56 x n_items x J + 128 x n_items + 1536: the slots, two job tables and two status tables
 * (see checksum_enabled below), a record per item. That is the price of not knowing the items on the host; keep it down with a
 * tight max_capacity. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_batch_device_work_size(uint32_t n_items, uint64_t max_capacity, uint32_t block_size);

/* For r in [0, n_items): the complete v8 archive d_src[src_off_r, src_off_r + src_size_r) is decoded to d_dst + dst_off_r,
 * asynchronously on `stream`; d_results[r] (device memory) receives, once, after that item's last byte, what zxc_decompress
 * returns for the same bytes, options and the capacity cap_r = min(dst_capacity_r, max_capacity, dst_capacity - dst_off_r) (0 when
 * dst_off_r > dst_capacity): the decoded size or the negative zxc_error_t, with the precedence zxc_mi355x_decompress_device
 * documents (file header; the first failing block in archive order; a bad block header only behind decoded blocks;
 * DST_TOO_SMALL; footer size; global hash). cap_r == 0 is the empty-frame probe. That call's two departures hold per item: a
 * header block size other than block_size is ZXC_ERROR_BAD_BLOCK_SIZE, an irregular frame ZXC_ERROR_GPU_UNSUPPORTED. Two more,
 * decided on the device with nothing read for the item: src_size_r < 28 -> ZXC_ERROR_SRC_TOO_SMALL; src_off_r + src_size_r >
 * src_capacity (compared without overflow) -> ZXC_ERROR_SRC_TOO_SMALL. An archive written with a dictionary is
 * ZXC_ERROR_DICT_REQUIRED here (zxc_mi355x_decompress_batch_dict_device below takes one).
 * d_items lies in device memory and is read on the stream: a kernel enqueued before the call may write it, a replayed graph may
 * see other items each time. One thread per item walks that item's block headers, as zxc_decompress does (a seek table is not
 * looked at), for at most ceil(cap_r / block_size) + 1 blocks; all items' blocks are decoded by one launch behind
 * zxc_mi355x_decode_blocks_device. An archive of many blocks belongs in zxc_mi355x_decompress_device: here its walk is serial,
 * and every item pays for J job slots, of which the unused ones cost a wavefront that exits at once.
 * opts may be NULL; only checksum_enabled and dict are read. opts->checksum_enabled verifies per item, when that item's header
 * carries checksums: every block's trailer by the decode launch, the footer's global hash folded while the headers are walked.
 * Items with and without checksums may be mixed: such a call enqueues the decode launch over two job tables, of which each item
 * fills one.
 * Synchronous errors, in this order, before any device is touched: NULL d_src / d_work / d_results, NULL d_items with
 * n_items > 0, NULL d_dst with dst_capacity > 0 -> ZXC_ERROR_NULL_INPUT; block_size not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict != NULL -> ZXC_ERROR_GPU_UNSUPPORTED; d_dst not 16-byte aligned ->
 * ZXC_ERROR_GPU_UNSUPPORTED; n_items x J above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_items == 0 is ZXC_OK
 * here and enqueues nothing; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * Guarantees: nothing is written outside [dst_off_r, dst_off_r + cap_r) of each item and d_work (a block is decoded straight
 * into d_dst only when its place d_dst + dst_off_r + i x block_size is 16-byte aligned and (i + 1) x block_size + 32 <= cap_r;
 * every other block goes through its slot of d_work and a copy of min(decoded size, capacity left) bytes). An item that fails
 * leaves its own destination bytes undefined and every other item untouched. Items whose destinations overlap are the caller's
 * error: undefined bytes, no fault. d_src must be READABLE up to src_capacity + 64 (as d_comp of
 * zxc_mi355x_decode_blocks_device) and is never written. No host synchronisation and no device allocation of its own (the decode
 * launch keeps its per-stream buffers as it does for zxc_mi355x_decode_blocks_device). d_work: any alignment, owned by the call
 * until the last result is written. Calls on different streams with different work areas may overlap. */
ZXC_EXPORT int zxc_mi355x_decompress_batch_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                                  uint32_t n_items, uint64_t max_capacity, void* d_dst, uint64_t dst_capacity,
                                                  uint32_t block_size, const zxc_decompress_opts_t* opts, void* d_work,
                                                  uint64_t work_size, int64_t* d_results, void* stream);

/* The call above with a dictionary in device memory that the whole batch shares: same contract and work size. Per item, behind
 * the file-header errors and the block-size departure: a header with a dictionary id gives ZXC_ERROR_DICT_REQUIRED without a
 * dictionary and ZXC_ERROR_DICT_MISMATCH with one whose *d_id differs, and no block of that item is decoded; a dictionary given
 * to an item written without one is handed to the decoder all the same, as the host does. Synchronous errors: the sibling's,
 * with dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT behind
 * the opts->dict check. */
ZXC_EXPORT int zxc_mi355x_decompress_batch_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                                       uint32_t n_items, uint64_t max_capacity, void* d_dst,
                                                       uint64_t dst_capacity, uint32_t block_size,
                                                       const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict,
                                                       void* d_work, uint64_t work_size, int64_t* d_results, void* stream);

/* ---- many buffers per call, device to device (zxc_amd/csrc/zxc_cbatch_device.hip, rules in zxc_amd/csrc/zxc_cbatch.h) ----
 * zxc_mi355x_compress_device for many small, independent buffers that already live in device memory: the write side of the
 * calls above. One source of a few blocks fills a sliver of the device and costs about eight launches and a work area of its own;
 * a few thousand in one call cost a handful of launches. The buffers lie in one source area, the archives go to one destination
 * area, and a zxc_dev_item_t table in device memory says where each one lies and goes: src_off / src_size are the buffer to
 * compress, dst_off / dst_capacity where its archive goes and how large it may be (size each with zxc_compress_bound). With
 * d_results as the sizes, the item table of a compress call is therefore almost the item table of the decompress call. */

/* Bytes of device scratch the call below needs; 0 for arguments it would refuse (options as zxc_mi355x_compress_device_work_size,
 * n_items x J > 2^31 - 2). The host never sees the items, only the promise that none is larger than max_size bytes: the call
 * launches J = max(1, ceil(max_size / block_size)) jobs per item, of which an item uses as many as it has blocks, and every job
 * has an encoder slot of S = zxc_mi355x_encode_slot_stride(block_size) bytes. The size is at most
 * n_items x J x (S + 28) + 64 x n_items + 1536: the slots, per job a table entry, a size and an archive offset, a record per item.
 * That is the price of not knowing the items on the host; keep it down with a tight max_size. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_batch_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts);

/* For r in [0, n_items): d_src[src_off_r, src_off_r + src_size_r) is compressed into a complete v8 archive at d_dst + dst_off_r,
 * asynchronously on `stream`; d_results[r] (device memory) receives, once, after that item's last byte, the archive size or a
 * negative zxc_error_t. The archive is byte for byte the one zxc_compress of this library (and zxc_mi355x_compress_device) writes
 * for the same source, level, block_size, checksum_enabled and seekable; it does not depend on the bytes around the item.
 * Per item, decided on the device in this order, with cap_r = min(dst_capacity_r, dst_capacity - dst_off_r) (0 when dst_off_r >
 * dst_capacity): src_off_r + src_size_r > src_capacity (compared without overflow) -> ZXC_ERROR_SRC_TOO_SMALL; src_size_r >
 * max_size -> ZXC_ERROR_OVERFLOW; cap_r below the part of the archive known before encoding (header, 8 (+4 with checksums) bytes
 * per block, EOF block, seek table, footer) -> ZXC_ERROR_DST_TOO_SMALL; none of these items' bytes is read and no block of theirs
 * is encoded. Behind the encoder: a block size outside [8 (+4), block_size + 64] -> ZXC_ERROR_CORRUPT_DATA; an archive larger
 * than cap_r -> ZXC_ERROR_DST_TOO_SMALL. An item that fails has nothing written to its destination.
 * d_items lies in device memory and is read on the stream: a kernel or copy enqueued before the call may write it, a replayed
 * graph may see other items each time. All items' blocks are encoded by one launch of the level's encoder over a job table (one
 * wavefront per job; the unused ones of an item's J exit at once); one thread per item then writes the container around them,
 * serially over the item's blocks, so this call is for items of few blocks: a source of many blocks belongs in
 * zxc_mi355x_compress_device. The archives are not packed back to back: each goes where its item says
 * (zxc_mi355x_compress_pack_device below packs them).
 * Options are read like zxc_mi355x_compress_device reads them (opts may be NULL: level 3, 512 KiB blocks); n_threads, progress_cb
 * and user_data are ignored.
 * Synchronous errors, in this order, before any device is touched: NULL d_src / d_work / d_results, NULL d_items with
 * n_items > 0, NULL d_dst with dst_capacity > 0 -> ZXC_ERROR_NULL_INPUT; block_size not a power of two in [4 KiB, 2 MiB] ->
 * ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict != NULL -> ZXC_ERROR_GPU_UNSUPPORTED (a dictionary in device memory: the call below);
 * n_items x J above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_items == 0 is ZXC_OK here and enqueues nothing;
 * then, without a device, ZXC_ERROR_GPU_UNAVAILABLE.
 * Guarantees: nothing is written outside [dst_off_r, dst_off_r + size_r) of the items that succeed and d_work; a failing item
 * leaves every other item untouched. d_dst and dst_off_r may have any alignment. Items whose destinations overlap are the
 * caller's error: undefined bytes, no fault. d_src must be READABLE up to src_capacity + 64 (the encoder compares 16 bytes at a
 * time and reads up to 32 bytes past a block; the bytes themselves are never used) and is never written. No host synchronisation
 * and no device allocation (beyond the encoder's stream-ordered scratch at levels 6-7). d_work: any alignment, owned by the call
 * until the last result is written. Calls on different streams with different work areas may overlap. */
ZXC_EXPORT int zxc_mi355x_compress_batch_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                                uint32_t n_items, uint64_t max_size, void* d_dst, uint64_t dst_capacity,
                                                const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size,
                                                int64_t* d_results, void* stream);

/* The call above with a dictionary in device memory that the whole batch shares: every archive is the one zxc_compress writes
 * with that dictionary, its file header carrying the dictionary flag and *d_id (zxc_mi355x_compress_dict_device). The blocks are
 * encoded from [dict | block] images in chunks of C = max(4096, 256 MiB / (block_size + dict_size)) jobs: one image area of
 * min(n_items x J, C) images is reused from chunk to chunk in stream order. The work size is at most the sibling's plus
 * min(n_items x J, C) x (block_size + dict_size) + 320 (0 also for dict_size > 65535); with dict_size 0, and in the call with a
 * NULL dict or one of size 0, everything is the sibling's. The images are copies of exactly the items' bytes.
 * Synchronous errors: the sibling's, with dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0
 * -> ZXC_ERROR_NULL_INPUT behind the opts->dict check. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_batch_dict_device_work_size(uint32_t n_items, uint64_t max_size,
                                                                   const zxc_compress_opts_t* opts, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_compress_batch_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                                     uint32_t n_items, uint64_t max_size, void* d_dst, uint64_t dst_capacity,
                                                     const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                                     uint64_t work_size, int64_t* d_results, void* stream);

/* ---- many buffers per call, packed back to back (zxc_amd/csrc/zxc_cbatch_device.hip, rules in zxc_amd/csrc/zxc_cpack.h) ----
 * zxc_mi355x_compress_batch_device wants a destination of zxc_compress_bound per item, because nobody knows an archive's size
 * before the call, and leaves the archives with gaps of unknown size between them. This call takes no destination per item: it
 * lays the archives out itself, one behind the other in table order, and writes the table with which
 * zxc_mi355x_decompress_batch_device finds them again. No size or offset is ever known to the host. */

/* Bytes of device scratch the call below needs; 0 for whatever zxc_mi355x_compress_batch_device_work_size answers 0. The size is
 * that call's plus the words of the layout's scan, one 64-bit sum per tile of 1024 items and the end word: at most
 * n_items x J x (S + 28) + 64 x n_items + 1536 + 8 x ceil(n_items / 1024) + 256. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_pack_device_work_size(uint32_t n_items, uint64_t max_size, const zxc_compress_opts_t* opts);

/* zxc_mi355x_compress_batch_device with the archives packed. Of d_items[r] only src_off and src_size are read (dst_off and
 * dst_capacity are not looked at: the table of a zxc_mi355x_compress_batch_device call can be passed as it is); the table is
 * device data read on the stream, as there.
 * Layout: an item is SIZED when its source lies inside d_src[0, src_capacity), src_size_r <= max_size and the encoder left legal
 * block sizes for it; its archive size size_r is the one zxc_compress gives for those bytes and options. The sized items are laid
 * out in table order: at_r = the end of the sized item in front of it rounded up to `align`, the first at 0. Items that are not
 * sized take no room. The layout does not depend on dst_capacity. *d_total (device memory) receives the end at_r + size_r of the
 * last sized item, 0 when there is none, whether or not everything fits: it is the dst_capacity with which everything fits, so a
 * caller whose capacity was too small learns the right one from one word. *d_total is never an error word.
 * Per item, decided on the device in this order: src_off_r + src_size_r > src_capacity (compared without overflow) ->
 * ZXC_ERROR_SRC_TOO_SMALL; src_size_r > max_size -> ZXC_ERROR_OVERFLOW (after either, nothing of the item is read and no block of
 * it is encoded); behind the encoder, a block size outside [8 (+4), block_size + 64] -> ZXC_ERROR_CORRUPT_DATA; at_r + size_r >
 * dst_capacity -> ZXC_ERROR_DST_TOO_SMALL, and nothing of the item is written; else the archive is written at d_dst + at_r and
 * d_results[r] = size_r. The archive is byte for byte the one zxc_mi355x_compress_batch_device and zxc_compress of this library
 * write for that buffer and those options. Offsets only grow and every archive has at least 36 bytes, so the items that fit are a
 * prefix of the sized ones.
 * d_packed[r] (n_items entries, device memory) is the item of zxc_mi355x_decompress_batch_device that restores buffer r. For an
 * item that was written: src_off = at_r, src_size = size_r, dst_off = d_items[r].src_off, dst_capacity = d_items[r].src_size. For
 * every other item src_off = 0 and src_size = 0, which that call answers with ZXC_ERROR_SRC_TOO_SMALL without reading anything
 * (dst_off and dst_capacity are the item's all the same). d_packed may be d_items itself: the plan keeps what it needs in the
 * item's record, and the packed table is written by the last stage. Any other overlap is the caller's error.
 * Synchronous errors, in this order, before any device is touched: NULL d_src / d_work / d_results / d_packed / d_total, NULL
 * d_items with n_items > 0, NULL d_dst with dst_capacity > 0 -> ZXC_ERROR_NULL_INPUT; block_size not a power of two in [4 KiB,
 * 2 MiB] -> ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict != NULL -> ZXC_ERROR_GPU_UNSUPPORTED; align not a power of two in [1, 4096] ->
 * ZXC_ERROR_GPU_UNSUPPORTED; n_items x J above 2^31 - 2, or work_size too small -> ZXC_ERROR_MEMORY; n_items == 0 is ZXC_OK here,
 * enqueues nothing and does not write *d_total; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. dst_capacity == 0 with a NULL
 * d_dst is legal, the sizing run: every sized item gets ZXC_ERROR_DST_TOO_SMALL, and *d_total holds the need.
 * Guarantees: nothing is written outside [at_r, at_r + size_r) of the written items, d_work, d_packed, d_results and d_total; the
 * alignment gaps between archives, and everything at and past *d_total or dst_capacity, are left as they were. d_dst may have
 * any alignment (at_r is aligned relative to d_dst). d_src must be READABLE up to src_capacity + 64 and is never written, as in
 * the sibling. No host synchronisation and no device allocation (beyond the encoder's stream-ordered scratch at levels 6-7).
 * d_work: any alignment, owned by the call until the last result is written; the result words, the packed table and *d_total are
 * written once, behind the last archive byte. Calls on different streams with different work areas may overlap. */
ZXC_EXPORT int zxc_mi355x_compress_pack_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                               uint32_t n_items, uint64_t max_size, void* d_dst, uint64_t dst_capacity, uint32_t align,
                                               const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size,
                                               zxc_dev_item_t* d_packed, int64_t* d_results, uint64_t* d_total, void* stream);

/* The call above with a dictionary in device memory that the whole batch shares, as zxc_mi355x_compress_batch_dict_device: every
 * header carries the dictionary flag and *d_id, and the archives go back through zxc_mi355x_decompress_batch_dict_device. The work
 * size is at most the sibling's plus min(n_items x J, C) x (block_size + dict_size) + 320 (0 also for dict_size > 65535); a NULL
 * dict, or one of size 0, is the call without one. Synchronous errors: the sibling's, with dict->size > 65535 ->
 * ZXC_ERROR_DICT_TOO_LARGE and NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT behind the opts->dict check and in
 * front of the one of align. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_pack_dict_device_work_size(uint32_t n_items, uint64_t max_size,
                                                                  const zxc_compress_opts_t* opts, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_compress_pack_dict_device(const void* d_src, uint64_t src_capacity, const zxc_dev_item_t* d_items,
                                                    uint32_t n_items, uint64_t max_size, void* d_dst, uint64_t dst_capacity,
                                                    uint32_t align, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict,
                                                    void* d_work, uint64_t work_size, zxc_dev_item_t* d_packed, int64_t* d_results,
                                                    uint64_t* d_total, void* stream);

/* ---- one archive from many pieces, device to device (zxc_amd/csrc/zxc_append_device.hip, rules in zxc_amd/csrc/zxc_append.h) ----
 * zxc_mi355x_compress_device wants the whole source in one device buffer, a work area of about twice the source and a destination
 * of zxc_compress_bound: compressing S bytes that lie in HBM costs about 3 S more HBM, and a list of tensors (a state dict,
 * optimizer shards, pages produced step by step) has to be concatenated first. A session takes the source in pieces, as
 * zxc_cstream_* does for host memory, and writes one archive: its work area is sized by the largest piece, not by the source. */

/* The session: a host struct the caller owns, with no allocation behind it. begin fills it, end spends it; it may be dropped at
 * any time (what is enqueued runs on). One session is one thread's at a time. */
typedef struct zxc_dev_cappend { uint64_t opaque[16]; } zxc_dev_cappend_t;

/* Bytes of device scratch a session needs; 0 for arguments begin would refuse (options as zxc_mi355x_compress_device_work_size,
 * max_piece < block_size, more than 2^31 - 1 blocks in max_total or jobs in a piece). max_total is the most bytes the session
 * will be given in all, max_piece the most it works on at a time: an append of more is processed in pieces of at most max_piece
 * bytes. A piece has J = max_piece / block_size + 2 jobs, each with an encoder slot of S = zxc_mi355x_encode_slot_stride(block_size)
 * bytes, which every piece reuses. With NB = ceil(max_total / block_size) the size is at most
 * J x (S + 28) + 16 x ceil(J / 1024) + 3 x (block_size + 64) + 4096, and with opts->seekable + 4 x NB: the slots, per job a table
 * entry, a size and an archive offset, three words per tile of 1024 jobs, two carry areas and a stage area, the seek-table entries
 * until end puts them behind the blocks. Without a seek table it does not depend on max_total. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_append_device_work_size(uint64_t max_total, uint64_t max_piece, const zxc_compress_opts_t* opts);

/* begin, any number of appends, end: afterwards d_dst holds byte for byte the archive zxc_mi355x_compress_device (and zxc_compress
 * of this library) writes for the concatenation of the appended bytes with the same level, block_size, checksum_enabled and
 * seekable, however the source was cut: appends of 0 bytes, of less than a block, many of those in a row, appends that end inside
 * a block. *d_result (device memory) is written once, last, by end: the archive size, or the negative zxc_error_t
 * zxc_mi355x_compress_device would have stored for that source and dst_capacity (where that call refuses a capacity below the
 * part of the archive known before encoding synchronously, the session, which cannot know the source at begin, stores
 * ZXC_ERROR_DST_TOO_SMALL). begin + end gives the archive of the empty source.
 * Everything is asynchronous on `stream`: no host synchronisation, no device allocation (beyond the encoder's stream-ordered
 * scratch at levels 6-7). The calls of one session must be in stream order with each other (one stream, or the caller's events);
 * sessions with different work areas and destinations may run concurrently. d_work (any alignment) and d_dst are the session's
 * from begin until *d_result is written.
 * An append reads exactly d_src[0, n), whatever its alignment; d_src may be reused or freed, in stream order, behind the call.
 * The host knows every n, so it knows the carry, (bytes so far) mod block_size, and each piece's exact grid; nothing about the
 * shape is decided on the device. The trailing partial block of an append is copied into a carry area of d_work, the next
 * append's first block is assembled there from the carry and the head of the new bytes, and end encodes what is left there as the
 * short last block. A whole block is encoded where it lies in d_src when the encoder's 32-byte over-read stays inside the piece,
 * else (the last whole block of a piece, at most) from a zero-padded copy, as zxc_mi355x_compress_device stages its last blocks.
 * An append of more than max_piece bytes is a loop of enqueues over pieces cut on the archive's block boundaries, which reuse
 * the slots in stream order. Per piece, on the device: every block size is checked against [8 (+4), block_size + 64]
 * (ZXC_ERROR_CORRUPT_DATA); the blocks are gathered right behind the previous piece's; the seek-table entries join an array in
 * d_work; the global hash is carried on. Once the blocks so far, plus the EOF block, the seek table for them and the footer, exceed
 * dst_capacity the session's status is ZXC_ERROR_DST_TOO_SMALL and no further block is gathered: the archive only grows, so this
 * is exactly zxc_mi355x_compress_device's size > dst_capacity. Both errors stay and end reports them. Nothing is written at or
 * past d_dst + dst_capacity; d_dst may have any alignment; after an error its bytes are undefined.
 * Options are read like zxc_mi355x_compress_device reads them (opts may be NULL: level 3, 512 KiB blocks). opts->dict != NULL is
 * ZXC_ERROR_GPU_UNSUPPORTED: a dictionary in device memory goes through zxc_mi355x_compress_begin_dict_device below.
 * Synchronous errors, before any device is touched, in this order. begin: NULL cs / d_dst / d_work -> ZXC_ERROR_NULL_INPUT;
 * opts->dict -> ZXC_ERROR_GPU_UNSUPPORTED; block_size not a power of two in [4 KiB, 2 MiB], max_piece < block_size, more than
 * 2^31 - 1 blocks in max_total (or jobs in a piece) -> ZXC_ERROR_BAD_BLOCK_SIZE; work_size too small -> ZXC_ERROR_MEMORY;
 * dst_capacity below the empty archive -> ZXC_ERROR_DST_TOO_SMALL; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. append:
 * NULL cs, NULL d_src with n > 0 -> ZXC_ERROR_NULL_INPUT; a session that was never begun or is ended -> ZXC_ERROR_NULL_INPUT;
 * bytes so far + n > max_total (compared without overflow) -> ZXC_ERROR_OVERFLOW, with nothing enqueued and the session as it
 * was. end: NULL cs / d_result, a session never begun or ended -> ZXC_ERROR_NULL_INPUT; afterwards the struct is spent. A launch
 * failure (ZXC_ERROR_GPU_UNAVAILABLE, ZXC_ERROR_MEMORY) in append or end leaves part of the work enqueued: the session is spent,
 * *d_result is not written, and the bytes of d_dst are undefined. */
ZXC_EXPORT int zxc_mi355x_compress_begin_device(zxc_dev_cappend_t* cs, void* d_dst, uint64_t dst_capacity, uint64_t max_total,
                                                uint64_t max_piece, const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size,
                                                void* stream);
ZXC_EXPORT int zxc_mi355x_compress_append_device(zxc_dev_cappend_t* cs, const void* d_src, uint64_t n, void* stream);
ZXC_EXPORT int zxc_mi355x_compress_end_device(zxc_dev_cappend_t* cs, int64_t* d_result, void* stream);

/* The session with a dictionary in device memory: begin with a zxc_dev_dict_t, then zxc_mi355x_compress_append_device and
 * zxc_mi355x_compress_end_device as above, which serve both kinds of session. After begin, any number of appends and end, d_dst
 * holds byte for byte the archive zxc_mi355x_compress_dict_device (and zxc_compress of this library with opts->dict) writes for
 * the concatenation of the appended bytes with the same level, block_size, checksum_enabled, seekable and dictionary, however the
 * source was cut. The file header carries the dictionary flag and *d_id, which is read on the device when end writes the header;
 * as in zxc_compress the encoder is given the content only, d_huf enters the id alone. *d_result is written once, last, by end:
 * the archive size, or the error zxc_mi355x_compress_dict_device would store for that source and capacity, with the one departure
 * of the session above (ZXC_ERROR_DST_TOO_SMALL is stored where that call refuses a capacity synchronously). What dict points to
 * must stay valid and unchanged until *d_result is written; the struct itself is read by begin and not kept.
 * Every block is encoded from a [dict | block] image, as in zxc_mi355x_compress_dict_device: a piece's jobs go through the
 * encoder in chunks of C = max(4096, 256 MiB / (block_size + dict_size)) jobs, and one image area of min(J, C) images is reused
 * from chunk to chunk in stream order. The work size is the sibling's plus that area: at most
 * J x (S + 28) + 16 x ceil(J / 1024) + 3 x (block_size + 64) + 4 x NB (seekable only) + 4096
 *   + min(J, C) x (block_size + dict_size) + 320,
 * exactly zxc_mi355x_compress_append_device_work_size with dict_size == 0, and 0 for dict_size > 65535 and for whatever the
 * sibling refuses. An append still reads exactly d_src[0, n): an image is a copy with padding behind it, so no block is staged
 * (the stage area goes unused) and the head of an append that completes the waiting block goes from d_src straight into that
 * block's image, behind the waiting bytes, without passing through the carry area. The trailing partial block is carried as above.
 * A NULL dict, or one with size == 0, makes begin behave exactly as zxc_mi355x_compress_begin_device: same work size, same bytes.
 * Synchronous errors of begin: the sibling's, in its order, with two additions directly behind the opts->dict check:
 * dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE; NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT. opts->dict != NULL
 * stays ZXC_ERROR_GPU_UNSUPPORTED. A refused begin leaves the struct alone. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_append_dict_device_work_size(uint64_t max_total, uint64_t max_piece,
                                                                    const zxc_compress_opts_t* opts, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_compress_begin_dict_device(zxc_dev_cappend_t* cs, void* d_dst, uint64_t dst_capacity, uint64_t max_total,
                                                     uint64_t max_piece, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict,
                                                     void* d_work, uint64_t work_size, void* stream);

/* Append a table of buffers: the writev of the session (rules in zxc_amd/csrc/zxc_appendv.h). One append per tensor of a state
 * dict is about six launches per tensor, and the encode launch of a small tensor holds a handful of blocks, one wavefront each;
 * concatenating the tensors first is the second copy of everything the session exists to avoid. Here one call takes a table of
 * (base, len) entries that lies in device memory and appends their concatenation X, in table order: the blocks of a chunk of at
 * most max_piece bytes are cut from X, not from the entries, so one encode launch carries max_piece / block_size blocks however
 * small the entries are. The call is exactly zxc_mi355x_compress_append_device(cs, X, total, stream): after end the archive and
 * *d_result are byte for byte what the session gives for X. append and appendv mix freely in one session, in any order, with a
 * carry across every boundary.
 * The table: d_iov lies in device memory and is read on the stream (a kernel or copy enqueued before the call may write it, a
 * replayed graph may see other pointers). The host knows only n_iov and total, the caller's promise of the sum of the lengths:
 * that gives it what it knows in append (carry, chunk cuts, grids), so nothing about the launch shape is decided on the device.
 * Entries of length 0 are legal anywhere and their base is not looked at; an entry may have any alignment; entries may overlap
 * each other; entries that overlap d_dst, the work area or d_scratch are the caller's error. The call reads exactly
 * [base, base + len) of every entry: nothing is promised readable behind an entry.
 * Stream order: once per call a scan (exclusive prefix sums of the lengths into the scratch, and the table check, in three tile
 * passes), then per chunk prep, encode, tiles, advance, scatter, gather as in append. Prep runs one workgroup per job: the head
 * that completes the waiting block and the tail are gathered into the session's carry areas; a whole block that lies inside one
 * entry with its 32-byte over-read inside that same entry is encoded in place; every other whole block is gathered into an image
 * in the scratch with 64 zero bytes behind it. The gather is destination-driven (a thread owns 16-byte units of the image, finds
 * the entry of its first byte by a search over the start offsets, and takes the unit with one 16-byte load when it lies inside
 * one entry, else byte by byte from consecutive entries), so its cost does not depend on how small the entries are.
 * Scratch: d_scratch (any alignment) is the call's own until the work this call enqueued has run; a later appendv on the same
 * stream may reuse it. It is not part of the session's work area. With J = max_piece / block_size + 2 its size is at most
 * 8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + J x (block_size + 256) + 4096: the entries' start offsets, the words of the scan per
 * tile of 1024 entries, one image per job of a chunk, alignment. The size function returns 0 for options or a max_piece that begin
 * would refuse; max_piece is the session's.
 * Table errors are found on the device and become the session's sticky status, which end reports: an error the session already
 * has stays; else an entry with len > 0 and base == 0 -> ZXC_ERROR_NULL_INPUT; else an entry longer than total, or a sum above
 * total (compared without overflow) -> ZXC_ERROR_OVERFLOW; else a sum below total -> ZXC_ERROR_SRC_TOO_SMALL. After any of these
 * no byte of any entry of that call is read and none of its blocks is encoded or gathered; the host's byte count has moved on by
 * total, as it cannot know.
 * Synchronous errors, before anything is enqueued and with the session as it was, in this order: NULL cs, NULL d_scratch, NULL
 * d_iov with n_iov > 0 -> ZXC_ERROR_NULL_INPUT; a session never begun or ended -> ZXC_ERROR_NULL_INPUT; a session begun with a
 * dictionary -> ZXC_ERROR_GPU_UNSUPPORTED (zxc_mi355x_compress_appendv_dict_device below serves it); n_iov == 0 with total > 0 -> ZXC_ERROR_SRC_TOO_SMALL; bytes so far + total > max_total
 * -> ZXC_ERROR_OVERFLOW; scratch_size too small -> ZXC_ERROR_MEMORY. n_iov == 0 with total == 0 is ZXC_OK and enqueues nothing.
 * A launch failure leaves the session spent, as in append. Asynchronous on `stream` and capturable like append: no host
 * synchronisation, no device allocation beyond the encoder's stream-ordered scratch at levels 6-7. */

/* One entry of a source table (16 bytes, device-visible layout): len bytes at the device address base. */
typedef struct zxc_dev_iov { uint64_t base; uint64_t len; } zxc_dev_iov_t;

ZXC_EXPORT uint64_t zxc_mi355x_compress_appendv_device_scratch_size(uint32_t n_iov, uint64_t max_piece,
                                                                    const zxc_compress_opts_t* opts);
ZXC_EXPORT int zxc_mi355x_compress_appendv_device(zxc_dev_cappend_t* cs, const zxc_dev_iov_t* d_iov, uint32_t n_iov,
                                                  uint64_t total, void* d_scratch, uint64_t scratch_size, void* stream);

/* The same call for a session begun with a dictionary (zxc_mi355x_compress_begin_dict_device): with X the concatenation of the
 * entries in table order it is exactly zxc_mi355x_compress_append_device(cs, X, total, stream) on that session, so after end the
 * archive and *d_result are byte for byte what zxc_mi355x_compress_dict_device writes for the concatenation of everything
 * appended, with the same options, dictionary and capacity, however the bytes were cut into calls and entries. append and
 * appendv_dict mix freely in one dictionary session, with a carry across every boundary.
 * The table, its rules, the table errors with their precedence and the sticky status are those of
 * zxc_mi355x_compress_appendv_device above, word for word: device data read on the stream; entries of length 0 legal anywhere,
 * their base not looked at; any alignment; exactly [base, base + len) of each entry is read; after a table error no entry of that
 * call is read and no block of it is encoded or gathered, and the host's byte count has moved on by total.
 * Stream order: once per call the scan, then per chunk of at most max_piece bytes the loop of a dictionary session's append over
 * at most C = min(J, zc_image_chunk(block_size, dict_size)) jobs: one launch gathers every job's [dict | block] image straight
 * from the entries into the session's own image area (the carried block takes the waiting bytes of the carry area and then the
 * head of X, which is copied nowhere else; one more workgroup of a chunk's first launch gathers the tail into the other carry
 * area), then the encode launch over those images; then tiles, advance, scatter, gather once per chunk. No block is encoded where
 * it lies: an image is a copy by construction.
 * Scratch: as above, but it holds no images, since every block is an image in the session's work area: the control word, the
 * entries' start offsets and the words of the scan, at most 8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + 4096 for dict_size in
 * [1, 65535]. For dict_size == 0 the size function returns zxc_mi355x_compress_appendv_device_scratch_size's value; it returns 0
 * for dict_size > 65535 and for options or a max_piece that begin would refuse. The call requires the size that belongs to the
 * session's own dict_size. A session begun without a dictionary (NULL dict or size 0) is served exactly as
 * zxc_mi355x_compress_appendv_device serves it: same launches, same bytes, same scratch need.
 * Synchronous errors, before anything is enqueued and with the session as it was, in this order: NULL cs, NULL d_scratch, NULL
 * d_iov with n_iov > 0 -> ZXC_ERROR_NULL_INPUT; a session never begun or ended -> ZXC_ERROR_NULL_INPUT; n_iov == 0 with total > 0
 * -> ZXC_ERROR_SRC_TOO_SMALL; bytes so far + total > max_total (compared without overflow) -> ZXC_ERROR_OVERFLOW; scratch_size
 * too small -> ZXC_ERROR_MEMORY. n_iov == 0 with total == 0 is ZXC_OK and enqueues nothing. A launch failure leaves the session
 * spent, as in append. Asynchronous on `stream` and capturable like append: no host synchronisation, no device allocation beyond
 * the encoder's stream-ordered scratch at levels 6-7. */
ZXC_EXPORT uint64_t zxc_mi355x_compress_appendv_dict_device_scratch_size(uint32_t n_iov, uint64_t max_piece,
                                                                         const zxc_compress_opts_t* opts, uint32_t dict_size);
ZXC_EXPORT int zxc_mi355x_compress_appendv_dict_device(zxc_dev_cappend_t* cs, const zxc_dev_iov_t* d_iov, uint32_t n_iov,
                                                       uint64_t total, void* d_scratch, uint64_t scratch_size, void* stream);

/* ---- one archive into many pieces, device to device (zxc_amd/csrc/zxc_take_device.hip, rules in zxc_amd/csrc/zxc_take.h) ----
 * zxc_mi355x_decompress_device wants one contiguous, 16-byte aligned destination of the whole decoded size: whoever wrote an
 * archive from a list of tensors with the session above needs a second copy of everything in HBM to read it back, and a device
 * copy per tensor. A take session is the mirror image of the append session and the device counterpart of pulling from
 * zxc_dstream_*: begin parses the archive once, every take delivers the next n decoded bytes to a destination of its own (the
 * tensors of a state dict, or one buffer that is reused layer by layer), end writes one result word. */

/* The session: a host struct the caller owns, with no allocation behind it. begin fills it, end spends it; it may be dropped at
 * any time (what is enqueued runs on). One session is one thread's at a time. */
typedef struct zxc_dev_dtake { uint64_t opaque[16]; } zxc_dev_dtake_t;

/* Bytes of device scratch a session needs; 0 for arguments begin would refuse (src_size < 28, block_size, max_piece < block_size,
 * more than 2^31 - 2 blocks in dst_capacity or jobs in a chunk). Does not depend on opts or a dictionary. dst_capacity is the
 * number of bytes the takes will ask for in all, max_piece the most a take works on at a time: a take of more is processed in
 * chunks of at most max_piece bytes. With n_jobs = ceil(dst_capacity / block_size) + 1 and J = max_piece / block_size + 2 the size
 * is at most 56 x n_jobs + 16 x ceil(n_jobs / 1024) + J x (block_size + 64 + 48) + 2 x (block_size + 64) + 4096: per block of the
 * capacity what zxc_mi355x_decompress_device keeps (two job tables and two status tables, see checksum_enabled there; three
 * words per tile of 1024 jobs), per job of a chunk a slot and its entry in two chunk tables, two carry slots. It grows with
 * dst_capacity exactly as zxc_mi355x_decompress_device_work_size does. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_take_device_work_size(uint64_t src_size, uint64_t dst_capacity, uint64_t max_piece,
                                                                uint32_t block_size);

/* begin, takes of dst_capacity bytes in all, end: the session decodes the complete v8 archive d_src[0, src_size) as if into one
 * destination of dst_capacity bytes that the caller hands over in pieces. dst_capacity plays exactly the role it has in
 * zxc_mi355x_decompress_device: the caller knows it as the writer, or from zxc_mi355x_frame_info_device. Take k delivers decoded
 * bytes [pos_k, pos_k + n_k) to d_dst_k[0, n_k), pos_k being the sum of the earlier n. *d_result (device memory) is written once,
 * last, by end: what zxc_mi355x_decompress_device (after the _dict begin: zxc_mi355x_decompress_dict_device) stores for the same
 * archive, dst_capacity, block_size, options and dictionary, that is the decoded size or the negative zxc_error_t with that
 * call's precedence and its two departures (a header block size other than block_size is ZXC_ERROR_BAD_BLOCK_SIZE, an irregular
 * frame ZXC_ERROR_GPU_UNSUPPORTED). On success the pieces, concatenated, are the bytes that call writes. dst_capacity == 0 is the
 * empty-frame probe: begin, then end.
 * Everything is asynchronous on `stream`: no host synchronisation, no device allocation of the session's own (the decode launch
 * keeps its per-stream buffers as it does for zxc_mi355x_decode_blocks_device). The calls of one session must be in stream order
 * with each other (one stream, or the caller's events); sessions with different work areas may run concurrently. d_work (any
 * alignment) is the session's from begin until *d_result is written. d_src is never written and must be READABLE up to src_size
 * + 64, as for zxc_mi355x_decompress_device, until then. A d_dst may be reused or freed, in stream order, behind its take.
 * begin enqueues the container stages of zxc_mi355x_decompress_device once, for n_jobs = ceil(dst_capacity / block_size) + 1
 * (clear, head, tiles, scan, scatter, walk; a non-seekable archive, or one whose table disagrees with its headers, takes the
 * header walk); the block index and one status word per block stay in d_work for the session. The host knows block_size, pos and
 * every n, so the plan of every take is the host's and nothing about the shape is decided on the device. d_dst of a take may have
 * any alignment. A block is decoded straight into the piece only when it lies wholly inside the piece, its place
 * d_dst + (i x block_size - pos) is 16-byte aligned and its slot plus 32 bytes ends inside the piece,
 * (i + 1) x block_size - pos + 32 <= n (the decoders store 16 bytes at a time; the rule of zxc_mi355x_decompress_batch_device);
 * every other block goes through a slot of d_work and a copy of min(decoded size, bytes wanted of it) bytes. A block that a take
 * ends inside is decoded once, into one of two carry slots that take turns; that take copies the block's head out and the next
 * takes copy their parts out of the same slot (any number of takes may lie wholly inside one block: they only copy). A take of
 * more than max_piece bytes is a loop of enqueues over chunks cut on the archive's block boundaries, each with at most J jobs and,
 * where the blocks cannot be decoded in place, J slots reused in stream order. Every block of the archive is decoded exactly once
 * per session. All copies of a chunk are enqueued behind its decode launches. With opts->checksum_enabled every chunk enqueues
 * the decode launch over two tables (verify_trailer 0 and 1), of which the head stage filled one, as in that call.
 * end decodes the one job behind the capacity, block n_max, into a slot (only its status counts: it lets a failing block behind
 * a full destination keep its precedence over DST_TOO_SMALL), then runs that call's events pass over the whole status table and
 * its result kernel. The verdict is taken at end because it is the first event in archive order over all blocks.
 * Guarantees: nothing is written outside [d_dst, d_dst + n) of each take and d_work. After an error, or at and past the decoded
 * size when the archive is shorter than dst_capacity, the bytes inside the pieces are undefined. After a file-header error
 * (dictionary errors included) no block is decoded and no piece is written.
 * opts may be NULL; only checksum_enabled and dict are read. opts->dict != NULL is ZXC_ERROR_GPU_UNSUPPORTED: a dictionary in
 * device memory goes through zxc_mi355x_decompress_begin_dict_device, with the DICT_REQUIRED / DICT_MISMATCH rules of
 * zxc_mi355x_decompress_dict_device; a NULL dict, or one of size 0, behaves as the sibling.
 * Synchronous errors, before any device is touched, in this order. begin: NULL ds / d_src / d_work -> ZXC_ERROR_NULL_INPUT;
 * src_size < 28 -> ZXC_ERROR_SRC_TOO_SMALL; block_size not a power of two in [4 KiB, 2 MiB], max_piece < block_size, more than
 * 2^31 - 2 blocks in dst_capacity or jobs in a chunk -> ZXC_ERROR_BAD_BLOCK_SIZE; opts->dict -> ZXC_ERROR_GPU_UNSUPPORTED; the
 * _dict begin: dict->size > 65535 -> ZXC_ERROR_DICT_TOO_LARGE, NULL d_content or d_id with size > 0 -> ZXC_ERROR_NULL_INPUT;
 * work_size too small -> ZXC_ERROR_MEMORY; then, without a device, ZXC_ERROR_GPU_UNAVAILABLE. A refused begin leaves the struct
 * alone. take: NULL ds, NULL d_dst with n > 0 -> ZXC_ERROR_NULL_INPUT; a session that was never begun or is ended ->
 * ZXC_ERROR_NULL_INPUT; bytes so far + n > dst_capacity (compared without overflow) -> ZXC_ERROR_OVERFLOW, with nothing enqueued
 * and the session as it was; n == 0 is ZXC_OK and enqueues nothing. end: NULL ds / d_result, a session never begun or ended ->
 * ZXC_ERROR_NULL_INPUT; fewer than dst_capacity bytes taken -> ZXC_ERROR_DST_TOO_SMALL, with nothing enqueued and the session as
 * it was (the verdict needs every block's status: the caller may take the rest and end again); afterwards the struct is spent. A
 * launch failure (ZXC_ERROR_GPU_UNAVAILABLE, ZXC_ERROR_MEMORY) in take or end leaves part of the work enqueued: the session is
 * spent and *d_result is not written. */
ZXC_EXPORT int zxc_mi355x_decompress_begin_device(zxc_dev_dtake_t* ds, const void* d_src, uint64_t src_size, uint64_t dst_capacity,
                                                  uint64_t max_piece, uint32_t block_size, const zxc_decompress_opts_t* opts,
                                                  void* d_work, uint64_t work_size, void* stream);
ZXC_EXPORT int zxc_mi355x_decompress_begin_dict_device(zxc_dev_dtake_t* ds, const void* d_src, uint64_t src_size,
                                                       uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size,
                                                       const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                                       uint64_t work_size, void* stream);
ZXC_EXPORT int zxc_mi355x_decompress_take_device(zxc_dev_dtake_t* ds, void* d_dst, uint64_t n, void* stream);
ZXC_EXPORT int zxc_mi355x_decompress_end_device(zxc_dev_dtake_t* ds, int64_t* d_result, void* stream);

/* Take into a table of buffers: the readv of the session (rules in zxc_amd/csrc/zxc_takev.h), the mirror of
 * zxc_mi355x_compress_appendv_device. One take per tensor of a state dict is a plan launch, one or two decode launches and a copy
 * launch per tensor, and the decode launch of a small tensor holds a handful of blocks, one wavefront each. Here one call delivers
 * the next `total` decoded bytes into a table of (base, len) entries that lies in device memory: with Y the concatenation of the
 * entries' destinations in table order, the call is exactly zxc_mi355x_decompress_take_device(ds, Y, total, stream). The blocks
 * of a chunk of at most max_piece bytes are cut from Y, not from the entries, so one decode launch carries max_piece / block_size
 * blocks however small the entries are. After end, *d_result is what the session stores for the same archive, capacity, options
 * and dictionary; on success the entries hold, in table order, the next `total` decoded bytes. take and takev mix freely in one
 * session, in any order: the block that a call ends inside waits in the carry slot for whichever call comes next. The call serves
 * sessions begun with and without a dictionary (the decode launch is the session's).
 * The table: d_iov lies in device memory and is read on the stream (a kernel or copy enqueued before the call may write it, a
 * replayed graph may see other pointers). The host knows only n_iov and total, the caller's promise of the sum of the lengths:
 * that gives it what it knows in take (position, chunk cuts, grids), so nothing about the launch shape is decided on the device.
 * Entries of length 0 are legal anywhere and their base is not looked at; an entry may have any alignment; entries that overlap
 * each other, d_src, the work area or d_scratch are the caller's error (undefined bytes, no fault). The call writes nothing
 * outside [base, base + len) of the entries, the session's work area and d_scratch: nothing is promised writable behind an entry.
 * Stream order: once per call a scan (appendv's three tile passes: exclusive prefix sums of the lengths into the scratch, and the
 * table check) and a fold of the verdict into the session, then per chunk plan, decode, copy as in take. The plan decides on the
 * device where each whole block is decoded: where it belongs when that place is 16-byte aligned and the block plus the decoders'
 * 32 bytes end inside that one entry; else in a slot of the work area. The copy moves a range that lies inside one entry with the
 * aligned 16-byte stores take uses; a range that meets an entry boundary is scattered (a lane owns 16-byte units of the slot,
 * finds the entry of its first byte by a search over the start offsets, and stores the unit with one 16-byte store of any
 * alignment when it lies inside one entry, else byte by byte into consecutive entries), so its cost does not depend on how small
 * the entries are.
 * Scratch: d_scratch (any alignment) is the call's own until the work this call enqueued has run; a later takev on the same
 * stream may reuse it. It is not part of the session's work area. With J = max_piece / block_size + 2 its size is at most
 * 8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + 16 x J + 4096: a control word, the entries' start offsets, the words of the scan per
 * tile of 1024 entries, one place record per job of a chunk, alignment. The size function returns 0 for a block_size or max_piece
 * that begin would refuse; max_piece and block_size are the session's.
 * Table errors are found on the device and become the session's result, which end stores: a session whose result is already
 * final (a file-header error, a dictionary error, the empty-frame probe, an earlier table error) keeps it; else an entry with
 * len > 0 and base == 0 -> ZXC_ERROR_NULL_INPUT; else an entry longer than total, or a sum above total (compared without overflow)
 * -> ZXC_ERROR_OVERFLOW; else a sum below total -> ZXC_ERROR_DST_TOO_SMALL (fewer destination bytes than promised). After any of
 * these no byte of any entry of that call is written and none of its blocks is decoded; every later copy of the session moves nothing
 * (the bytes of later pieces are undefined); the host's position has moved on by total, as it cannot know, and the session is still taken to the capacity and ended as
 * usual.
 * Synchronous errors, before anything is enqueued and with the session as it was, in this order: NULL ds, NULL d_scratch, NULL
 * d_iov with n_iov > 0 -> ZXC_ERROR_NULL_INPUT; a session never begun or ended -> ZXC_ERROR_NULL_INPUT; n_iov == 0 with total > 0
 * -> ZXC_ERROR_DST_TOO_SMALL; bytes so far + total > dst_capacity (compared without overflow) -> ZXC_ERROR_OVERFLOW; scratch_size
 * too small -> ZXC_ERROR_MEMORY. n_iov == 0 with total == 0 is ZXC_OK and enqueues nothing; n_iov > 0 with total == 0 enqueues the
 * scan alone (a non-empty entry is then an error). A launch failure leaves the session spent, as in take. Asynchronous on `stream`
 * and capturable like take: no host synchronisation, no device allocation of its own. */
ZXC_EXPORT uint64_t zxc_mi355x_decompress_takev_device_scratch_size(uint32_t n_iov, uint64_t max_piece, uint32_t block_size);
ZXC_EXPORT int zxc_mi355x_decompress_takev_device(zxc_dev_dtake_t* ds, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total,
                                                  void* d_scratch, uint64_t scratch_size, void* stream);

#ifdef __cplusplus
}
#endif
#endif
