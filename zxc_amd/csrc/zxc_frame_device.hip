// zxc_frame_device.hip — zxc_mi355x_compress_device: a whole v8 archive from device memory to device memory.
//
// zxc_compress (zxc_host.c) writes the container on the host around the device encoder; this file writes the same bytes on the
// device, so that data already in HBM never crosses the link uncompressed. The stream order of one call:
//
//   stage    the last block or two (those whose encoder over-read would pass src_size) -> work area, zero padded
//   encode   blocks [0, k) straight from d_src, blocks [k, nb) from the staged copy (zxc_mi355x_encode_blocks_device x 2)
//   tiles    per tile of ZC_TILE_BLOCKS blocks: sum of the sizes, size check, part of the global hash
//   finish   one workgroup: tile offsets, archive size, capacity check, status word, header / EOF / SEK header / footer
//   scatter  per tile: block offsets and seek-table entries            (only when the status word says the archive fits)
//   gather   one wave per block: slot -> archive, 16-byte loads/stores (idem)
//   result   *d_result = archive size or the error, written once, after everything above
//
// No workgroup waits for another: every dependency is the stream order between launches.
//
// zxc_mi355x_compress_dict_device is the same call with a dictionary in device memory. Two stages differ: the blocks are encoded
// from [dict | block] images (zxc_mi355x_encode_blocks_dict_device), in chunks that reuse one image area in stream order, and
// nothing is staged, because an image's padding serves the encoder's over-read; and the finish pass makes the file header's words
// (zc_file_header_words) itself, because the dictionary's id is a word in device memory.
#include "zxc_device_util.h"  // the tile passes, the copy, the host-side plumbing; zxc_container.h: the container's constants and check bytes

#define FRAME_ENC_OVERREAD 32u      // the encoder reads up to 32 bytes past its input (include/zxc_mi355x.h)
#define FRAME_STAGE_PAD 64u         // zero bytes behind the staged blocks (covers the over-read)
#define FRAME_IMAGE_PAD ZC_IMAGE_PAD  // behind the last image; the chunk constants are zxc_container.h's, shared with zxc_cbatch.h

// Per-call state at the start of the work area (one call owns it from the first launch to the last).
struct FrameCtl {
    int64_t status;    // archive size, or a negative zxc_error_t (finish pass)
    uint64_t seek_at;  // byte offset of the first seek-table entry in d_dst
};

// ---------------------------------------------------------------- kernels
// stage[0, n) = src[0, n), stage[n, n + FRAME_STAGE_PAD) = 0. Reads exactly src[0, n).
extern "C" __global__ void __launch_bounds__(256)
zxc_frame_stage_kernel(const uint8_t* __restrict__ src, uint32_t n, uint8_t* __restrict__ stage) {
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n + FRAME_STAGE_PAD; i += step) stage[i] = i < n ? src[i] : 0u;
}

// Tile t covers blocks [t * ZC_TILE_BLOCKS, ...), ZD_PER_THREAD consecutive blocks per thread. Writes the tile's sum of sizes,
// whether a size lies outside [8 (+4), block_size + 64] (the check of comp_sink, zxc_host.c), and the tile's part of the global hash:
// h = rotl(h, 1) ^ t_i folded from 0 over all nb trailers equals XOR_i rotl(t_i, (nb - 1 - i) mod 32).
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_frame_tiles_kernel(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes, uint32_t nb,
                       uint32_t block_size, uint32_t checksum, uint64_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_hash,
                       uint32_t* __restrict__ tile_bad) {
    const uint32_t t = threadIdx.x;
    const uint32_t min_size = 8u + (checksum ? 4u : 0u), max_size = block_size + 64u;
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + t * ZD_PER_THREAD;
    uint32_t sum = 0, hash = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        const uint32_t sz = sizes[b];
        if (sz < min_size || sz > max_size) {  // never used as a length or to find the trailer
            bad = 1u;
            continue;
        }
        sum += sz;
        if (checksum) hash ^= zc_rotl(zc_rd32(slots + (uint64_t)b * slot_stride + sz - 4u), (nb - 1u - b) & 31u);
    }
    const zd_totals tile = zd_tile_reduce(sum, hash, bad);
    if (t == 0) {
        tile_sum[blockIdx.x] = tile.sum;
        tile_hash[blockIdx.x] = tile.hash;
        tile_bad[blockIdx.x] = tile.bad;
    }
}

// One workgroup. tile_sum[t] becomes the archive offset of tile t's first block (exclusive prefix + ZC_FILE_HDR, in place); then the
// archive size is checked against the capacity and, when it fits, the header, the EOF block, the SEK header and the footer are written.
// hdr_lo / hdr_hi, eof and sek are the little-endian images of those 16 + 8 + 8 bytes, made on the host (they depend on options only).
// dict_id != NULL (the dictionary call): the header carries *dict_id, so its words are made here, from lg and the checksum flag.
extern "C" __global__ void __launch_bounds__(256)
zxc_frame_finish_kernel(uint64_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_hash, const uint32_t* __restrict__ tile_bad,
                        uint32_t n_tiles, uint32_t nb, uint64_t src_size, uint8_t* __restrict__ dst, uint64_t dst_capacity,
                        uint64_t hdr_lo, uint64_t hdr_hi, uint64_t eof, uint64_t sek, uint32_t seekable, uint32_t checksum,
                        FrameCtl* __restrict__ ctl, uint32_t lg, const uint32_t* __restrict__ dict_id) {
    const zd_totals all = zd_scan_tiles(
        n_tiles, ZC_FILE_HDR,
        [=](uint32_t i, uint32_t& hash, uint32_t& bad) { const uint64_t s = tile_sum[i]; hash ^= tile_hash[i]; bad |= tile_bad[i]; return s; },
        [=](uint32_t i, uint64_t off) { tile_sum[i] = off; });
    if (threadIdx.x != 0) return;

    const uint64_t eof_at = ZC_FILE_HDR + all.sum;
    const uint64_t seek_bytes = (seekable && nb) ? ZC_BLK_HDR + 4ull * nb : 0ull;
    const uint64_t size = eof_at + ZC_BLK_HDR + seek_bytes + ZC_FOOTER;
    const int64_t status = all.bad ? (int64_t)ZXC_ERROR_CORRUPT_DATA : size > dst_capacity ? (int64_t)ZXC_ERROR_DST_TOO_SMALL : (int64_t)size;
    ctl->status = status;
    ctl->seek_at = eof_at + 2u * ZC_BLK_HDR;
    if (status < 0) return;
    if (dict_id) zc_file_header_words(lg, (int)checksum, 1, *dict_id, &hdr_lo, &hdr_hi);
    zc_st_le(dst, hdr_lo, 8);
    zc_st_le(dst + 8, hdr_hi, 8);
    zc_st_le(dst + eof_at, eof, 8);
    if (seek_bytes) zc_st_le(dst + eof_at + ZC_BLK_HDR, sek, 8);
    uint8_t* foot = dst + size - ZC_FOOTER;
    zc_put_footer(foot, src_size, checksum ? all.hash : 0u);
}

// Per tile: offsets[b] = archive offset of block b; with a seek table also its entry (the block's size, 4 bytes LE).
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_frame_scatter_kernel(const uint32_t* __restrict__ sizes, uint32_t nb, const uint64_t* __restrict__ tile_off,
                         uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t seekable, const FrameCtl* __restrict__ ctl) {
    if (ctl->status < 0) return;
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint32_t sz[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        sz[j] = b0 + j < nb ? sizes[b0 + j] : 0u;
        sum += sz[j];
    }
    uint64_t run = zd_tile_offset(sum, tile_off[blockIdx.x]);
    uint8_t* seek = dst + ctl->seek_at;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        offsets[b] = run;
        run += sz[j];
        if (seekable) zc_st_le(seek + 4ull * b, sz[j], 4);
    }
}

// Compaction, one wave per block: block b's sizes[b] bytes at its slot -> dst + offsets[b]. Sizes were checked by the tiles pass
// (status >= 0 only when every one lies in [8, block_size + 64]); nothing is written at or past offsets[b] + sizes[b].
extern "C" __global__ void __launch_bounds__(256)
zxc_frame_gather_kernel(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes,
                        const uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t nb, const FrameCtl* __restrict__ ctl) {
    if (ctl->status < 0) return;
    zd_gather_blocks(slots, slot_stride, sizes, offsets, dst, nb);
}

extern "C" __global__ void zxc_frame_result_kernel(const FrameCtl* __restrict__ ctl, int64_t* __restrict__ result) {
    if (threadIdx.x == 0) *result = ctl->status;
}

// ---------------------------------------------------------------- host side
namespace {

struct FramePlan {
    uint32_t block_size, lg, level, checksum, seekable, nb, n_tiles, k_direct, stride;
    uint64_t staged;  // source bytes of the staged blocks [k_direct, nb)
    // work-area offsets (relative to the 256-byte aligned base)
    uint64_t o_tile_sum, o_tile_hash, o_tile_bad, o_sizes, o_offsets, o_stage, o_slots, o_images, bytes;  // o_images: the dictionary call's image area, behind the rest
};

// The options (zd_compress_opts) and the call's shape. -> ZXC_OK or a negative zxc_error_t.
int frame_plan(uint64_t src_size, const zxc_compress_opts_t* opts, FramePlan* p) {
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    zd_copts_t co;
    const int orc = zd_compress_opts(opts, &co);
    if (orc != ZXC_OK) return orc;
    const uint64_t bs = co.block_size, nb = (src_size + bs - 1u) / bs;
    if (nb > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    p->block_size = co.block_size; p->level = co.level; p->checksum = co.checksum; p->seekable = co.seekable;
    p->lg = zc_block_size_lg(bs);
    p->nb = (uint32_t)nb;
    p->n_tiles = (uint32_t)((nb + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS);
    p->stride = zxc_mi355x_encode_slot_stride(p->block_size);
    // block b (not the last) reads up to (b + 1) * bs + FRAME_ENC_OVERREAD: straight from d_src while that stays inside it
    uint64_t k = src_size >= FRAME_ENC_OVERREAD ? (src_size - FRAME_ENC_OVERREAD) / bs : 0u;
    if (nb && k > nb - 1u) k = nb - 1u;
    p->k_direct = (uint32_t)k;
    p->staged = src_size - k * bs;  // < bs + FRAME_ENC_OVERREAD
    uint64_t o = zc_round_up(sizeof(FrameCtl), ZD_WORK_ALIGN);
    p->o_tile_sum = o;  o = zc_round_up(o + 8ull * p->n_tiles, ZD_WORK_ALIGN);
    p->o_tile_hash = o; o = zc_round_up(o + 4ull * p->n_tiles, ZD_WORK_ALIGN);
    p->o_tile_bad = o;  o = zc_round_up(o + 4ull * p->n_tiles, ZD_WORK_ALIGN);
    p->o_sizes = o;     o = zc_round_up(o + 4ull * nb, ZD_WORK_ALIGN);
    p->o_offsets = o;   o = zc_round_up(o + 8ull * nb, ZD_WORK_ALIGN);
    p->o_stage = o;     o = zc_round_up(o + (nb ? bs + FRAME_ENC_OVERREAD + FRAME_STAGE_PAD : 0u), ZD_WORK_ALIGN);
    p->o_slots = o;     o = zc_round_up(o + nb * p->stride, ZD_WORK_ALIGN);
    p->o_images = o;
    p->bytes = o + ZD_WORK_ALIGN;  // (the caller's d_work may have any alignment)
    return ZXC_OK;
}

// What the archive needs whatever the encoder writes: header, the smallest block per block, EOF, seek table, footer.
uint64_t frame_known_size(const FramePlan& p) { return zc_known_size(p.nb, (int)p.checksum, (int)p.seekable); }

// The dictionary path's image area: blocks per chunk, and the area's bytes, added to p.bytes of the plain plan (0 blocks: none).
uint64_t frame_chunk_blocks(const FramePlan& p, uint32_t dict_size) {
    return zc_image_chunk(p.block_size, dict_size);
}
uint64_t frame_image_bytes(const FramePlan& p, uint32_t dict_size) {
    if (!p.nb) return 0u;
    const uint64_t c = frame_chunk_blocks(p, dict_size), n = p.nb < c ? p.nb : c;
    return zc_round_up(n * ((uint64_t)p.block_size + dict_size) + FRAME_IMAGE_PAD, ZD_WORK_ALIGN);
}

// Both calls behind their argument checks. dict == NULL: the plain call.
int frame_enqueue(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, const FramePlan& p, const zxc_dev_dict_t* dict,
                  void* d_work, int64_t* d_result, void* stream) {
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    uint8_t* base = zd_work_base(d_work);
    FrameCtl* ctl = (FrameCtl*)base;
    uint64_t* tile_sum = (uint64_t*)(base + p.o_tile_sum);
    uint32_t* tile_hash = (uint32_t*)(base + p.o_tile_hash);
    uint32_t* tile_bad = (uint32_t*)(base + p.o_tile_bad);
    uint32_t* sizes = (uint32_t*)(base + p.o_sizes);
    uint64_t* offsets = (uint64_t*)(base + p.o_offsets);
    uint8_t* stage = base + p.o_stage;
    uint8_t* slots = base + p.o_slots;
    uint8_t* images = base + p.o_images;  // (dictionary call only: its work size adds frame_image_bytes() behind the plain plan)
    uint8_t* dst = (uint8_t*)d_dst;

    if (p.nb && dict) {
        // Blocks are independent, so chunk by chunk gives the bytes of one launch over all of them. A chunk's images are built and
        // consumed in stream order before the next chunk overwrites them. zxc_prepend_dict_kernel reads exactly the source's bytes.
        const uint64_t chunk = frame_chunk_blocks(p, dict->size);
        for (uint64_t b0 = 0; b0 < p.nb; b0 += chunk) {
            const uint64_t n = p.nb - b0 < chunk ? p.nb - b0 : chunk, at = b0 * p.block_size;
            const uint64_t bytes = src_size - at < n * p.block_size ? src_size - at : n * p.block_size;
            const int rc = zxc_mi355x_encode_blocks_dict_device((const uint8_t*)d_src + at, bytes, p.block_size, (int)p.level, (int)p.checksum,
                                                                dict->d_content, dict->size, images, slots + b0 * p.stride, sizes + b0, stream);
            if (rc != ZXC_OK) return rc;
        }
    } else if (p.nb) {
        const uint64_t direct = (uint64_t)p.k_direct * p.block_size;
        hipLaunchKernelGGL(zxc_frame_stage_kernel, dim3((unsigned)((p.staged + FRAME_STAGE_PAD + 4095u) / 4096u)), dim3(256), 0, st,
                           (const uint8_t*)d_src + direct, (uint32_t)p.staged, stage);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
        int rc = ZXC_OK;
        if (p.k_direct)
            rc = zxc_mi355x_encode_blocks_device(d_src, direct, p.block_size, (int)p.level, (int)p.checksum, slots, sizes, stream);
        if (rc == ZXC_OK)
            rc = zxc_mi355x_encode_blocks_device(stage, p.staged, p.block_size, (int)p.level, (int)p.checksum,
                                                 slots + (uint64_t)p.k_direct * p.stride, sizes + p.k_direct, stream);
        if (rc != ZXC_OK) return rc;
    }
    if (p.nb) {
        hipLaunchKernelGGL(zxc_frame_tiles_kernel, dim3(p.n_tiles), dim3(ZD_TILE_THREADS), 0, st, (const uint8_t*)slots, p.stride,
                           (const uint32_t*)sizes, p.nb, p.block_size, p.checksum, tile_sum, tile_hash, tile_bad);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    // the little-endian words of the file header (with a dictionary the finish pass makes them, around the id), of the EOF block
    // and of the SEK header
    uint64_t hdr_lo = 0, hdr_hi = 0;
    if (!dict) zc_file_header_words(p.lg, (int)p.checksum, 0, 0u, &hdr_lo, &hdr_hi);
    hipLaunchKernelGGL(zxc_frame_finish_kernel, dim3(1), dim3(256), 0, st, tile_sum, (const uint32_t*)tile_hash, (const uint32_t*)tile_bad,
                       p.n_tiles, p.nb, src_size, dst, dst_capacity, hdr_lo, hdr_hi, zc_blk_hdr(ZC_BLK_EOF, 0u), zc_blk_hdr(ZC_BLK_SEK, p.nb * 4u), p.seekable, p.checksum, ctl,
                       p.lg, zd_dict_of(dict).id);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    if (p.nb) {
        hipLaunchKernelGGL(zxc_frame_scatter_kernel, dim3(p.n_tiles), dim3(ZD_TILE_THREADS), 0, st, (const uint32_t*)sizes, p.nb,
                           (const uint64_t*)tile_sum, offsets, dst, p.seekable, (const FrameCtl*)ctl);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
        const uint32_t groups = (p.nb + 3u) / 4u < 65536u ? (p.nb + 3u) / 4u : 65536u;
        hipLaunchKernelGGL(zxc_frame_gather_kernel, dim3(groups), dim3(256), 0, st, (const uint8_t*)slots, p.stride, (const uint32_t*)sizes,
                           (const uint64_t*)offsets, dst, p.nb, (const FrameCtl*)ctl);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    hipLaunchKernelGGL(zxc_frame_result_kernel, dim3(1), dim3(64), 0, st, (const FrameCtl*)ctl, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_compress_device_work_size(uint64_t src_size, const zxc_compress_opts_t* opts) {
    FramePlan p;
    return frame_plan(src_size, opts, &p) == ZXC_OK ? p.bytes : 0u;
}

int zxc_mi355x_compress_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity,
                               const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if (!d_dst || !d_result || !d_work || (src_size > 0 && !d_src)) return ZXC_ERROR_NULL_INPUT;
    FramePlan p;
    const int prc = frame_plan(src_size, opts, &p);
    if (prc != ZXC_OK) return prc;
    if (work_size < p.bytes) return ZXC_ERROR_MEMORY;
    if (dst_capacity < frame_known_size(p)) return ZXC_ERROR_DST_TOO_SMALL;
    return frame_enqueue(d_src, src_size, d_dst, dst_capacity, p, NULL, d_work, d_result, stream);
}

uint64_t zxc_mi355x_compress_dict_device_work_size(uint64_t src_size, const zxc_compress_opts_t* opts, uint32_t dict_size) {
    FramePlan p;
    if (frame_plan(src_size, opts, &p) != ZXC_OK || dict_size > ZC_DICT_MAX) return 0u;
    return p.bytes + (dict_size ? frame_image_bytes(p, dict_size) : 0u);
}

int zxc_mi355x_compress_dict_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, const zxc_compress_opts_t* opts,
                                    const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if (!d_dst || !d_result || !d_work || (src_size > 0 && !d_src)) return ZXC_ERROR_NULL_INPUT;
    FramePlan p;
    const int prc = frame_plan(src_size, opts, &p);
    if (prc != ZXC_OK) return prc;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if (work_size < p.bytes + (dict ? frame_image_bytes(p, dict->size) : 0u)) return ZXC_ERROR_MEMORY;
    if (dst_capacity < frame_known_size(p)) return ZXC_ERROR_DST_TOO_SMALL;
    return frame_enqueue(d_src, src_size, d_dst, dst_capacity, p, dict, d_work, d_result, stream);
}

}  // extern "C"
