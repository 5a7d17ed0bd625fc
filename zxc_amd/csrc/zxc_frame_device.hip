// zxc_frame_device.hip — zxc_mi355x_compress_device: a whole v8 archive from device memory to device memory.
//
// zxc_compress (zxc_host.c) writes the container on the host around the device encoder; this file writes the same bytes on the
// device, so that data already in HBM never crosses the link uncompressed. The stream order of one call:
//
//   stage    the last block or two (those whose encoder over-read would pass src_size) -> work area, zero padded
//   encode   blocks [0, k) straight from d_src, blocks [k, nb) from the staged copy (zxc_mi355x_encode_blocks_device x 2)
//   tiles    per tile of FRAME_TILE_BLOCKS blocks: sum of the sizes, size check, part of the global hash
//   finish   one workgroup: tile offsets, archive size, capacity check, status word, header / EOF / SEK header / footer
//   scatter  per tile: block offsets and seek-table entries            (only when the status word says the archive fits)
//   gather   one wave per block: slot -> archive, 16-byte loads/stores (idem)
//   result   *d_result = archive size or the error, written once, after everything above
//
// No workgroup waits for another: every dependency is the stream order between launches.
//
// zxc_mi355x_compress_dict_device is the same call with a dictionary in device memory. Two stages differ: the blocks are encoded
// from [dict | block] images (zxc_mi355x_encode_blocks_dict_device), in chunks that reuse one image area in stream order, and
// nothing is staged, because an image's padding serves the encoder's over-read; and the finish pass assembles bytes 6..15 of the
// file header (dictionary flag, id, check bytes) itself, because the id is a word in device memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zxc_container.h"  // zc_hdr_hash16 on the device (and zxc_error.h, zxc_mi355x.h)

#define FRAME_MAGIC 0x9CB02EF5u
#define FRAME_VERSION 8u
#define FRAME_HDR 16u               // file header
#define FRAME_BLK_HDR 8u            // block header (EOF block, SEK header)
#define FRAME_FOOTER 12u            // source size + global hash
#define FRAME_ENC_OVERREAD 32u      // the encoder reads up to 32 bytes past its input (include/zxc_mi355x.h)
#define FRAME_STAGE_PAD 64u         // zero bytes behind the staged blocks (covers the over-read)
#define FRAME_TILE_THREADS 256u
#define FRAME_PER_THREAD 4u
#define FRAME_TILE_BLOCKS (FRAME_TILE_THREADS * FRAME_PER_THREAD)
#define FRAME_ALIGN 256u
#define FRAME_DICT_MAX 65535u
#define FRAME_IMAGE_BYTES (256ull << 20)  // the image area of a chunk of the dictionary path stays near this ...
#define FRAME_IMAGE_MIN_BLOCKS 4096u      // ... but a chunk is never fewer blocks than this
#define FRAME_IMAGE_PAD 64u               // behind the last image (the encoder's over-read, as zxc_mi355x_encode_dict_work_size)

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- header check bytes (zxc_host.c: hdr_hash8 / hdr_hash16)
static uint64_t fr_rd64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; i--) v = (v << 8) | p[i];
    return v;
}
static uint64_t fr_xs_mix(uint64_t h) {
    h ^= h << 13;
    h ^= h >> 7;
    h ^= h << 17;
    return h;
}
static uint8_t fr_hdr_hash8(const uint8_t* p) {
    const uint64_t h = fr_xs_mix(fr_rd64(p) ^ 0x9E3779B97F4A7C15ull);
    return (uint8_t)((h >> 32) ^ h);
}
static uint16_t fr_hdr_hash16(const uint8_t* p) {
    const uint64_t h = fr_xs_mix(fr_rd64(p) ^ fr_rd64(p + 8) ^ 0xD2D84A61D2D84A61ull);
    const uint32_t r = (uint32_t)((h >> 32) ^ h);
    return (uint16_t)((r >> 16) ^ r);
}

// ---------------------------------------------------------------- device helpers
// wave-wide inclusive prefix sum on the DPP crossbar (the same controls as wave_scan_add / e_scan_add of the kernel sources)
__device__ __forceinline__ uint32_t fr_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return v;
}
__device__ __forceinline__ uint32_t fr_wave_xor(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t fr_rotl(uint32_t x, uint32_t r) { return r ? (x << r) | (x >> (32u - r)) : x; }
__device__ __forceinline__ uint32_t fr_ld32u(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void fr_st_le(uint8_t* p, uint64_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8u * i));
}

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

// Tile t covers blocks [t * FRAME_TILE_BLOCKS, ...), FRAME_PER_THREAD consecutive blocks per thread. Writes the tile's sum of sizes,
// whether a size lies outside [8 (+4), block_size + 64] (the check of comp_sink, zxc_host.c), and the tile's part of the global hash:
// h = rotl(h, 1) ^ t_i folded from 0 over all nb trailers equals XOR_i rotl(t_i, (nb - 1 - i) mod 32).
extern "C" __global__ void __launch_bounds__(FRAME_TILE_THREADS)
zxc_frame_tiles_kernel(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes, uint32_t nb,
                       uint32_t block_size, uint32_t checksum, uint64_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_hash,
                       uint32_t* __restrict__ tile_bad) {
    __shared__ uint32_t w_sum[FRAME_TILE_THREADS / 64u], w_hash[FRAME_TILE_THREADS / 64u], w_bad[FRAME_TILE_THREADS / 64u];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t min_size = 8u + (checksum ? 4u : 0u), max_size = block_size + 64u;
    const uint32_t b0 = blockIdx.x * FRAME_TILE_BLOCKS + t * FRAME_PER_THREAD;
    uint32_t sum = 0, hash = 0, bad = 0;
#pragma unroll
    for (uint32_t j = 0; j < FRAME_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        const uint32_t sz = sizes[b];
        if (sz < min_size || sz > max_size) {  // never used as a length or to find the trailer
            bad = 1u;
            continue;
        }
        sum += sz;
        if (checksum) hash ^= fr_rotl(fr_ld32u(slots + (uint64_t)b * slot_stride + sz - 4u), (nb - 1u - b) & 31u);
    }
    // (a thread's sum is < 4 x (2 MiB + 65), a wave's < 2^30: 32 bits hold both)
    sum = (uint32_t)__builtin_amdgcn_readlane((int)fr_scan_add(sum), 63);
    hash = fr_wave_xor(hash);
    bad = __any(bad) ? 1u : 0u;
    if (lane == 0) { w_sum[wave] = sum; w_hash[wave] = hash; w_bad[wave] = bad; }
    __syncthreads();
    if (t == 0) {
        uint64_t s = 0;
        uint32_t h = 0, d = 0;
        for (uint32_t w = 0; w < FRAME_TILE_THREADS / 64u; w++) { s += w_sum[w]; h ^= w_hash[w]; d |= w_bad[w]; }
        tile_sum[blockIdx.x] = s;
        tile_hash[blockIdx.x] = h;
        tile_bad[blockIdx.x] = d;
    }
}

// One workgroup. tile_sum[t] becomes the archive offset of tile t's first block (exclusive prefix + FRAME_HDR, in place); then the
// archive size is checked against the capacity and, when it fits, the header, the EOF block, the SEK header and the footer are written.
// hdr_lo / hdr_hi, eof and sek are the little-endian images of those 16 + 8 + 8 bytes, made on the host (they depend on options only).
// dict_id != NULL (the dictionary call): the header gets the dictionary flag and *dict_id in bytes 7..10, and its check bytes are
// computed here over that (zxc_compress: zxc_host.c, "HAS_DICTIONARY + dict_id").
extern "C" __global__ void __launch_bounds__(256)
zxc_frame_finish_kernel(uint64_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_hash, const uint32_t* __restrict__ tile_bad,
                        uint32_t n_tiles, uint32_t nb, uint64_t src_size, uint8_t* __restrict__ dst, uint64_t dst_capacity,
                        uint64_t hdr_lo, uint64_t hdr_hi, uint64_t eof, uint64_t sek, uint32_t seekable, uint32_t checksum,
                        FrameCtl* __restrict__ ctl, const uint32_t* __restrict__ dict_id) {
    __shared__ uint64_t w_tot[4];
    __shared__ uint32_t w_hash[4], w_bad[4];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    // thread t owns tiles [t * per, (t + 1) * per): a serial sum, a workgroup scan of the 256 sums, a serial write-back
    const uint32_t per = (n_tiles + 255u) / 256u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t mine = 0;
    uint32_t hash = 0, bad = 0;
    for (uint32_t i = lo; i < hi; i++) { mine += tile_sum[i]; hash ^= tile_hash[i]; bad |= tile_bad[i]; }
    uint64_t incl = mine;  // wave inclusive scan, 64-bit (a tile sum can pass 2^31)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(incl, (unsigned)d);
        if ((int)lane >= d) incl += o;
    }
    hash = fr_wave_xor(hash);
    bad = __any(bad) ? 1u : 0u;
    if (lane == 63) w_tot[wave] = incl;
    if (lane == 0) { w_hash[wave] = hash; w_bad[wave] = bad; }
    __syncthreads();
    uint64_t base = FRAME_HDR, total = 0;
    uint32_t ghash = 0, gbad = 0;
    for (uint32_t w = 0; w < 4u; w++) {
        if (w < wave) base += w_tot[w];
        total += w_tot[w];
        ghash ^= w_hash[w];
        gbad |= w_bad[w];
    }
    uint64_t run = base + incl - mine;
    for (uint32_t i = lo; i < hi; i++) { const uint64_t s = tile_sum[i]; tile_sum[i] = run; run += s; }
    if (t != 0) return;

    const uint64_t eof_at = FRAME_HDR + total;
    const uint64_t seek_bytes = (seekable && nb) ? FRAME_BLK_HDR + 4ull * nb : 0ull;
    const uint64_t size = eof_at + FRAME_BLK_HDR + seek_bytes + FRAME_FOOTER;
    const int64_t status = gbad ? (int64_t)ZXC_ERROR_CORRUPT_DATA : size > dst_capacity ? (int64_t)ZXC_ERROR_DST_TOO_SMALL : (int64_t)size;
    ctl->status = status;
    ctl->seek_at = eof_at + 2u * FRAME_BLK_HDR;
    if (status < 0) return;
    if (dict_id) {  // bytes 6..15: flags | 0x40, the id in 7..10, zeros, the 16-bit check over the rest
        const uint64_t id = *dict_id;
        hdr_lo = (hdr_lo & 0x0000FFFFFFFFFFFFull) | (((hdr_lo >> 48) & 0xFFu) | 0x40u) << 48 | (id & 0xFFu) << 56;
        hdr_hi = id >> 8;
        hdr_hi |= (uint64_t)zc_hdr_hash16(hdr_lo, hdr_hi) << 48;
    }
    fr_st_le(dst, hdr_lo, 8);
    fr_st_le(dst + 8, hdr_hi, 8);
    fr_st_le(dst + eof_at, eof, 8);
    if (seek_bytes) fr_st_le(dst + eof_at + FRAME_BLK_HDR, sek, 8);
    uint8_t* foot = dst + size - FRAME_FOOTER;
    fr_st_le(foot, src_size, 8);
    fr_st_le(foot + 8, checksum ? ghash : 0u, 4);
}

// Per tile: offsets[b] = archive offset of block b; with a seek table also its entry (the block's size, 4 bytes LE).
extern "C" __global__ void __launch_bounds__(FRAME_TILE_THREADS)
zxc_frame_scatter_kernel(const uint32_t* __restrict__ sizes, uint32_t nb, const uint64_t* __restrict__ tile_off,
                         uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t seekable, const FrameCtl* __restrict__ ctl) {
    __shared__ uint32_t w_sum[FRAME_TILE_THREADS / 64u];
    if (ctl->status < 0) return;
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t b0 = blockIdx.x * FRAME_TILE_BLOCKS + t * FRAME_PER_THREAD;
    uint32_t sz[FRAME_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < FRAME_PER_THREAD; j++) {
        sz[j] = b0 + j < nb ? sizes[b0 + j] : 0u;
        sum += sz[j];
    }
    const uint32_t incl = fr_scan_add(sum);
    if (lane == 63) w_sum[wave] = incl;
    __syncthreads();
    uint64_t run = tile_off[blockIdx.x] + incl - sum;
    for (uint32_t w = 0; w < wave; w++) run += w_sum[w];
    uint8_t* seek = dst + ctl->seek_at;
#pragma unroll
    for (uint32_t j = 0; j < FRAME_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb) break;
        offsets[b] = run;
        run += sz[j];
        if (seekable) fr_st_le(seek + 4ull * b, sz[j], 4);
    }
}

// Compaction, one wave per block: block b's sizes[b] bytes at its slot -> dst + offsets[b]. Sizes were checked by the tiles pass
// (status >= 0 only when every one lies in [8, block_size + 64]); nothing is written at or past offsets[b] + sizes[b].
extern "C" __global__ void __launch_bounds__(256)
zxc_frame_gather_kernel(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes,
                        const uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t nb, const FrameCtl* __restrict__ ctl) {
    if (ctl->status < 0) return;
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    for (uint64_t b = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); b < nb; b += (uint64_t)gridDim.x * waves) {
        const uint8_t* s = slots + b * slot_stride;
        uint8_t* d = dst + offsets[b];
        const uint32_t n = sizes[b];
        for (uint32_t o = 16u * lane; o < n; o += 1024u) {
            if (o + 16u <= n) {
                v4u v;
                __builtin_memcpy(&v, s + o, 16);
                __builtin_memcpy(d + o, &v, 16);
            } else {
                for (uint32_t k = o; k < n; k++) d[k] = s[k];
            }
        }
    }
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

uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1u) / a * a; }

// Options as zxc_compress reads them (zxc_host.c). -> ZXC_OK or a negative zxc_error_t.
int frame_plan(uint64_t src_size, const zxc_compress_opts_t* opts, FramePlan* p) {
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    int level = (opts && opts->level > 0) ? opts->level : 3;
    if (level > 7) level = 7;
    const uint64_t bs = (opts && opts->block_size > 0) ? (uint64_t)opts->block_size : 512u * 1024u;
    if (bs < (1u << 12) || bs > (1u << 21) || (bs & (bs - 1u))) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t nb = (src_size + bs - 1u) / bs;
    if (nb > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    p->block_size = (uint32_t)bs;
    p->lg = 0;
    while ((1ull << p->lg) < bs) p->lg++;
    p->level = (uint32_t)level;
    p->checksum = (opts && opts->checksum_enabled) ? 1u : 0u;
    p->seekable = (opts && opts->seekable) ? 1u : 0u;
    p->nb = (uint32_t)nb;
    p->n_tiles = (uint32_t)((nb + FRAME_TILE_BLOCKS - 1u) / FRAME_TILE_BLOCKS);
    p->stride = zxc_mi355x_encode_slot_stride(p->block_size);
    // block b (not the last) reads up to (b + 1) * bs + FRAME_ENC_OVERREAD: straight from d_src while that stays inside it
    uint64_t k = src_size >= FRAME_ENC_OVERREAD ? (src_size - FRAME_ENC_OVERREAD) / bs : 0u;
    if (nb && k > nb - 1u) k = nb - 1u;
    p->k_direct = (uint32_t)k;
    p->staged = src_size - k * bs;  // < bs + FRAME_ENC_OVERREAD
    uint64_t o = round_up(sizeof(FrameCtl), FRAME_ALIGN);
    p->o_tile_sum = o;  o = round_up(o + 8ull * p->n_tiles, FRAME_ALIGN);
    p->o_tile_hash = o; o = round_up(o + 4ull * p->n_tiles, FRAME_ALIGN);
    p->o_tile_bad = o;  o = round_up(o + 4ull * p->n_tiles, FRAME_ALIGN);
    p->o_sizes = o;     o = round_up(o + 4ull * nb, FRAME_ALIGN);
    p->o_offsets = o;   o = round_up(o + 8ull * nb, FRAME_ALIGN);
    p->o_stage = o;     o = round_up(o + (nb ? bs + FRAME_ENC_OVERREAD + FRAME_STAGE_PAD : 0u), FRAME_ALIGN);
    p->o_slots = o;     o = round_up(o + nb * p->stride, FRAME_ALIGN);
    p->o_images = o;
    p->bytes = o + FRAME_ALIGN;  // (the caller's d_work may have any alignment)
    return ZXC_OK;
}

// What the archive needs whatever the encoder writes: header, the smallest block per block, EOF, seek table, footer.
uint64_t frame_known_size(const FramePlan& p) {
    return FRAME_HDR + (uint64_t)p.nb * (8u + 4u * p.checksum) + FRAME_BLK_HDR +
           ((p.seekable && p.nb) ? FRAME_BLK_HDR + 4ull * p.nb : 0u) + FRAME_FOOTER;
}

bool launched() { return hipGetLastError() == hipSuccess; }

// The dictionary path's image area: blocks per chunk, and the area's bytes, added to p.bytes of the plain plan (0 blocks: none).
uint64_t frame_chunk_blocks(const FramePlan& p, uint32_t dict_size) {
    const uint64_t c = FRAME_IMAGE_BYTES / ((uint64_t)p.block_size + dict_size);
    return c > FRAME_IMAGE_MIN_BLOCKS ? c : FRAME_IMAGE_MIN_BLOCKS;
}
uint64_t frame_image_bytes(const FramePlan& p, uint32_t dict_size) {
    if (!p.nb) return 0u;
    const uint64_t c = frame_chunk_blocks(p, dict_size), n = p.nb < c ? p.nb : c;
    return round_up(n * ((uint64_t)p.block_size + dict_size) + FRAME_IMAGE_PAD, FRAME_ALIGN);
}

// Both calls behind their argument checks. dict == NULL: the plain call.
int frame_enqueue(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, const FramePlan& p, const zxc_dev_dict_t* dict,
                  void* d_work, int64_t* d_result, void* stream) {
    int n_dev = 0, dev = -1;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || hipGetDevice(&dev) != hipSuccess || dev < 0)
        return ZXC_ERROR_GPU_UNAVAILABLE;

    const hipStream_t st = (hipStream_t)stream;
    uint8_t* base = (uint8_t*)round_up((uint64_t)(uintptr_t)d_work, FRAME_ALIGN);
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
        hipLaunchKernelGGL(zxc_frame_tiles_kernel, dim3(p.n_tiles), dim3(FRAME_TILE_THREADS), 0, st, (const uint8_t*)slots, p.stride,
                           (const uint32_t*)sizes, p.nb, p.block_size, p.checksum, tile_sum, tile_hash, tile_bad);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    uint8_t hdr[FRAME_HDR] = {0}, eof[FRAME_BLK_HDR] = {0}, sek[FRAME_BLK_HDR] = {0};
    hdr[0] = (uint8_t)FRAME_MAGIC; hdr[1] = (uint8_t)(FRAME_MAGIC >> 8); hdr[2] = (uint8_t)(FRAME_MAGIC >> 16); hdr[3] = (uint8_t)(FRAME_MAGIC >> 24);
    hdr[4] = FRAME_VERSION;
    hdr[5] = (uint8_t)p.lg;
    hdr[6] = p.checksum ? 0x80u : 0u;
    if (!dict) {  // (with a dictionary the finish pass completes bytes 6..15)
        const uint16_t h16 = fr_hdr_hash16(hdr);
        hdr[14] = (uint8_t)h16;
        hdr[15] = (uint8_t)(h16 >> 8);
    }
    eof[0] = 255u;  // BLK_EOF
    eof[7] = fr_hdr_hash8(eof);
    const uint32_t sek_len = p.nb * 4u;
    sek[0] = 254u;  // BLK_SEK
    sek[3] = (uint8_t)sek_len; sek[4] = (uint8_t)(sek_len >> 8); sek[5] = (uint8_t)(sek_len >> 16); sek[6] = (uint8_t)(sek_len >> 24);
    sek[7] = fr_hdr_hash8(sek);
    hipLaunchKernelGGL(zxc_frame_finish_kernel, dim3(1), dim3(256), 0, st, tile_sum, (const uint32_t*)tile_hash, (const uint32_t*)tile_bad,
                       p.n_tiles, p.nb, src_size, dst, dst_capacity, fr_rd64(hdr), fr_rd64(hdr + 8), fr_rd64(eof), fr_rd64(sek), p.seekable, p.checksum, ctl,
                       dict ? dict->d_id : (const uint32_t*)NULL);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    if (p.nb) {
        hipLaunchKernelGGL(zxc_frame_scatter_kernel, dim3(p.n_tiles), dim3(FRAME_TILE_THREADS), 0, st, (const uint32_t*)sizes, p.nb,
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
    if (frame_plan(src_size, opts, &p) != ZXC_OK || dict_size > FRAME_DICT_MAX) return 0u;
    return p.bytes + (dict_size ? frame_image_bytes(p, dict_size) : 0u);
}

int zxc_mi355x_compress_dict_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_capacity, const zxc_compress_opts_t* opts,
                                    const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if (!d_dst || !d_result || !d_work || (src_size > 0 && !d_src)) return ZXC_ERROR_NULL_INPUT;
    FramePlan p;
    const int prc = frame_plan(src_size, opts, &p);
    if (prc != ZXC_OK) return prc;
    if (dict && dict->size > FRAME_DICT_MAX) return ZXC_ERROR_DICT_TOO_LARGE;
    if (dict && dict->size > 0 && (!dict->d_content || !dict->d_id)) return ZXC_ERROR_NULL_INPUT;
    if (dict && dict->size == 0) dict = NULL;
    if (work_size < p.bytes + (dict ? frame_image_bytes(p, dict->size) : 0u)) return ZXC_ERROR_MEMORY;
    if (dst_capacity < frame_known_size(p)) return ZXC_ERROR_DST_TOO_SMALL;
    return frame_enqueue(d_src, src_size, d_dst, dst_capacity, p, dict, d_work, d_result, stream);
}

}  // extern "C"
