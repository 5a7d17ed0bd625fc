// zxc_append_device.hip — zxc_mi355x_compress_begin_device / _begin_dict_device / _append_device / _appendv_device /
// _appendv_dict_device / _end_device: one v8 archive in device memory from a source that arrives in pieces, each in device memory. The device counterpart of
// zxc_cstream_* (zxc_stream_host.c).
//
// zxc_mi355x_compress_device (zxc_frame_device.hip) wants the whole source in one buffer and a slot per block of it. Here a session
// keeps the archive's running state (offset, blocks, global hash, status) in its work area between calls, and a set of J slots
// that every piece reuses in stream order, so the work area does not grow with the source. The host knows every n, so it knows the
// carry and each piece's exact grid: the plan of a piece, its advance and the finish are the inline C of zxc_append.h and
// zxc_appendv.h, which the CPU tests run as well.
//
// One pipeline. A piece is at most max_piece bytes of one call; a longer call is a loop of pieces (ap_pieces). A piece is a front
// end, which fills the job table and launches the encoder over it, and one back half (ap_back); a piece that completes no block
// ends behind its prep. The four front ends:
//
//   plain    (append; any session's piece that completes no block)
//            prep     zxc_append_prep_kernel: head of the source -> carry area (completes the waiting block), last whole block ->
//                     stage area when its over-read would leave the source, tail -> the other carry area; zero padding behind
//                     each; the job table
//            encode   the job-table entry of the level over the piece's blocks, in archive order
//   images   (append and `end` in a session with a dictionary, zxc_mi355x_compress_begin_dict_device) a loop over chunks of at
//            most C = zc_image_chunk(block_size, dict_size) jobs, which reuse one image area in stream order:
//            images   zxc_append_images_kernel, one workgroup per job of the chunk: [dict | the job's bytes] into the image area
//                     and the job-table entry that points at it; the carried block's bytes come from the carry area and then from
//                     the head of the source, which is not copied anywhere else; in the first chunk one more workgroup copies the
//                     tail into the other carry area. Nothing is staged: an image is a copy with the next image, or ZC_IMAGE_PAD,
//                     behind it
//            encode   the job-table entry of the level over the chunk's images, into the chunk's slots and sizes
//   appendv  (a chunk of zxc_mi355x_compress_appendv_device: the source is the concatenation of a table of (base, len) entries in
//            device memory, zxc_appendv.h) once per call, in front of its chunks,
//            scan     three tile passes over the table: start offsets of the entries into the call's scratch, the table check and
//                     its verdict, which becomes the session's status unless that holds an error; then per chunk
//            prep     zxc_appendv_prep_kernel, one workgroup per job and one for the tail: head and tail gathered into the carry
//                     areas, a whole block left in place (inside one entry, over-read included) or gathered into its image in the
//                     scratch; nothing is read after a table error
//            encode   as plain's (the two share the launch, ap_encode)
//   appendv images  (a chunk of zxc_mi355x_compress_appendv_dict_device in a session with a dictionary that completes a block)
//            scan     as appendv's, into a scratch that holds no images; then per chunk the loop of `images` over at most C jobs:
//            images   zxc_appendv_images_kernel, one workgroup per job: [dict | the job's bytes] into the session's image area,
//                     the bytes gathered straight from the table's entries (the carried block: the carry area, then the head of
//                     the concatenation); in the first launch one more workgroup gathers the tail into the other carry area;
//                     nothing is read after a table error, every job is then unused
//            encode   as images'
//
// and the back half, once over the whole piece:
//   tiles    zxc_frame_tiles_kernel: per tile the sum of the sizes, the size check, the piece's part of the global hash
//   advance  one workgroup: tile offsets from the running offset; status, offset, block count and hash move on (zap_advance); not
//            run for a chunk of an appendv whose table is in error
//   scatter  per tile: block offsets, seek-table entries into the array in the work area  (only while the status is no error)
//   gather   one wave per block: slot -> archive                                           (idem)
//
// `end` is the piece above for what waits in the carry area, as the short last block (plain's or images' front end, no source); then
//   finish   file header (with a dictionary: its flag and *d_id), EOF block, SEK header, footer (zap_finish_dict)
//   seek     the entries from the work area to their unaligned place, 4 byte stores each
//   result   *d_result = archive size or the error, written once, after everything above
//
// No workgroup waits for another: every dependency is the stream order between launches.
#include <string.h>

#include "zxc_device_util.h"  // the tile passes, copy_bytes (zxc_wave.h), zxc_frame_tiles_kernel, the host-side plumbing
#include "zxc_kernels.h"      // the scan kernels of appendv, which zxc_take_device.hip launches too
#include "zxc_append.h"
#include "zxc_appendv.h"

#ifndef ZAP_IMAGE_THREADS
#define ZAP_IMAGE_THREADS 256  // threads per image of zxc_append_images_kernel (64 is the other value measured)
#endif

static_assert(sizeof(zxc_enc_job_t) + 4 + 8 == ZAP_JOB_BYTES && 8 + 4 + 4 == ZAP_TILE_BYTES, "the documented work size");
static_assert(sizeof(zap_ctl_t) <= 256, "the state's place at the start of the work area");

// hidden entry point of zxc_hip_shim.hip (the encode launch over a job table)
extern "C" int zxc_hip_encode_jobs(const void* d_base, zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level,
                                   int with_checksum, const void* d_dict, uint32_t dict_size, void* d_images, void* d_slots,
                                   uint32_t* d_sizes, void* stream);
extern "C" int zxc_hip_encode_job_images(const void* d_images, const zxc_enc_job_t* d_jobs, uint32_t n_jobs, uint32_t block_size, int level,
                                         int with_checksum, uint32_t dict_size, void* d_slots, uint32_t* d_sizes, void* stream);

// ---------------------------------------------------------------- kernels
extern "C" __global__ void zxc_append_begin_kernel(zap_ctl_t* __restrict__ ctl) {
    if (threadIdx.x == 0) zap_begin(ctl);
}

// The copies of the piece's plan, each with ZAP_PAD zero bytes behind it, and the job table: job j's src_off is the address of its
// bytes (the encode launch is given the base 0), since a piece's jobs read the source and the areas. Reads exactly the source bytes
// the plan's copies name; the areas hold block_size + ZAP_PAD bytes and no copy with its padding passes that (zap_plan_piece).
extern "C" __global__ void __launch_bounds__(256)
zxc_append_prep_kernel(const uint8_t* __restrict__ src, zap_piece_t p, uint8_t* __restrict__ carry, uint8_t* __restrict__ next,
                       uint8_t* __restrict__ stage, zxc_enc_job_t* __restrict__ jobs) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, threads = gridDim.x * blockDim.x;
    for (uint32_t c = 0; c < 3u; c++) {
        const zap_copy_t cp = p.cp[c];
        if (cp.area == ZAP_SRC) continue;
        uint8_t* d = (cp.area == ZAP_CARRY ? carry : cp.area == ZAP_NEXT ? next : stage) + cp.at;
        copy_bytes(d, src + cp.from, cp.len, t, threads);
        if (t < ZAP_PAD) d[cp.len + t] = 0u;
    }
    for (uint32_t j = t; j < p.nb; j += threads) {
        const zap_src_t s = zap_job(&p, j);
        const uint8_t* at = (s.area == ZAP_SRC ? src : s.area == ZAP_CARRY ? (const uint8_t*)carry : (const uint8_t*)stage) + s.off;
        zxc_enc_job_t job = {(uint64_t)(uintptr_t)at, s.len, 0u};
        jobs[j] = job;
    }
}

// The dictionary session's prep, for the chunk [j0, j0 + n) of the piece's jobs: workgroup w < n builds the image of job j0 + w,
// [dict | the job's bytes], at images + w x (block_size + dict_size), from the one or two places zap_job_images names (the carried
// block: the waiting bytes of the carry area, then the head of the source), and writes the job's table entry: the image's offset
// from `images`, which the encode launch is given as its base. Workgroup n, which only the piece's first chunk has (j0 == 0),
// copies the tail into the other carry area with ZAP_PAD zero bytes behind it, as prep does. Reads exactly the source bytes the
// plan names, at any alignment of source, carry and image (dict_size is odd in general); the image area holds n images and
// ZC_IMAGE_PAD bytes that are left as they are.
extern "C" __global__ void __launch_bounds__(ZAP_IMAGE_THREADS)
zxc_append_images_kernel(const uint8_t* __restrict__ src, zap_piece_t p, uint32_t j0, uint32_t n, const uint8_t* __restrict__ dict,
                         uint32_t dict_size, const uint8_t* __restrict__ carry, uint8_t* __restrict__ next,
                         uint8_t* __restrict__ images, zxc_enc_job_t* __restrict__ jobs) {
    const uint32_t w = blockIdx.x, t = threadIdx.x, threads = blockDim.x;
    if (w >= n) {
        const zap_copy_t cp = p.cp[2];
        if (w == n && j0 == 0 && cp.area == ZAP_NEXT) {
            uint8_t* d = next + cp.at;
            copy_bytes(d, src + cp.from, cp.len, t, threads);
            if (t < ZAP_PAD) d[cp.len + t] = 0u;
        }
        return;
    }
    const zap_src2_t s = zap_job_images(&p, j0 + w);
    const uint64_t at = (uint64_t)w * ((uint64_t)p.block_size + dict_size);
    uint8_t* d = images + at;
    copy_bytes(d, dict, dict_size, t, threads);
    d += dict_size;
#pragma unroll
    for (uint32_t k = 0; k < 2u; k++) {
        const zap_src_t g = s.seg[k];
        copy_bytes(d, (g.area == ZAP_CARRY ? carry : src) + g.off, g.len, t, threads);
        d += g.len;
    }
    if (t == 0) {
        zxc_enc_job_t job = {at, s.seg[0].len + s.seg[1].len, 0u};
        jobs[j0 + w] = job;
    }
}

// One workgroup. tile_sum[t] becomes the archive offset of tile t's first block (exclusive prefix + the running offset, in place);
// then the session's state moves on. Every thread reads the running offset in front of the barrier of zd_scan_tiles, thread 0
// writes the state behind it. vctl != NULL: the piece is a chunk of an appendv. After a table error its blocks were never encoded,
// their sizes are whatever the slots' last user left, and the session's state stays as the scan left it: the whole workgroup
// returns in front of the barrier.
extern "C" __global__ void __launch_bounds__(256)
zxc_append_advance_kernel(uint64_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_hash, const uint32_t* __restrict__ tile_bad,
                          uint32_t n_tiles, uint32_t nb_piece, uint64_t dst_capacity, uint32_t checksum, uint32_t seekable,
                          zap_ctl_t* __restrict__ ctl, const zav_ctl_t* __restrict__ vctl) {
    if (vctl && vctl->status < 0) return;
    const uint64_t base = ctl->off;
    const zd_totals all = zd_scan_tiles(
        n_tiles, base,
        [=](uint32_t i, uint32_t& hash, uint32_t& bad) { const uint64_t s = tile_sum[i]; hash ^= tile_hash[i]; bad |= tile_bad[i]; return s; },
        [=](uint32_t i, uint64_t off) { tile_sum[i] = off; });
    if (threadIdx.x == 0) zap_advance(ctl, nb_piece, all.sum, all.hash, all.bad, dst_capacity, (int)checksum, (int)seekable);
}

// Per tile: offsets[b] = archive offset of the piece's block b; with a seek table also its entry, ctl->first + b of the array.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_append_scatter_kernel(const uint32_t* __restrict__ sizes, uint32_t nb_piece, const uint64_t* __restrict__ tile_off,
                          uint64_t* __restrict__ offsets, uint32_t* __restrict__ seek, uint32_t seekable, const zap_ctl_t* __restrict__ ctl) {
    if (ctl->status < 0) return;
    const uint32_t b0 = blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint32_t sz[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        sz[j] = b0 + j < nb_piece ? sizes[b0 + j] : 0u;
        sum += sz[j];
    }
    uint64_t run = zd_tile_offset(sum, tile_off[blockIdx.x]);
    const uint64_t first = ctl->first;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        const uint32_t b = b0 + j;
        if (b >= nb_piece) break;
        offsets[b] = run;
        run += sz[j];
        if (seekable) seek[first + b] = sz[j];
    }
}

// Compaction, one wave per block: block b's sizes[b] bytes at its slot -> dst + offsets[b]. While the status is no error every
// size of the piece lies in [8, block_size + 64] and the blocks so far, this piece's included, end in front of the capacity
// (zap_advance): nothing is written at or past offsets[b] + sizes[b].
extern "C" __global__ void __launch_bounds__(256)
zxc_append_gather_kernel(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes,
                         const uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst, uint32_t nb_piece, const zap_ctl_t* __restrict__ ctl) {
    if (ctl->status < 0) return;
    zd_gather_blocks(slots, slot_stride, sizes, offsets, dst, nb_piece);
}

// dict_id != NULL (the dictionary session): the file header carries the flag and *dict_id, a word in device memory read here.
extern "C" __global__ void zxc_append_finish_kernel(zap_ctl_t* __restrict__ ctl, uint8_t* __restrict__ dst, uint64_t dst_capacity,
                                                    uint64_t total, uint32_t block_size, uint32_t checksum, uint32_t seekable,
                                                    const uint32_t* __restrict__ dict_id) {
    if (threadIdx.x == 0)
        zap_finish_dict(ctl, dst, dst_capacity, total, block_size, (int)checksum, (int)seekable, dict_id != NULL, dict_id ? *dict_id : 0u);
}

extern "C" __global__ void __launch_bounds__(256)
zxc_append_seek_kernel(const zap_ctl_t* __restrict__ ctl, uint8_t* __restrict__ dst, const uint32_t* __restrict__ seek, uint32_t nb) {
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x)
        zap_put_seek_entry(ctl, dst, seek, b);
}

extern "C" __global__ void zxc_append_result_kernel(const zap_ctl_t* __restrict__ ctl, int64_t* __restrict__ result) {
    if (threadIdx.x == 0) *result = ctl->status;
}

// ---------------------------------------------------------------- appendv: a table of sources (zxc_appendv.h)
// The scan of a call, three tile passes of 256 threads over tiles of 1024 entries, like the passes of zxc_device_util.h but over
// 64-bit lengths that add up saturating (zav_sat_add), so that a table whose sum passes 2^64 is still seen as above `total`. The
// workgroup scan itself is zd_wg_scan64 of zxc_device_util.h (same adds), which the pack call's passes use as well.

// The flags of the check ored over the workgroup (__syncthreads_or answers only whether any thread's value is non-zero). Two barriers.
__device__ __forceinline__ uint32_t zav_wg_flags(uint32_t flags) {
    const uint32_t null = __syncthreads_or((int)(flags & ZAV_NULL)) ? ZAV_NULL : 0u;
    const uint32_t big = __syncthreads_or((int)(flags & ZAV_BIG)) ? ZAV_BIG : 0u;
    return null | big;
}

// Reduce, per tile: the sum of the tile's lengths and the flags of its entries.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_appendv_reduce_kernel(const zxc_dev_iov_t* __restrict__ iov, uint32_t n_iov, uint64_t total, uint64_t* __restrict__ tile_sum,
                          uint32_t* __restrict__ tile_flags) {
    const uint64_t r0 = (uint64_t)blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint64_t sum = 0;
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        if (r0 + j >= n_iov) break;
        const zxc_dev_iov_t e = iov[r0 + j];
        flags |= zav_entry_flags(e.base, e.len, total);
        sum = zav_sat_add(sum, e.len);
    }
    uint64_t all;
    (void)zd_wg_scan64(sum, &all);
    flags = zav_wg_flags(flags);
    if (threadIdx.x == 0) { tile_sum[blockIdx.x] = all; tile_flags[blockIdx.x] = flags; }
}

// One workgroup: tile_sum[t] becomes the virtual offset of tile t's first entry; the table's verdict goes to the call's control
// word, which every later kernel of the call reads, and into the session's status unless that holds an error already.
extern "C" __global__ void __launch_bounds__(256)
zxc_appendv_scan_kernel(uint64_t* __restrict__ tile_sum, const uint32_t* __restrict__ tile_flags, uint32_t n_tiles, uint64_t total,
                        uint64_t* __restrict__ starts, uint32_t n_iov, zav_ctl_t* __restrict__ vctl, zap_ctl_t* __restrict__ ctl) {
    const uint32_t t = threadIdx.x, per = (n_tiles + 255u) / 256u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    uint64_t mine = 0;
    uint32_t flags = 0;
    for (uint32_t i = lo; i < hi; i++) { mine = zav_sat_add(mine, tile_sum[i]); flags |= tile_flags[i]; }
    uint64_t all;
    uint64_t run = zd_wg_scan64(mine, &all);
    flags = zav_wg_flags(flags);
    for (uint32_t i = lo; i < hi; i++) {
        const uint64_t s = tile_sum[i];
        tile_sum[i] = run;
        run = zav_sat_add(run, s);
    }
    if (t == 0) {
        const int status = zav_table_status(flags, all, total);
        vctl->status = status; vctl->rsv = 0; vctl->sum = all;
        starts[n_iov] = all;
        zav_fold_status(ctl, status);
    }
}

// Scatter, per tile: starts[r] = the virtual offset of entry r.
extern "C" __global__ void __launch_bounds__(ZD_TILE_THREADS)
zxc_appendv_starts_kernel(const zxc_dev_iov_t* __restrict__ iov, uint32_t n_iov, const uint64_t* __restrict__ tile_off,
                          uint64_t* __restrict__ starts) {
    const uint64_t r0 = (uint64_t)blockIdx.x * ZC_TILE_BLOCKS + threadIdx.x * ZD_PER_THREAD;
    uint64_t len[ZD_PER_THREAD], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        len[j] = r0 + j < n_iov ? iov[r0 + j].len : 0u;
        sum = zav_sat_add(sum, len[j]);
    }
    uint64_t all;
    uint64_t run = zav_sat_add(tile_off[blockIdx.x], zd_wg_scan64(sum, &all));
#pragma unroll
    for (uint32_t j = 0; j < ZD_PER_THREAD; j++) {
        if (r0 + j >= n_iov) break;
        starts[r0 + j] = run;
        run = zav_sat_add(run, len[j]);
    }
}

// Prep of one chunk: workgroup w runs task w of the chunk's plan (zav_prep: the gather into the carry areas and the images, the
// in-place jobs, the job table), the new hot path: a chunk made of small entries passes through it whole.
extern "C" __global__ void __launch_bounds__(256)
zxc_appendv_prep_kernel(const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, uint32_t n_iov,
                        const zav_ctl_t* __restrict__ vctl, zav_chunk_t c, uint8_t* __restrict__ carry, uint8_t* __restrict__ next,
                        uint8_t* __restrict__ images, uint32_t image, zxc_enc_job_t* __restrict__ jobs) {
    zav_prep(iov, starts, n_iov, vctl->status, &c, blockIdx.x, threadIdx.x, blockDim.x, carry, next, images, image, jobs);
}

// The same chunk in a session with a dictionary, for the jobs [j0, j0 + n) of it: workgroup w < n gathers image w of the session's
// image area, [dict | the job's bytes], from the entries (zav_prep_images); workgroup n, which only the first launch of a chunk
// has, gathers the tail. The grid is n + (j0 == 0).
extern "C" __global__ void __launch_bounds__(ZAP_IMAGE_THREADS)
zxc_appendv_images_kernel(const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, uint32_t n_iov,
                          const zav_ctl_t* __restrict__ vctl, zav_chunk_t c, uint32_t j0, uint32_t n, const uint8_t* __restrict__ dict,
                          uint32_t dict_size, const uint8_t* __restrict__ carry, uint8_t* __restrict__ next, uint8_t* __restrict__ images,
                          zxc_enc_job_t* __restrict__ jobs) {
    zav_prep_images(iov, starts, n_iov, vctl->status, &c, j0, n, blockIdx.x, threadIdx.x, blockDim.x, dict, dict_size, carry, next, images, jobs);
}

// ---------------------------------------------------------------- host side
namespace {

#define SESS_LIVE 0x7a78632d61707064ull  // a session between begin and end

// What zxc_dev_cappend_t holds: the arguments of begin and the bytes appended. The work area's layout follows from them.
struct Sess {
    uint64_t magic;
    uint8_t* dst;
    uint64_t dst_capacity, max_total, max_piece;
    uint8_t* base;  // the work area's aligned base
    uint64_t total;
    uint32_t block_size, level, checksum, seekable;
    uint32_t cur;   // which of the two carry areas holds the waiting bytes
    uint32_t dict_size;         // 0: a session without a dictionary, the two pointers below NULL
    const uint8_t* dict;        // the dictionary's d_content
    const uint32_t* dict_id;    // ... and its d_id
};
static_assert(sizeof(Sess) <= sizeof(zxc_dev_cappend_t), "the session fits the caller's struct");

// The options of a session (zd_compress_opts), refused in the order of zxc_mi355x_compress_device.
int ap_opts(const zxc_compress_opts_t* opts, Sess* s) {
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    zd_copts_t o;
    const int rc = zd_compress_opts(opts, &o);
    if (rc != ZXC_OK) return rc;
    s->block_size = o.block_size; s->level = o.level; s->checksum = o.checksum; s->seekable = o.seekable;
    return ZXC_OK;
}
int ap_shape(const Sess& s, zap_shape_images_t* sh) {
    return zap_shape_images(s.max_total, s.max_piece, s.block_size, zxc_mi355x_encode_slot_stride(s.block_size), (int)s.seekable,
                            s.dict_size, sh);
}

// The parts of a session's work area. The carry area that holds the waiting bytes is carry[s.cur].
struct Work {
    zap_ctl_t* ctl;
    uint64_t *tile_sum, *offsets;
    uint32_t *tile_hash, *tile_bad, *sizes, *seek;
    zxc_enc_job_t* jobs;
    uint8_t *slots, *stage, *images, *carry[2];
    uint32_t slot_stride, chunk_jobs;
};
Work ap_work(const Sess& s, const zap_shape_images_t& shi) {
    const zap_shape_t& sh = shi.s;
    uint8_t* base = s.base;
    Work w;
    w.ctl = (zap_ctl_t*)base; w.jobs = (zxc_enc_job_t*)(base + sh.o_jobs);
    w.tile_sum = (uint64_t*)(base + sh.o_tile_sum); w.offsets = (uint64_t*)(base + sh.o_offsets);
    w.tile_hash = (uint32_t*)(base + sh.o_tile_hash); w.tile_bad = (uint32_t*)(base + sh.o_tile_bad);
    w.sizes = (uint32_t*)(base + sh.o_sizes); w.seek = (uint32_t*)(base + sh.o_seek);
    w.slots = base + sh.o_slots; w.stage = base + sh.o_stage; w.images = base + shi.o_images;
    w.carry[0] = base + sh.o_carry[0]; w.carry[1] = base + sh.o_carry[1];
    w.slot_stride = sh.slot_stride; w.chunk_jobs = shi.chunk_jobs;
    return w;
}

// The virtual source of an appendv (zxc_appendv.h): the table, what the call's scan left in its scratch, and the offset in the
// concatenation of the chunk at hand.
struct Vsrc {
    const zxc_dev_iov_t* iov;
    uint32_t n_iov, image;
    const uint64_t* starts;
    const zav_ctl_t* vctl;
    uint8_t* images;
    uint64_t v;
};

// ---- the front ends of a piece: the job table and the encode launch over it
// the encode launch of the two front ends without a dictionary: job j's src_off is an address
int ap_encode(const Sess& s, const Work& w, uint32_t nb, hipStream_t st) {
    return zxc_hip_encode_jobs(NULL, w.jobs, nb, s.block_size, (int)s.level, (int)s.checksum, NULL, 0u, NULL, w.slots, w.sizes, (void*)st);
}
// src is the piece's first byte (not read when the plan has no copy and no direct job)
int ap_front_plain(const Sess& s, const Work& w, const uint8_t* src, const zap_piece_t& p, hipStream_t st) {
    const uint64_t units = ((uint64_t)p.cp[0].len + p.cp[1].len + p.cp[2].len) / 16u + p.nb;  // a thread moves 16 bytes or writes a job
    const uint32_t groups = units < 256u ? 1u : units / 256u < 1024u ? (uint32_t)(units / 256u) : 1024u;
    hipLaunchKernelGGL(zxc_append_prep_kernel, dim3(groups), dim3(256), 0, st, src, p, w.carry[s.cur], w.carry[s.cur ^ 1u], w.stage, w.jobs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    return p.nb ? ap_encode(s, w, p.nb, st) : ZXC_OK;
}
// Blocks are independent, so chunk by chunk gives the bytes of one launch over all of them. A chunk's images are built and
// consumed in stream order before the next chunk overwrites them (frame_enqueue of zxc_frame_device.hip). p.nb > 0.
int ap_front_images(const Sess& s, const Work& w, const uint8_t* src, const zap_piece_t& p, hipStream_t st) {
    for (uint32_t j0 = 0; j0 < p.nb; j0 += w.chunk_jobs) {
        const uint32_t n = p.nb - j0 < w.chunk_jobs ? p.nb - j0 : w.chunk_jobs;
        hipLaunchKernelGGL(zxc_append_images_kernel, dim3(n + (j0 == 0 ? 1u : 0u)), dim3(ZAP_IMAGE_THREADS), 0, st, src, p, j0, n, s.dict,
                           s.dict_size, (const uint8_t*)w.carry[s.cur], w.carry[s.cur ^ 1u], w.images, w.jobs);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
        const int rc = zxc_hip_encode_job_images(w.images, w.jobs + j0, n, s.block_size, (int)s.level, (int)s.checksum, s.dict_size,
                                                 w.slots + (uint64_t)j0 * w.slot_stride, w.sizes + j0, (void*)st);
        if (rc != ZXC_OK) return rc;
    }
    return ZXC_OK;
}
int ap_front_v(const Sess& s, const Work& w, const Vsrc& vs, const zap_piece_t& p, hipStream_t st) {
    zav_chunk_t c;
    c.p = p; c.v = vs.v;
    hipLaunchKernelGGL(zxc_appendv_prep_kernel, dim3(zav_groups(&c)), dim3(256), 0, st, vs.iov, vs.starts, vs.n_iov, vs.vctl, c, w.carry[s.cur],
                       w.carry[s.cur ^ 1u], vs.images, vs.image, w.jobs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    return p.nb ? ap_encode(s, w, p.nb, st) : ZXC_OK;
}
// The chunk loop of ap_front_images over the table's entries. p.nb > 0, s.dict_size != 0.
int ap_front_v_images(const Sess& s, const Work& w, const Vsrc& vs, const zap_piece_t& p, hipStream_t st) {
    zav_chunk_t c;
    c.p = p; c.v = vs.v;
    for (uint32_t j0 = 0; j0 < p.nb; j0 += w.chunk_jobs) {
        const uint32_t n = p.nb - j0 < w.chunk_jobs ? p.nb - j0 : w.chunk_jobs;
        hipLaunchKernelGGL(zxc_appendv_images_kernel, dim3(n + (j0 == 0 ? 1u : 0u)), dim3(ZAP_IMAGE_THREADS), 0, st, vs.iov, vs.starts, vs.n_iov,
                           vs.vctl, c, j0, n, s.dict, s.dict_size, (const uint8_t*)w.carry[s.cur], w.carry[s.cur ^ 1u], w.images, w.jobs);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
        const int rc = zxc_hip_encode_job_images(w.images, w.jobs + j0, n, s.block_size, (int)s.level, (int)s.checksum, s.dict_size,
                                                 w.slots + (uint64_t)j0 * w.slot_stride, w.sizes + j0, (void*)st);
        if (rc != ZXC_OK) return rc;
    }
    return ZXC_OK;
}

// The back half of a piece that completes nb > 0 blocks: tiles, advance, scatter, gather. vctl: the verdict of the appendv whose
// chunk the piece is, or NULL.
int ap_back(const Sess& s, const Work& w, uint32_t nb, const zav_ctl_t* vctl, hipStream_t st) {
    const uint32_t n_tiles = (nb + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS;
    hipLaunchKernelGGL(zxc_frame_tiles_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, (const uint8_t*)w.slots, w.slot_stride,
                       (const uint32_t*)w.sizes, nb, s.block_size, s.checksum, w.tile_sum, w.tile_hash, w.tile_bad);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_append_advance_kernel, dim3(1), dim3(256), 0, st, w.tile_sum, (const uint32_t*)w.tile_hash, (const uint32_t*)w.tile_bad,
                       n_tiles, nb, s.dst_capacity, s.checksum, s.seekable, w.ctl, vctl);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_append_scatter_kernel, dim3(n_tiles), dim3(ZD_TILE_THREADS), 0, st, (const uint32_t*)w.sizes, nb,
                       (const uint64_t*)w.tile_sum, w.offsets, w.seek, s.seekable, (const zap_ctl_t*)w.ctl);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint32_t waves = (nb + 3u) / 4u < 65536u ? (nb + 3u) / 4u : 65536u;
    hipLaunchKernelGGL(zxc_append_gather_kernel, dim3(waves), dim3(256), 0, st, (const uint8_t*)w.slots, w.slot_stride, (const uint32_t*)w.sizes,
                       (const uint64_t*)w.offsets, s.dst, nb, (const zap_ctl_t*)w.ctl);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

// One piece behind its plan. vs != NULL: a chunk of an appendv, src is not looked at. Else src is the piece's first byte, NULL for
// the plan of `end`. A piece that completes no block ends behind the plain prep or appendv's, with a dictionary or without.
int ap_piece(const Sess& s, const Work& w, const uint8_t* src, const Vsrc* vs, const zap_piece_t& p, hipStream_t st) {
    const int rc = vs ? (s.dict_size && p.nb ? ap_front_v_images(s, w, *vs, p, st) : ap_front_v(s, w, *vs, p, st))
                      : s.dict_size && p.nb ? ap_front_images(s, w, src, p, st) : ap_front_plain(s, w, src, p, st);
    if (rc != ZXC_OK || !p.nb) return rc;
    return ap_back(s, w, p.nb, vs ? vs->vctl : NULL, st);
}

// The next n bytes of the source, at src or (vs != NULL) from vs->v of an appendv's table, and the session back into *cs. rc:
// what the launches in front of the pieces gave; nothing more is enqueued behind an error.
// Pieces are independent but for the state, so piece by piece gives the archive of one piece over all the bytes. A piece's areas,
// jobs and slots are written and consumed in stream order before the next piece overwrites them. Every piece but the last ends on
// a block boundary of the archive.
int ap_pieces(zxc_dev_cappend_t* cs, Sess& s, const zap_shape_images_t& sh, const uint8_t* src, Vsrc* vs, uint64_t n, int rc, hipStream_t st) {
    const Work w = ap_work(s, sh);
    uint64_t left = n;
    while (left && rc == ZXC_OK) {
        const uint32_t carry = (uint32_t)(s.total % s.block_size);
        const uint64_t m = zap_piece_len(carry, left, s.max_piece, s.block_size);
        zap_piece_t p;
        if (s.dict_size) zap_plan_piece_images(carry, m, s.block_size, &p);
        else zap_plan_piece(carry, m, s.block_size, &p);
        rc = ap_piece(s, w, src, vs, p, st);
        if (p.swap) s.cur ^= 1u;
        s.total += m; left -= m;
        if (vs) vs->v += m;
        else src += m;
    }
    if (rc != ZXC_OK) s.magic = 0;  // part of the call may be enqueued: the session cannot go on
    memcpy(cs, &s, sizeof s);
    return rc;
}

// Both kinds of begin behind their names. dict == NULL: the session without a dictionary.
int ap_begin(zxc_dev_cappend_t* cs, void* d_dst, uint64_t dst_capacity, uint64_t max_total, uint64_t max_piece, const zxc_compress_opts_t* opts,
             const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, void* stream) {
    if (!cs || !d_dst || !d_work) return ZXC_ERROR_NULL_INPUT;
    Sess s = {};
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    const int orc = ap_opts(opts, &s);
    if (orc != ZXC_OK) return orc;
    s.dst = (uint8_t*)d_dst; s.dst_capacity = dst_capacity; s.max_total = max_total; s.max_piece = max_piece;
    s.base = zd_work_base(d_work);
    if (dict) { s.dict = (const uint8_t*)dict->d_content; s.dict_id = dict->d_id; s.dict_size = dict->size; }
    zap_shape_images_t sh;
    const int src = ap_shape(s, &sh);
    if (src != 0) return src;
    if (work_size < sh.bytes) return ZXC_ERROR_MEMORY;
    if (dst_capacity < zc_known_size(0u, (int)s.checksum, (int)s.seekable)) return ZXC_ERROR_DST_TOO_SMALL;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_append_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (zap_ctl_t*)s.base);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    s.magic = SESS_LIVE;
    memset(cs, 0, sizeof *cs);
    memcpy(cs, &s, sizeof s);
    return ZXC_OK;
}

// Both kinds of appendv behind their names. with_dict: the call that serves a session begun with a dictionary; the other refuses it.
int ap_appendv(zxc_dev_cappend_t* cs, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_scratch, uint64_t scratch_size,
               void* stream, bool with_dict) {
    if (!cs || !d_scratch || (n_iov > 0 && !d_iov)) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    memcpy(&s, cs, sizeof s);
    if (s.magic != SESS_LIVE) return ZXC_ERROR_NULL_INPUT;
    if (s.dict_size && !with_dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_SRC_TOO_SMALL;
    if (total > s.max_total - s.total) return ZXC_ERROR_OVERFLOW;
    zap_shape_images_t sh;
    zav_shape_t vsh;
    if (ap_shape(s, &sh) != 0 || zav_shape_dict(n_iov, s.max_piece, s.block_size, s.dict_size, &vsh) != 0) return ZXC_ERROR_NULL_INPUT;  // (begin accepted these)
    if (scratch_size < vsh.bytes) return ZXC_ERROR_MEMORY;
    if (n_iov == 0) return ZXC_OK;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* sb = zd_work_base(d_scratch);
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + vsh.o_starts);
    // The scan, once per call: the chunks read starts and the verdict in stream order.
    const int rc = zd_iov_scan(d_iov, n_iov, total, vsh.n_tiles, (uint64_t*)(sb + vsh.o_tile_sum), (uint32_t*)(sb + vsh.o_tile_flags), starts, vctl,
                               (zap_ctl_t*)s.base, st);
    // The chunks, cut like the pieces of an append of `total` bytes.
    Vsrc vs = {d_iov, n_iov, vsh.image, starts, vctl, sb + vsh.o_images, 0u};
    return ap_pieces(cs, s, sh, NULL, &vs, total, rc, st);
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_compress_append_dict_device_work_size(uint64_t max_total, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                          uint32_t dict_size) {
    Sess s = {};
    zap_shape_images_t sh;
    if (ap_opts(opts, &s) != ZXC_OK || dict_size > ZC_DICT_MAX) return 0u;
    s.max_total = max_total; s.max_piece = max_piece; s.dict_size = dict_size;
    return ap_shape(s, &sh) == 0 ? sh.bytes : 0u;
}

uint64_t zxc_mi355x_compress_append_device_work_size(uint64_t max_total, uint64_t max_piece, const zxc_compress_opts_t* opts) {
    return zxc_mi355x_compress_append_dict_device_work_size(max_total, max_piece, opts, 0u);
}

int zxc_mi355x_compress_begin_device(zxc_dev_cappend_t* cs, void* d_dst, uint64_t dst_capacity, uint64_t max_total, uint64_t max_piece,
                                     const zxc_compress_opts_t* opts, void* d_work, uint64_t work_size, void* stream) {
    return ap_begin(cs, d_dst, dst_capacity, max_total, max_piece, opts, NULL, d_work, work_size, stream);
}

int zxc_mi355x_compress_begin_dict_device(zxc_dev_cappend_t* cs, void* d_dst, uint64_t dst_capacity, uint64_t max_total,
                                          uint64_t max_piece, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                          uint64_t work_size, void* stream) {
    return ap_begin(cs, d_dst, dst_capacity, max_total, max_piece, opts, dict, d_work, work_size, stream);
}

int zxc_mi355x_compress_append_device(zxc_dev_cappend_t* cs, const void* d_src, uint64_t n, void* stream) {
    if (!cs || (n > 0 && !d_src)) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    memcpy(&s, cs, sizeof s);
    if (s.magic != SESS_LIVE) return ZXC_ERROR_NULL_INPUT;
    if (n > s.max_total - s.total) return ZXC_ERROR_OVERFLOW;
    if (n == 0) return ZXC_OK;
    zap_shape_images_t sh;
    if (ap_shape(s, &sh) != 0) return ZXC_ERROR_NULL_INPUT;  // (begin accepted these)
    return ap_pieces(cs, s, sh, (const uint8_t*)d_src, NULL, n, ZXC_OK, (hipStream_t)stream);
}

uint64_t zxc_mi355x_compress_appendv_dict_device_scratch_size(uint32_t n_iov, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                              uint32_t dict_size) {
    Sess s = {};
    zav_shape_t sh;
    if (ap_opts(opts, &s) != ZXC_OK || dict_size > ZC_DICT_MAX) return 0u;
    return zav_shape_dict(n_iov, max_piece, s.block_size, dict_size, &sh) == 0 ? sh.bytes : 0u;
}

uint64_t zxc_mi355x_compress_appendv_device_scratch_size(uint32_t n_iov, uint64_t max_piece, const zxc_compress_opts_t* opts) {
    return zxc_mi355x_compress_appendv_dict_device_scratch_size(n_iov, max_piece, opts, 0u);
}

int zxc_mi355x_compress_appendv_device(zxc_dev_cappend_t* cs, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_scratch,
                                       uint64_t scratch_size, void* stream) {
    return ap_appendv(cs, d_iov, n_iov, total, d_scratch, scratch_size, stream, false);
}

int zxc_mi355x_compress_appendv_dict_device(zxc_dev_cappend_t* cs, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total,
                                            void* d_scratch, uint64_t scratch_size, void* stream) {
    return ap_appendv(cs, d_iov, n_iov, total, d_scratch, scratch_size, stream, true);
}

int zxc_mi355x_compress_end_device(zxc_dev_cappend_t* cs, int64_t* d_result, void* stream) {
    if (!cs || !d_result) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    memcpy(&s, cs, sizeof s);
    if (s.magic != SESS_LIVE) return ZXC_ERROR_NULL_INPUT;
    memset(cs, 0, sizeof *cs);  // spent, whatever happens below
    zap_shape_images_t sh;
    if (ap_shape(s, &sh) != 0) return ZXC_ERROR_NULL_INPUT;
    const hipStream_t st = (hipStream_t)stream;
    const Work w = ap_work(s, sh);
    zap_piece_t p;
    zap_plan_end((uint32_t)(s.total % s.block_size), s.block_size, &p);
    if (p.nb) {
        const int rc = ap_piece(s, w, NULL, NULL, p, st);
        if (rc != ZXC_OK) return rc;
    }
    hipLaunchKernelGGL(zxc_append_finish_kernel, dim3(1), dim3(64), 0, st, w.ctl, s.dst, s.dst_capacity, s.total, s.block_size, s.checksum, s.seekable,
                       s.dict_size ? s.dict_id : (const uint32_t*)NULL);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const uint64_t nb = s.total / s.block_size + (s.total % s.block_size != 0);  // <= 2^31 - 1 (begin)
    if (s.seekable && nb) {
        const uint32_t groups = (nb + 255u) / 256u < 4096u ? (uint32_t)((nb + 255u) / 256u) : 4096u;
        hipLaunchKernelGGL(zxc_append_seek_kernel, dim3(groups), dim3(256), 0, st, (const zap_ctl_t*)w.ctl, s.dst, (const uint32_t*)w.seek, (uint32_t)nb);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    }
    hipLaunchKernelGGL(zxc_append_result_kernel, dim3(1), dim3(64), 0, st, (const zap_ctl_t*)w.ctl, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // extern "C"
