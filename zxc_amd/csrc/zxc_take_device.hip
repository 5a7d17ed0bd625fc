// zxc_take_device.hip — zxc_mi355x_decompress_begin_device / _take_device / _takev_device / _end_device: one v8 archive in device
// memory decoded into a destination that is handed over in pieces, each in device memory (takev: a table of them, zxc_takev.h).
// The device counterpart of pulling from zxc_dstream_* (zxc_pstream_host.c) and the mirror image of the append session
// (zxc_append_device.hip).
//
// zxc_mi355x_decompress_device (zxc_unframe_device.hip) wants one contiguous, 16-byte aligned destination of the whole decoded
// size. Here a session parses the container once, keeps the block index and one status word per block in its work area, and every
// take decodes the next n bytes to a destination of its own. The host knows block_size, the position and every n, so it knows which
// block lands where and each launch's exact grid: the plan of a chunk and its advance are the inline C of zxc_take.h, which the
// CPU tests run as well. The container rules are zxc_container.h's and the container kernels zxc_unframe_device.hip's, as they are.
//
//   begin    clear, head, tiles, scan, scatter, walk: the stages of zxc_mi355x_decompress_device over n_jobs = ceil(capacity / bs) + 1
//            jobs, whose out_off nobody reads                                                  -> control word, block index
//
// the stream order of one chunk (a take of at most max_piece bytes; a longer one is a loop of these):
//
//   plan     one thread per block the chunk decodes: its index entry with out_off into the piece, a slot or the next carry slot
//   decode   the existing decode launch over the chunk's table (two tables with verification, as in that call); the statuses go
//            to the blocks' words of the session's status table
//   copy     carry slot -> head of the piece, slots -> piece, next carry slot -> tail of the piece: min(decoded size, bytes wanted)
//            of each, one wavefront per 8 KiB of destination. Behind the decode launches: a block decoded straight into the piece
//            may store up to 32 bytes behind itself, into what a copy fills.
//
// and of `end`: block n_max, the one job behind the capacity, decoded into a slot for its status; then
//
//   events   zxc_unframe_events_kernel over the whole status table
//   result   zxc_unframe_result_kernel: *d_result, written once, after everything above
//
// No workgroup waits for another: every dependency is the stream order between launches, and every stage is predicated on the
// control word.
//
// The host side, as the append session's: tk_load reads the caller's struct for take, takev and end; tk_chunks is the one chunk
// loop and the one store, over a destination pointer or a Vdst; tk_chunk and tkv_chunk are its two front ends (their plan and copy
// kernels differ), whose decode step is tk_tables. begin's stages, end's verdict, the tables loop and the scan of a takev's table
// are zxc_device_util.h's (zd_container_stages, zd_verdict_stages, zd_decode_tables, zd_iov_scan), which other calls launch too.
#include <string.h>

#include "zxc_device_util.h"  // zd_copy_chunk, the host-side plumbing and shared launches (zxc_kernels.h through it)
#include "zxc_take.h"
#include "zxc_takev.h"

static_assert(ZT_COPY_CHUNK == ZD_COPY_CHUNK, "the shape counts the chunks zd_copy_chunk moves");
static_assert(2 * sizeof(zxc_dev_job_t) + 2 * 4 == ZT_BLOCK_BYTES && 2 * sizeof(zxc_dev_job_t) == ZT_JOB_BYTES, "the documented work size");
static_assert(sizeof(zc_ctl_t) <= 256, "the state's place at the start of the work area");
static_assert(sizeof(ztv_place_t) == ZTV_PLACE_BYTES && 8 + 4 + 4 == ZTV_TILE_BYTES, "the documented scratch size");
static_assert(sizeof(zav_ctl_t) <= ZTV_SINK && ZTV_SINK + sizeof(zap_ctl_t) <= 256, "the call's control word and the unread zap_ctl_t");

// ---------------------------------------------------------------- kernels
// Job j of the chunk is block c.first + j of the index (both tables: the head stage left one of them empty), decoded where the
// plan says. The launch's d_out is one base below the piece and the work area: piece = base + dst_rel, carry slot s = base +
// carry_rel[s], slot i = base + slots_rel + i slot_stride. c.first + c.nb <= n_jobs (the takes end at the capacity; `end` asks
// for the last job), c.nb <= J.
extern "C" __global__ void __launch_bounds__(256)
zxc_take_plan_kernel(const zxc_dev_job_t* __restrict__ index, uint32_t n_jobs, uint32_t tables, zt_chunk_t c, uint64_t dst_rel,
                     uint64_t carry_rel0, uint64_t carry_rel1, uint64_t slots_rel, uint32_t slot_stride, uint32_t J,
                     zxc_dev_job_t* __restrict__ cjobs) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= c.nb || j >= J || c.first + j >= n_jobs) return;
    const zt_place_t p = zt_job_place(&c, j);
    const uint64_t out_off = p.kind == ZT_DIRECT ? dst_rel + p.at
                             : p.kind == ZT_SLOT ? slots_rel + (uint64_t)p.slot * slot_stride
                                                 : (p.slot ? carry_rel1 : carry_rel0);
    for (uint32_t tb = 0; tb < tables; tb++) {
        zxc_dev_job_t job = index[(uint64_t)tb * n_jobs + c.first + j];
        job.out_off = out_off;
        cjobs[(uint64_t)tb * J + j] = job;
    }
}

// One wavefront per (copy, 8 KiB of destination), as in zxc_batch_copy_kernel: copy k of the plan moves min(decoded size, bytes
// wanted) of its block from the slot or carry slot to its place in the piece, at any alignment. Most units are empty (blocks
// decoded straight, chunks behind a short copy) and end at once. A block the chain does not have moves nothing.
extern "C" __global__ void __launch_bounds__(256)
zxc_take_copy_kernel(const uint8_t* __restrict__ carry0, const uint8_t* __restrict__ carry1, const uint8_t* __restrict__ slots,
                     uint32_t slot_stride, zt_chunk_t c, const int32_t* __restrict__ status, uint32_t n_jobs,
                     const zc_ctl_t* __restrict__ ctl, uint32_t chunks, uint8_t* __restrict__ dst) {
    if (ctl->final) return;
    const uint32_t lane = threadIdx.x & 63u, found = ctl->found;
    const int32_t* st = status + (uint64_t)ctl->sel * n_jobs;
    const uint64_t units = ((uint64_t)c.nb + 1u) * chunks, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < units; it += waves) {
        const uint32_t k = (uint32_t)(it / chunks), ch = (uint32_t)(it - (uint64_t)k * chunks);
        const zt_copy_t cp = zt_copy(&c, k);
        if (cp.kind == ZT_NONE || cp.block >= found) continue;
        const uint32_t n = zt_copy_bytes(&cp, st[cp.block], c.block_size);
        uint8_t* d = dst + cp.to;
        if (n == 0 || (uint64_t)ch * ZT_COPY_CHUNK >= ((uintptr_t)d & 15u) + n) continue;
        const uint8_t* s = (cp.kind == ZT_SLOT ? slots + (uint64_t)cp.slot * slot_stride : cp.slot ? carry1 : carry0) + cp.from;
        zd_copy_chunk(d, s, (int64_t)n, ch, lane);
    }
}

// ---------------------------------------------------------------- takev: a table of destinations (zxc_takev.h)
// The stream order of one call: the scan of zxc_mi355x_compress_appendv_device (zxc_appendv_reduce_kernel, _scan_kernel,
// _starts_kernel as they are: starts[0 .. n_iov] and the table's status in the call's control word), the fold below, then per chunk
// plan, the decode launch and copy.

// One thread: the table's status becomes the call's verdict and, an error, the session's result unless that is final already.
extern "C" __global__ void zxc_takev_fold_kernel(zav_ctl_t* __restrict__ vctl, zc_ctl_t* __restrict__ ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int verdict = ztv_verdict(vctl->status);
    vctl->status = verdict;
    ztv_fold(ctl, verdict);
}

// zxc_take_plan_kernel over a virtual destination: job j of the chunk is block c.c.first + j of the index, decoded where
// ztv_job_place says (inside its entry, into slot j, into the next carry slot); the job's out_off is that address minus the
// launch's d_out (the work area's base) modulo 2^64, a multiple of 16. Behind a table error, and in a session whose result is
// final, every job is written empty and neither the table nor an entry is read.
extern "C" __global__ void __launch_bounds__(256)
zxc_takev_plan_kernel(const zxc_dev_job_t* __restrict__ index, uint32_t n_jobs, uint32_t tables, ztv_chunk_t c,
                      const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, uint32_t n_iov,
                      const zav_ctl_t* __restrict__ vctl, const zc_ctl_t* __restrict__ ctl, uint64_t out_base, uint64_t carry0, uint64_t carry1,
                      uint64_t slots, uint32_t slot_stride, uint32_t J, zxc_dev_job_t* __restrict__ cjobs, ztv_place_t* __restrict__ places) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= c.c.nb || j >= J || c.c.first + j >= n_jobs) return;
    if (vctl->status < 0 || ctl->final) {
        const zxc_dev_job_t empty = {0u, slots + (uint64_t)j * slot_stride - out_base, 0u, c.c.block_size};  // (its wave leaves at once)
        const ztv_place_t none = {ZT_NONE, 0u, 0u};
        for (uint32_t tb = 0; tb < tables; tb++) cjobs[(uint64_t)tb * J + j] = empty;
        places[j] = none;
        return;
    }
    uint64_t addr;
    places[j] = ztv_job_place(&c, j, iov, starts, n_iov, carry0, carry1, slots, slot_stride, &addr);
    for (uint32_t tb = 0; tb < tables; tb++) {
        zxc_dev_job_t job = index[(uint64_t)tb * n_jobs + c.c.first + j];
        job.out_off = addr - out_base;
        cjobs[(uint64_t)tb * J + j] = job;
    }
}

// zxc_take_copy_kernel over a virtual destination, one wavefront per (copy, 8 KiB): a copy whose bytes lie inside one entry is
// zd_copy_chunk to its place there, 8 KiB of destination per wavefront; one that meets an entry boundary is the scatter, 8 KiB of
// the slot per wavefront, a lane owning 16-byte units of the slot. A block decoded in its entry has no copy.
extern "C" __global__ void __launch_bounds__(256)
zxc_takev_copy_kernel(const uint8_t* __restrict__ carry0, const uint8_t* __restrict__ carry1, const uint8_t* __restrict__ slots,
                      uint32_t slot_stride, ztv_chunk_t c, const int32_t* __restrict__ status, uint32_t n_jobs,
                      const zc_ctl_t* __restrict__ ctl, const zav_ctl_t* __restrict__ vctl, uint32_t chunks,
                      const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, uint32_t n_iov,
                      const ztv_place_t* __restrict__ places) {
    if (vctl->status < 0 || ctl->final) return;
    const uint32_t lane = threadIdx.x & 63u, found = ctl->found;
    const int32_t* st = status + (uint64_t)ctl->sel * n_jobs;
    const uint64_t units = ((uint64_t)c.c.nb + 1u) * chunks, waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < units; it += waves) {
        const uint32_t k = (uint32_t)(it / chunks), ch = (uint32_t)(it - (uint64_t)k * chunks);
        const zt_copy_t cp = zt_copy(&c.c, k);
        if (cp.kind == ZT_NONE || cp.block >= found) continue;
        const ztv_place_t* rec = k ? places + (k - 1u) : NULL;
        if (rec && rec->kind != cp.kind) continue;  // decoded in its entry
        const uint32_t n = zt_copy_bytes(&cp, st[cp.block], c.c.block_size);
        if (n == 0 || (uint64_t)ch * ZT_COPY_CHUNK >= (uint64_t)n + 15u) continue;
        const ztv_copy_t o = ztv_copy_place(&c, &cp, n, rec, iov, starts, n_iov);
        const uint8_t* s = (cp.kind == ZT_SLOT ? slots + (uint64_t)cp.slot * slot_stride : cp.slot ? carry1 : carry0) + cp.from;
        if (o.one) {
            uint8_t* d = (uint8_t*)(uintptr_t)o.d;
            if ((uint64_t)ch * ZT_COPY_CHUNK < ((uintptr_t)d & 15u) + n) zd_copy_chunk(d, s, (int64_t)n, ch, lane);
            continue;
        }
        ztv_scatter_lane(s, n, o.y, ch, lane, iov, starts, o.e_lo, n_iov);
    }
}

// ---------------------------------------------------------------- host side
namespace {

#define TAKE_LIVE 0x7a78632d74616b65ull  // a session between begin and end

// What zxc_dev_dtake_t holds: the arguments of begin and the bytes taken. The work area's layout follows from them.
struct Sess {
    uint64_t magic;
    const uint8_t* src;
    uint64_t src_size, dst_capacity, max_piece;
    uint8_t* base;  // the work area's aligned base
    uint64_t pos;   // bytes taken so far
    const void *d_dict, *d_huf;
    uint32_t dict_size, block_size, tables;
    uint32_t cur;   // which of the two carry slots holds block pos / block_size
};
static_assert(sizeof(Sess) <= sizeof(zxc_dev_dtake_t), "the session fits the caller's struct");

// A live session and its shape out of the caller's struct. -> false: never begun, ended, or spent by an error.
bool tk_load(const zxc_dev_dtake_t* ds, Sess* s, zt_shape_t* sh) {
    memcpy(s, ds, sizeof *s);
    return s->magic == TAKE_LIVE && zt_shape(s->dst_capacity, s->max_piece, s->block_size, sh) == 0;  // (begin accepted these)
}

// The parts of a session's work area: the container's, then what a chunk uses.
struct Work {
    zd_cwork_t c;
    zxc_dev_job_t* cjobs;  // the chunk's two tables of J jobs
    const uint8_t *carry[2], *slots;
};
Work tk_work(const Sess& s, const zt_shape_t& sh) {
    uint8_t* b = s.base;
    return Work{zd_cwork(b, sh), (zxc_dev_job_t*)(b + sh.o_cjobs), {b + sh.o_carry[0], b + sh.o_carry[1]}, b + sh.o_slots};
}

// The decode step of both front ends, behind their plan kernels: the chunk's tables into `out`, the statuses to the blocks' words
// of the session's status table.
int tk_tables(const Sess& s, const zt_shape_t& sh, const Work& w, const zt_chunk_t& c, const uint8_t* out, hipStream_t st) {
    const zd_dict_t dc = {s.d_dict, s.d_huf, NULL, s.dict_size};
    return zd_decode_tables(s.src, w.cjobs, sh.J, c.nb, (void*)out, w.c.status + c.first, sh.n_jobs, s.block_size, s.tables, dc, (void*)st);
}

// plan and decode of one chunk of a take: d = where its first byte goes (not touched when no block is decoded straight)
int tk_decode(const Sess& s, const zt_shape_t& sh, const Work& w, uint8_t* d, const zt_chunk_t& c, hipStream_t st) {
    if (!c.nb) return ZXC_OK;
    // One decode launch for the piece and the work area: job offsets are 64-bit and counted from d_out, so d_out is the lower of
    // the two; the piece's side is rounded down to 16, which keeps d_out and the out_off of every slot and of every block decoded
    // straight (whose place is 16-byte aligned) multiples of 16. (Not zd_out_base: the rounding, and a piece no block goes to.)
    const uint8_t* lo = (const uint8_t*)((uintptr_t)d & ~(uintptr_t)15u);
    const uint8_t* out = (c.n_direct && lo < w.carry[0]) ? lo : w.carry[0];
    const uint64_t dst_rel = c.n_direct ? (uint64_t)(d - out) : 0u;
    hipLaunchKernelGGL(zxc_take_plan_kernel, dim3((c.nb + 255u) / 256u), dim3(256), 0, st, (const zxc_dev_job_t*)w.c.jobs, sh.n_jobs, s.tables, c,
                       dst_rel, (uint64_t)(w.carry[0] - out), (uint64_t)(w.carry[1] - out), (uint64_t)(w.slots - out), sh.slot_stride, sh.J,
                       w.cjobs);
    if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
    return tk_tables(s, sh, w, c, out, st);
}

// One chunk of a take behind its plan: decode, then the copies.
int tk_chunk(const Sess& s, const zt_shape_t& sh, const Work& w, uint8_t* d, const zt_chunk_t& c, hipStream_t st) {
    const int rc = tk_decode(s, sh, w, d, c, st);
    if (rc != ZXC_OK) return rc;
    if (!c.head && c.nb == c.n_direct) return ZXC_OK;  // every byte lies in a block decoded straight
    hipLaunchKernelGGL(zxc_take_copy_kernel, zd_copy_grid(((uint64_t)c.nb + 1u) * sh.copy_chunks), dim3(256), 0, st, w.carry[0], w.carry[1],
                       w.slots, sh.slot_stride, c, (const int32_t*)w.c.status, sh.n_jobs, (const zc_ctl_t*)w.c.ctl, sh.copy_chunks, d);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

// The virtual destination of a takev (zxc_takev.h): the table, what the call's scan left in its scratch.
struct Vdst {
    const zxc_dev_iov_t* iov;
    uint32_t n_iov;
    const uint64_t* starts;
    const zav_ctl_t* vctl;
    ztv_place_t* places;
};

// One chunk of a takev behind its plan: plan, decode, copy. The decode launch's d_out is the work area's 256-byte aligned base;
// a job's out_off is its address minus that base modulo 2^64 (the entries may lie above or below the work area), which the decode
// kernels only ever add to d_out in 64 bits. Slots, carry slots and the places of blocks decoded in their entries are 16-byte
// aligned, so every out_off is a multiple of 16.
int tkv_chunk(const Sess& s, const zt_shape_t& sh, const Work& w, const Vdst& vd, const ztv_chunk_t& c, hipStream_t st) {
    const zc_ctl_t* ctl = w.c.ctl;
    if (c.c.nb) {
        hipLaunchKernelGGL(zxc_takev_plan_kernel, dim3((c.c.nb + 255u) / 256u), dim3(256), 0, st, (const zxc_dev_job_t*)w.c.jobs, sh.n_jobs, s.tables,
                           c, vd.iov, vd.starts, vd.n_iov, vd.vctl, ctl, (uint64_t)(uintptr_t)s.base, (uint64_t)(uintptr_t)w.carry[0],
                           (uint64_t)(uintptr_t)w.carry[1], (uint64_t)(uintptr_t)w.slots, sh.slot_stride, sh.J, w.cjobs, vd.places);
        if (!launched()) return ZXC_ERROR_GPU_UNAVAILABLE;
        const int rc = tk_tables(s, sh, w, c.c, s.base, st);
        if (rc != ZXC_OK) return rc;
    }
    hipLaunchKernelGGL(zxc_takev_copy_kernel, zd_copy_grid(((uint64_t)c.c.nb + 1u) * sh.copy_chunks), dim3(256), 0, st, w.carry[0], w.carry[1],
                       w.slots, sh.slot_stride, c, (const int32_t*)w.c.status, sh.n_jobs, ctl, vd.vctl, sh.copy_chunks, vd.iov, vd.starts, vd.n_iov,
                       (const ztv_place_t*)vd.places);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

// The next n bytes, to d or (vd != NULL) into the table of a takev, and the session back into *ds. rc: what the launches in front
// of the chunks gave; nothing more is enqueued behind an error, which spends the session (part of the call may be enqueued).
// Chunk by chunk: a chunk's table and slots are written and consumed in stream order before the next chunk overwrites them. Every
// chunk but the last ends on a block boundary of the archive. The 32 bytes a block decoded straight may store behind itself stay
// inside the call: a copy of the same or a later chunk fills them. v: the chunk's offset in the piece or in the entries' concatenation.
int tk_chunks(zxc_dev_dtake_t* ds, Sess& s, const zt_shape_t& sh, uint8_t* d, const Vdst* vd, uint64_t n, int rc, hipStream_t st) {
    const Work w = tk_work(s, sh);
    uint64_t left = n, v = 0;
    while (left && rc == ZXC_OK) {
        const uint64_t m = zt_chunk_len(s.pos, left, s.max_piece, s.block_size);
        ztv_chunk_t c;
        if (vd) {
            ztv_plan_chunk(s.pos, m, s.block_size, s.cur, v, &c);
            rc = tkv_chunk(s, sh, w, *vd, c, st);
        } else {
            zt_plan_chunk(s.pos, m, left, (uint32_t)((uintptr_t)(d + v) & 15u), s.block_size, s.cur, &c.c);
            rc = tk_chunk(s, sh, w, d + v, c.c, st);
        }
        zt_advance(&c.c, &s.pos, &s.cur);
        v += m; left -= m;
    }
    if (rc != ZXC_OK) s.magic = 0;
    memcpy(ds, &s, sizeof s);
    return rc;
}

// Both begins. dict == NULL: the one that takes no dictionary.
int tk_begin(zxc_dev_dtake_t* ds, const void* d_src, uint64_t src_size, uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size,
             const zxc_decompress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, void* stream) {
    if (!ds || !d_src || !d_work) return ZXC_ERROR_NULL_INPUT;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER) return ZXC_ERROR_SRC_TOO_SMALL;
    zt_shape_t sh;
    if (zt_shape(dst_capacity, max_piece, block_size, &sh) != 0) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (opts && opts->dict) return ZXC_ERROR_GPU_UNSUPPORTED;
    const int drc = dict_arg(&dict);
    if (drc != ZXC_OK) return drc;
    if (work_size < sh.bytes) return ZXC_ERROR_MEMORY;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;

    const uint32_t want_verify = (opts && opts->checksum_enabled) ? 1u : 0u;
    const zd_dict_t dc = zd_dict_of(dict);
    Sess s = {};
    s.src = (const uint8_t*)d_src; s.src_size = src_size; s.dst_capacity = dst_capacity; s.max_piece = max_piece;
    s.base = zd_work_base(d_work);
    s.d_dict = dc.content; s.d_huf = dc.huf; s.dict_size = dc.size;
    s.block_size = block_size; s.tables = 1u + want_verify;
    // The container stages of zxc_mi355x_decompress_device. k_direct = n_jobs: every entry's out_off is its block's place in one
    // destination, which no take reads (the chunk plan writes its own).
    const int rc = zd_container_stages(zd_cwork(s.base, sh), s.src, src_size, dst_capacity, block_size, want_verify, sh.n_jobs, dc.id,
                                       (hipStream_t)stream);
    if (rc != ZXC_OK) return rc;
    s.magic = TAKE_LIVE;
    memset(ds, 0, sizeof *ds);
    memcpy(ds, &s, sizeof s);
    return ZXC_OK;
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_decompress_take_device_work_size(uint64_t src_size, uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size) {
    zt_shape_t sh;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER || zt_shape(dst_capacity, max_piece, block_size, &sh) != 0) return 0u;
    return sh.bytes;
}

int zxc_mi355x_decompress_begin_device(zxc_dev_dtake_t* ds, const void* d_src, uint64_t src_size, uint64_t dst_capacity, uint64_t max_piece,
                                       uint32_t block_size, const zxc_decompress_opts_t* opts, void* d_work, uint64_t work_size,
                                       void* stream) {
    return tk_begin(ds, d_src, src_size, dst_capacity, max_piece, block_size, opts, NULL, d_work, work_size, stream);
}

int zxc_mi355x_decompress_begin_dict_device(zxc_dev_dtake_t* ds, const void* d_src, uint64_t src_size, uint64_t dst_capacity,
                                            uint64_t max_piece, uint32_t block_size, const zxc_decompress_opts_t* opts,
                                            const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, void* stream) {
    return tk_begin(ds, d_src, src_size, dst_capacity, max_piece, block_size, opts, dict, d_work, work_size, stream);
}

int zxc_mi355x_decompress_take_device(zxc_dev_dtake_t* ds, void* d_dst, uint64_t n, void* stream) {
    if (!ds || (n > 0 && !d_dst)) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    zt_shape_t sh;
    if (!tk_load(ds, &s, &sh)) return ZXC_ERROR_NULL_INPUT;
    if (n > s.dst_capacity - s.pos) return ZXC_ERROR_OVERFLOW;
    if (n == 0) return ZXC_OK;
    return tk_chunks(ds, s, sh, (uint8_t*)d_dst, NULL, n, ZXC_OK, (hipStream_t)stream);
}

uint64_t zxc_mi355x_decompress_takev_device_scratch_size(uint32_t n_iov, uint64_t max_piece, uint32_t block_size) {
    ztv_shape_t sh;
    return ztv_shape(n_iov, max_piece, block_size, &sh) == 0 ? sh.bytes : 0u;
}

int zxc_mi355x_decompress_takev_device(zxc_dev_dtake_t* ds, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_scratch,
                                       uint64_t scratch_size, void* stream) {
    if (!ds || !d_scratch || (n_iov > 0 && !d_iov)) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    zt_shape_t sh;
    if (!tk_load(ds, &s, &sh)) return ZXC_ERROR_NULL_INPUT;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_DST_TOO_SMALL;
    if (total > s.dst_capacity - s.pos) return ZXC_ERROR_OVERFLOW;
    ztv_shape_t vsh;
    if (ztv_shape(n_iov, s.max_piece, s.block_size, &vsh) != 0) return ZXC_ERROR_NULL_INPUT;  // (begin accepted these)
    if (scratch_size < vsh.bytes) return ZXC_ERROR_MEMORY;
    if (n_iov == 0) return ZXC_OK;
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* sb = zd_work_base(d_scratch);
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + vsh.o_starts);
    // The scan, once per call (appendv's, as it is; its fold goes to a zap_ctl_t in the scratch that nobody reads), and the fold of
    // the verdict into the session: the chunks read starts and the verdict in stream order.
    int rc = zd_iov_scan(d_iov, n_iov, total, vsh.n_tiles, (uint64_t*)(sb + vsh.o_tile_sum), (uint32_t*)(sb + vsh.o_tile_flags), starts, vctl,
                         (zap_ctl_t*)(sb + ZTV_SINK), st);
    if (rc == ZXC_OK) {
        hipLaunchKernelGGL(zxc_takev_fold_kernel, dim3(1), dim3(64), 0, st, vctl, (zc_ctl_t*)s.base);
        if (!launched()) rc = ZXC_ERROR_GPU_UNAVAILABLE;
    }
    const Vdst vd = {d_iov, n_iov, starts, vctl, (ztv_place_t*)(sb + vsh.o_places)};
    return tk_chunks(ds, s, sh, NULL, &vd, total, rc, st);
}

int zxc_mi355x_decompress_end_device(zxc_dev_dtake_t* ds, int64_t* d_result, void* stream) {
    if (!ds || !d_result) return ZXC_ERROR_NULL_INPUT;
    Sess s;
    zt_shape_t sh;
    if (!tk_load(ds, &s, &sh)) return ZXC_ERROR_NULL_INPUT;
    if (s.pos < s.dst_capacity) return ZXC_ERROR_DST_TOO_SMALL;  // the verdict needs every block's status: take the rest, end again
    memset(ds, 0, sizeof *ds);  // spent, whatever happens below
    const hipStream_t st = (hipStream_t)stream;
    const Work w = tk_work(s, sh);
    if (s.dst_capacity > 0) {  // the one job behind the capacity, between the session's two halves of zxc_mi355x_decompress_device
        zt_chunk_t c;
        zt_plan_extra(sh.n_jobs - 1u, s.block_size, s.cur, &c);
        const int rc = tk_decode(s, sh, w, NULL, c, st);
        if (rc != ZXC_OK) return rc;
    }
    return zd_verdict_stages(w.c, s.block_size, s.dst_capacity, d_result, st);
}

}  // extern "C"
