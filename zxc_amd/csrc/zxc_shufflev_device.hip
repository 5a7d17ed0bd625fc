// zxc_shufflev_device.hip — the byte-shuffle of a table of buffers, device to device (include/zxc_mi355x_shufflev.h): the
// gather-shuffle kernels, zxc_mi355x_shufflev_device, and the archive call zxc_mi355x_compress_shufflev_device, which is
// zxc_mi355x_compress_shuffle_device (zxc_shuffle_device.hip) with the concatenation X of the table's entries in place of d_src.
// The rules are the inline C of zxc_shufflev.h on top of zxc_shuffle.h and zxc_appendv.h, which the CPU tests run as well.
//
// The kernels are the shuffle kernel's lane plan with another element side. A lane owns groups of 16 elements (zsh_group): its
// 16 E element bytes X[v + elem_at, + 16 E) come from the entries, E runs of 16 bytes, each one 16-byte load at whatever
// alignment base + off has when it lies inside one entry and else put together in registers a byte at a time (zsv_fetch16);
// then zsh_regs_shuffle and E 16-byte stores to the planes, contiguous across the wavefront. A wavefront narrows the entry
// search once to the entries that meet its 8 KiB, on wave-uniform arguments (scalar loads of starts[]), and a lane keeps a
// cursor, so with large entries almost no group searches or loads the table. No LDS.
//
// In stream order:
//   shufflev            scan (zd_iov_scan: appendv's three kernels, as they are) | gather-shuffle -> d_dst | result -> *d_status
//   compress_shufflev   begin | scan | per chunk: gather-shuffle X[at, at + n) -> stage, append(stage) | end -> word of d_work |
//                       result: the table's error or the word -> *d_result
// After a table error the gather kernels leave at once: no entry is read, and nothing but the scratch is written.
#include "zxc_device_util.h"  // the scan, the host-side plumbing; the kernels' declarations (zxc_kernels.h)
#include "zxc_shufflev.h"

static_assert(sizeof(zap_ctl_t) <= ZSV_SINK, "the zap_ctl_t the scan folds into");

namespace {

__device__ __forceinline__ void st128(uint8_t* p, v4u v) { *(v4u_unaligned*)p = v; }

template <uint32_t E>
__device__ __forceinline__ void shufflev_body(const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, uint32_t n_iov,
                                              const zav_ctl_t* __restrict__ vctl, uint64_t v, uint8_t* __restrict__ dst, const zsh_plan_t& pl,
                                              uint64_t n) {
    if (vctl->status < 0) return;  // (the table's error: no entry is read, nothing is written)
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform, and known to be
    for (uint64_t w = (uint64_t)blockIdx.x * waves + wave_in_group; w < pl.waves; w += (uint64_t)gridDim.x * waves) {
        const zsv_span_t sp = zsv_wave_span(starts, n_iov, v, n, w);
        zav_cursor_t cur = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t turn = 0; turn < 8u / E; turn++) {
            zsh_group_t g;
            if (!zsh_group(&pl, w, turn, lane, &g)) continue;
            uint32_t e[4u * E], p[4u * E];
            zsv_fetch_group(e, E, v + g.elem_at, iov, starts, sp.e_lo, sp.e_hi, &cur);
            zsh_regs_shuffle(e, p, E);
#pragma unroll
            for (uint32_t k = 0; k < E; k++) {
                const v4u o = {p[4u * k], p[4u * k + 1u], p[4u * k + 2u], p[4u * k + 3u]};
                st128(dst + g.plane_at + (uint64_t)k * g.q, o);
            }
        }
        if (w == pl.waves - 1u) {  // the leftovers of the ragged last unit, a byte at a time through the same cursor
            for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                uint64_t plain, shuffled;
                zsh_ragged_byte(&pl, j, &plain, &shuffled);
                dst[shuffled] = zsv_fetch_byte(v + plain, iov, starts, sp.e_lo, sp.e_hi, &cur);
            }
        }
    }
}

}  // namespace

#define ZSV_KERNEL(name, E)                                                                                                          \
    extern "C" __global__ void __launch_bounds__(256) name(const zxc_dev_iov_t* __restrict__ iov, const uint64_t* __restrict__ starts, \
                                                           uint32_t n_iov, const zav_ctl_t* __restrict__ vctl, uint64_t v,            \
                                                           uint8_t* __restrict__ dst, zsh_plan_t pl, uint64_t n) {                    \
        shufflev_body<E>(iov, starts, n_iov, vctl, v, dst, pl, n);                                                                  \
    }
ZSV_KERNEL(zxc_shufflev2_kernel, 2u)
ZSV_KERNEL(zxc_shufflev4_kernel, 4u)
ZSV_KERNEL(zxc_shufflev8_kernel, 8u)

// *d_result, once, behind everything else of the call: the table's error, else the session's word (no word: 0; no table: no error).
extern "C" __global__ void zxc_shufflev_result_kernel(const zav_ctl_t* __restrict__ vctl, const int64_t* __restrict__ word,
                                                      int64_t* __restrict__ d_result) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *d_result = zsv_result(vctl ? vctl->status : 0, word ? *word : 0);
}

namespace {

// The table of a call behind its scan: what the gather launches read.
struct Table {
    const zxc_dev_iov_t* iov;
    uint32_t n_iov;
    const uint64_t* starts;
    const zav_ctl_t* vctl;
};

// The scan, once per call, into the scratch at d_scratch (any alignment; zsv_scratch_size(n_iov) bytes); n_iov > 0.
int sv_scan(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_scratch, hipStream_t st, Table* tb) {
    zav_shape_t s;
    zsv_shape(n_iov, &s);
    uint8_t* sb = zd_work_base(d_scratch);
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + s.o_starts);
    *tb = Table{d_iov, n_iov, starts, vctl};
    return zd_iov_scan(d_iov, n_iov, total, s.n_tiles, (uint64_t*)(sb + s.o_tile_sum), (uint32_t*)(sb + s.o_tile_flags), starts, vctl,
                       (zap_ctl_t*)(sb + s.o_images), st);
}

// One launch: d_dst[0, n) = the shuffle of X[v, v + n), n > 0, v a multiple of unit; elem_size and unit were checked.
int sv_launch(const Table& tb, uint64_t v, void* d_dst, uint64_t n, uint32_t E, uint32_t unit, hipStream_t st) {
    const zsh_plan_t pl = zsh_plan(n, E, unit);
    const dim3 grid = zd_copy_grid(pl.waves), block(256);
    const auto kernel = E == 2u ? zxc_shufflev2_kernel : E == 4u ? zxc_shufflev4_kernel : zxc_shufflev8_kernel;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, tb.iov, tb.starts, tb.n_iov, tb.vctl, v, (uint8_t*)d_dst, pl, n);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int sv_result(const zav_ctl_t* vctl, const int64_t* word, int64_t* d_result, hipStream_t st) {
    hipLaunchKernelGGL(zxc_shufflev_result_kernel, dim3(1), dim3(64), 0, st, vctl, word, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_shufflev_device_scratch_size(uint32_t n_iov) { return zsv_scratch_size(n_iov); }

int zxc_mi355x_shufflev_device(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_dst, uint32_t elem_size, uint32_t unit,
                               void* d_scratch, uint64_t scratch_size, int64_t* d_status, void* stream) {
    if ((n_iov > 0 && !d_iov) || (total > 0 && !d_dst) || !d_scratch || !d_status) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (!zsh_unit_ok(unit)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_SRC_TOO_SMALL;
    if (scratch_size < zsv_scratch_size(n_iov)) return ZXC_ERROR_MEMORY;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const hipStream_t st = (hipStream_t)stream;
    if (n_iov == 0) return sv_result(NULL, NULL, d_status, st);  // (nothing to move: the store alone)
    Table tb;
    int rc = sv_scan(d_iov, n_iov, total, d_scratch, st, &tb);
    if (rc == ZXC_OK && total > 0) rc = sv_launch(tb, 0u, d_dst, total, elem_size, unit, st);
    return rc == ZXC_OK ? sv_result(tb.vctl, NULL, d_status, st) : rc;
}

uint64_t zxc_mi355x_compress_shufflev_device_work_size(uint32_t n_iov, uint64_t total, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                       uint32_t dict_size) {
    return zsv_work_size(zxc_mi355x_compress_shuffle_device_work_size(total, max_piece, opts, dict_size), n_iov);
}

int zxc_mi355x_compress_shufflev_device(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, uint32_t elem_size, void* d_dst,
                                        uint64_t dst_capacity, uint64_t max_piece, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict,
                                        void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if ((n_iov > 0 && !d_iov) || !d_result) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_SRC_TOO_SMALL;
    zxc_dev_cappend_t cs;
    zd_copts_t o;
    uint64_t piece = 0, session = 0, shuffle_ws = 0;
    const uint32_t dict_size = (dict && dict->size <= ZC_DICT_MAX) ? dict->size : 0u;
    if (zd_compress_opts(opts, &o) == ZXC_OK && (max_piece == 0 || max_piece >= o.block_size)) {
        piece = zsh_piece(total, max_piece, o.block_size);
        session = zxc_mi355x_compress_append_dict_device_work_size(total, piece, opts, dict_size);
        shuffle_ws = session ? session + ZSH_STAGE_ALIGN + piece : 0u;  // (zxc_mi355x_compress_shuffle_device_work_size)
    }
    // As in the sibling: without a chunk or a session size, begin is given the arguments as they are and refuses them at their
    // place in its order; with them, its own part of the work area when the whole fits and none when it does not (ZXC_ERROR_MEMORY).
    const uint64_t given = session ? (work_size >= zsv_work_size(shuffle_ws, n_iov) ? session : 0u) : work_size;
    int rc = zxc_mi355x_compress_begin_dict_device(&cs, d_dst, dst_capacity, total, session ? piece : max_piece, opts, dict, d_work, given, stream);
    if (rc != ZXC_OK) return rc;
    if (!session) return ZXC_ERROR_BAD_BLOCK_SIZE;  // (unreachable: begin refuses what the size functions refuse)
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* stage = (uint8_t*)zc_round_up((uint64_t)(uintptr_t)d_work + session, ZSH_STAGE_ALIGN);
    uint8_t* scratch = (uint8_t*)d_work + zc_round_up(shuffle_ws, 256u);
    zav_shape_t vs;
    zsv_shape(n_iov, &vs);
    // the session's result word: behind the scratch's sink, counted from the scratch's aligned base, inside the last 256 bytes
    int64_t* word = (int64_t*)(zd_work_base(scratch) + vs.o_images + ZSV_SINK);
    Table tb = {d_iov, n_iov, NULL, NULL};
    if (n_iov > 0) rc = sv_scan(d_iov, n_iov, total, scratch, st, &tb);
    for (uint64_t at = 0; at < total && rc == ZXC_OK; at += piece) {
        const uint64_t n = total - at < piece ? total - at : piece;
        rc = sv_launch(tb, at, stage, n, elem_size, o.block_size, st);
        if (rc == ZXC_OK) rc = zxc_mi355x_compress_append_device(&cs, stage, n, stream);
    }
    if (rc == ZXC_OK) rc = zxc_mi355x_compress_end_device(&cs, word, stream);
    return rc == ZXC_OK ? sv_result(tb.vctl, word, d_result, st) : rc;
}

}  // extern "C"
