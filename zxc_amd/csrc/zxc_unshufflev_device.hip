// zxc_unshufflev_device.hip — the inverse byte-shuffle into a table of buffers, device to device
// (include/zxc_mi355x_unshufflev.h): the scatter-un-shuffle kernels, zxc_mi355x_unshufflev_device, and the archive call
// zxc_mi355x_decompress_shufflev_device, which is zxc_mi355x_decompress_shuffle_device (zxc_shuffle_device.hip) with the
// concatenation Y of the table's entries in place of d_dst. The rules are the inline C of zxc_unshufflev.h on top of
// zxc_shufflev.h, zxc_shuffle.h and zxc_takev.h, which the CPU tests run as well.
//
// The kernels are the gather-shuffle kernels (zxc_shufflev_device.hip) run backwards. A lane owns groups of 16 elements
// (zsh_group): E 16-byte loads from the planes of the contiguous source, contiguous across the wavefront, zsh_regs_unshuffle, and
// the group's 16 E element bytes go to Y[v + elem_at, + 16 E) as E runs of 16 bytes: E stores back to back when the group lies
// inside one entry, else run by run, each one 16-byte store at whatever alignment base + off has when it lies inside one entry
// and else a byte at a time into consecutive entries (zuv_store_group, zuv_store16). A wavefront
// narrows the entry search once to the entries that meet its 8 KiB, on wave-uniform arguments (scalar loads of starts[]), and a
// lane keeps a cursor, so with large entries almost no group searches or loads the table. No LDS.
//
// In stream order:
//   unshufflev            scan (zd_iov_scan: appendv's three kernels, as they are) | scatter-un-shuffle d_src -> Y | result -> *d_status
//   decompress_shufflev   begin | scan | per chunk: take(stage), scatter-un-shuffle stage -> Y[at, at + n) | end -> word of d_work |
//                         result: the table's error, or the word with its size check -> *d_result
// After a table error the scatter kernels leave at once: no byte of any entry is written.
#include "zxc_device_util.h"  // ld128, the scan, the host-side plumbing; the kernels' declarations (zxc_kernels.h)
#include "zxc_unshufflev.h"

static_assert(sizeof(zap_ctl_t) <= ZSV_SINK, "the zap_ctl_t the scan folds into");

namespace {

template <uint32_t E>
__device__ __forceinline__ void unshufflev_body(const uint8_t* __restrict__ src, const zxc_dev_iov_t* __restrict__ iov,
                                                const uint64_t* __restrict__ starts, uint32_t n_iov, const zav_ctl_t* __restrict__ vctl,
                                                uint64_t v, const zsh_plan_t& pl, uint64_t n) {
    if (vctl->status < 0) return;  // (the table's error: no entry is looked at, nothing is written)
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
#pragma unroll
            for (uint32_t k = 0; k < E; k++) {
                const v4u o = ld128(src + g.plane_at + (uint64_t)k * g.q);
                p[4u * k] = o.x; p[4u * k + 1u] = o.y; p[4u * k + 2u] = o.z; p[4u * k + 3u] = o.w;
            }
            zsh_regs_unshuffle(p, e, E);
            zuv_store_group(e, E, v + g.elem_at, iov, starts, sp.e_lo, sp.e_hi, &cur);
        }
        if (w == pl.waves - 1u) {  // the leftovers of the ragged last unit, a byte at a time through the same cursor
            for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                uint64_t plain, shuffled;
                zsh_ragged_byte(&pl, j, &plain, &shuffled);
                zuv_store_byte(v + plain, src[shuffled], iov, starts, sp.e_lo, sp.e_hi, &cur);
            }
        }
    }
}

}  // namespace

#define ZUV_KERNEL(name, E)                                                                                                           \
    extern "C" __global__ void __launch_bounds__(256) name(const uint8_t* __restrict__ src, const zxc_dev_iov_t* __restrict__ iov,    \
                                                           const uint64_t* __restrict__ starts, uint32_t n_iov,                      \
                                                           const zav_ctl_t* __restrict__ vctl, uint64_t v, zsh_plan_t pl, uint64_t n) { \
        unshufflev_body<E>(src, iov, starts, n_iov, vctl, v, pl, n);                                                                 \
    }
ZUV_KERNEL(zxc_unshufflev2_kernel, 2u)
ZUV_KERNEL(zxc_unshufflev4_kernel, 4u)
ZUV_KERNEL(zxc_unshufflev8_kernel, 8u)

// *d_result, once, behind everything else of the call: zuv_result of the table's status and the session's word (no word: 0; no
// table: no error). zxc_shufflev_result_kernel is not reused: its callers get the scan's status as it is, this direction reads
// it through takev's verdict and checks the decoded size.
extern "C" __global__ void zxc_unshufflev_result_kernel(const zav_ctl_t* __restrict__ vctl, const int64_t* __restrict__ word, uint64_t total,
                                                        int64_t* __restrict__ d_result) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    *d_result = zuv_result(vctl ? vctl->status : 0, word ? *word : 0, total);
}

namespace {

// The table of a call behind its scan: what the scatter launches read.
struct Table {
    const zxc_dev_iov_t* iov;
    uint32_t n_iov;
    const uint64_t* starts;
    const zav_ctl_t* vctl;
};

// The scan, once per call, into the scratch at d_scratch (any alignment; zsv_scratch_size(n_iov) bytes); n_iov > 0.
int uv_scan(const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, void* d_scratch, hipStream_t st, Table* tb) {
    zav_shape_t s;
    zsv_shape(n_iov, &s);
    uint8_t* sb = zd_work_base(d_scratch);
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + s.o_starts);
    *tb = Table{d_iov, n_iov, starts, vctl};
    return zd_iov_scan(d_iov, n_iov, total, s.n_tiles, (uint64_t*)(sb + s.o_tile_sum), (uint32_t*)(sb + s.o_tile_flags), starts, vctl,
                       (zap_ctl_t*)(sb + s.o_images), st);
}

// One launch: Y[v, v + n) = the un-shuffle of d_src[0, n), n > 0, v a multiple of unit; elem_size and unit were checked.
int uv_launch(const void* d_src, const Table& tb, uint64_t v, uint64_t n, uint32_t E, uint32_t unit, hipStream_t st) {
    const zsh_plan_t pl = zsh_plan(n, E, unit);
    const dim3 grid = zd_copy_grid(pl.waves), block(256);
    const auto kernel = E == 2u ? zxc_unshufflev2_kernel : E == 4u ? zxc_unshufflev4_kernel : zxc_unshufflev8_kernel;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, (const uint8_t*)d_src, tb.iov, tb.starts, tb.n_iov, tb.vctl, v, pl, n);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int uv_result(const zav_ctl_t* vctl, const int64_t* word, uint64_t total, int64_t* d_result, hipStream_t st) {
    hipLaunchKernelGGL(zxc_unshufflev_result_kernel, dim3(1), dim3(64), 0, st, vctl, word, total, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // namespace

extern "C" {

uint64_t zxc_mi355x_unshufflev_device_scratch_size(uint32_t n_iov) { return zsv_scratch_size(n_iov); }

int zxc_mi355x_unshufflev_device(const void* d_src, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total, uint32_t elem_size,
                                 uint32_t unit, void* d_scratch, uint64_t scratch_size, int64_t* d_status, void* stream) {
    if ((n_iov > 0 && !d_iov) || (total > 0 && !d_src) || !d_scratch || !d_status) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (!zsh_unit_ok(unit)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_DST_TOO_SMALL;
    if (scratch_size < zsv_scratch_size(n_iov)) return ZXC_ERROR_MEMORY;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    const hipStream_t st = (hipStream_t)stream;
    if (n_iov == 0) return uv_result(NULL, NULL, 0u, d_status, st);  // (nothing to move: the store alone)
    Table tb;
    int rc = uv_scan(d_iov, n_iov, total, d_scratch, st, &tb);
    if (rc == ZXC_OK && total > 0) rc = uv_launch(d_src, tb, 0u, total, elem_size, unit, st);
    return rc == ZXC_OK ? uv_result(tb.vctl, NULL, 0u, d_status, st) : rc;
}

uint64_t zxc_mi355x_decompress_shufflev_device_work_size(uint32_t n_iov, uint64_t src_size, uint64_t total, uint64_t max_piece,
                                                         uint32_t block_size) {
    return zuv_work_size(zxc_mi355x_decompress_shuffle_device_work_size(src_size, total, max_piece, block_size), n_iov);
}

int zxc_mi355x_decompress_shufflev_device(const void* d_src, uint64_t src_size, const zxc_dev_iov_t* d_iov, uint32_t n_iov, uint64_t total,
                                          uint32_t elem_size, uint64_t max_piece, uint32_t block_size, const zxc_decompress_opts_t* opts,
                                          const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if ((n_iov > 0 && !d_iov) || !d_result) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (n_iov == 0 && total > 0) return ZXC_ERROR_DST_TOO_SMALL;
    zxc_dev_dtake_t ds;
    uint64_t piece = 0, session = 0, shuffle_ws = 0;
    if (zc_block_size_ok(block_size) && (max_piece == 0 || max_piece >= block_size)) {
        piece = zsh_piece(total, max_piece, block_size);
        session = zxc_mi355x_decompress_take_device_work_size(src_size, total, piece, block_size);
        shuffle_ws = session ? session + 2u * ZSH_STAGE_ALIGN + piece : 0u;  // (zxc_mi355x_decompress_shuffle_device_work_size)
    }
    // As in the sibling: without a chunk or a session size, begin is given the arguments as they are and refuses them at their
    // place in its order; with them, its own part of the work area when the whole fits and none when it does not (ZXC_ERROR_MEMORY).
    const uint64_t given = session ? (work_size >= zuv_work_size(shuffle_ws, n_iov) ? session : 0u) : work_size;
    int rc = zxc_mi355x_decompress_begin_dict_device(&ds, d_src, src_size, total, session ? piece : max_piece, block_size, opts, dict, d_work,
                                                     given, stream);
    if (rc != ZXC_OK) return rc;
    if (!session) return ZXC_ERROR_BAD_BLOCK_SIZE;  // (unreachable: begin refuses what the size functions refuse)
    const hipStream_t st = (hipStream_t)stream;
    int64_t* word = (int64_t*)zc_round_up((uint64_t)(uintptr_t)d_work + session, ZSH_STAGE_ALIGN);  // (the sibling's layout)
    uint8_t* stage = (uint8_t*)word + ZSH_STAGE_ALIGN;
    uint8_t* scratch = (uint8_t*)d_work + zc_round_up(shuffle_ws, 256u);
    Table tb = {d_iov, n_iov, NULL, NULL};
    if (n_iov > 0) rc = uv_scan(d_iov, n_iov, total, scratch, st, &tb);
    for (uint64_t at = 0; at < total && rc == ZXC_OK; at += piece) {
        const uint64_t n = total - at < piece ? total - at : piece;
        rc = zxc_mi355x_decompress_take_device(&ds, stage, n, stream);
        if (rc == ZXC_OK) rc = uv_launch(stage, tb, at, n, elem_size, block_size, st);
    }
    if (rc == ZXC_OK) rc = zxc_mi355x_decompress_end_device(&ds, word, stream);
    return rc == ZXC_OK ? uv_result(tb.vctl, word, total, d_result, st) : rc;
}

}  // extern "C"
