// zxc_shuffle_device.hip — the byte-shuffle pre-filter, device to device (include/zxc_mi355x_shuffle.h): the two transposition
// kernels, zxc_mi355x_shuffle_device / _unshuffle_device, and the archive calls zxc_mi355x_compress_shuffle_device /
// _decompress_shuffle_device, which run the kernels chunk by chunk in front of an append session (zxc_append_device.hip) and behind
// a take session (zxc_take_device.hip). The rules are the inline C of zxc_shuffle.h, which the CPU tests run as well: the index
// map, which 16-byte groups a lane owns, where each byte goes inside the lane's registers, and where the byte-wise leftovers begin.
//
// The kernels are data movement alone. A lane owns groups of 16 elements: E 16-byte accesses to 16 E contiguous bytes on the element
// side, one 16-byte access to each of the E planes, contiguous across the wavefront, and between them v_perm_b32 in registers (8
// per 4 x 4 bytes). One wavefront per 8 KiB whatever E is. Every group access is 16 bytes wide at the alignment the caller's
// pointers give it (global memory takes a 16-byte access at any address, as copy_bytes of zxc_wave.h relies on); only the last
// unit's leftovers, at most 127 bytes, move a byte at a time.
//
// The archive calls enqueue, in stream order:
//   compress     begin | per chunk: shuffle d_src -> stage, append(stage) | end -> *d_result
//   decompress   begin | per chunk: take(stage), un-shuffle stage -> d_dst | end -> word of d_work | fix: word -> *d_result
// The stage is one area of d_work behind the session's, reused from chunk to chunk: a kernel that writes it is enqueued behind the
// launches that read its previous contents.
#include "zxc_device_util.h"  // ld128, the host-side plumbing
#include "zxc_shuffle.h"

namespace {

__device__ __forceinline__ void st128(uint8_t* p, v4u v) { *(v4u_unaligned*)p = v; }

// INV false: element side of src -> planes of dst. INV true: planes of src -> element side of dst.
template <uint32_t E, bool INV>
__device__ __forceinline__ void shuffle_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const zsh_plan_t& pl) {
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    for (uint64_t w = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); w < pl.waves; w += (uint64_t)gridDim.x * waves) {
#pragma unroll
        for (uint32_t turn = 0; turn < 8u / E; turn++) {
            zsh_group_t g;
            if (!zsh_group(&pl, w, turn, lane, &g)) continue;
            uint32_t e[4u * E], p[4u * E];
            if (!INV) {
#pragma unroll
                for (uint32_t j = 0; j < E; j++) {
                    const v4u v = ld128(src + g.elem_at + 16u * j);
                    e[4u * j] = v.x; e[4u * j + 1u] = v.y; e[4u * j + 2u] = v.z; e[4u * j + 3u] = v.w;
                }
                zsh_regs_shuffle(e, p, E);
#pragma unroll
                for (uint32_t k = 0; k < E; k++) {
                    const v4u v = {p[4u * k], p[4u * k + 1u], p[4u * k + 2u], p[4u * k + 3u]};
                    st128(dst + g.plane_at + (uint64_t)k * g.q, v);
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < E; k++) {
                    const v4u v = ld128(src + g.plane_at + (uint64_t)k * g.q);
                    p[4u * k] = v.x; p[4u * k + 1u] = v.y; p[4u * k + 2u] = v.z; p[4u * k + 3u] = v.w;
                }
                zsh_regs_unshuffle(p, e, E);
#pragma unroll
                for (uint32_t j = 0; j < E; j++) {
                    const v4u v = {e[4u * j], e[4u * j + 1u], e[4u * j + 2u], e[4u * j + 3u]};
                    st128(dst + g.elem_at + 16u * j, v);
                }
            }
        }
        if (w == pl.waves - 1u) {  // the leftovers of the ragged last unit, a byte at a time
            for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                uint64_t plain, shuffled;
                zsh_ragged_byte(&pl, j, &plain, &shuffled);
                if (!INV) dst[shuffled] = src[plain];
                else dst[plain] = src[shuffled];
            }
        }
    }
}

}  // namespace

#define ZSH_KERNEL(name, E, INV)                                                                                                  \
    extern "C" __global__ void __launch_bounds__(256) name(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, zsh_plan_t pl) { \
        shuffle_body<E, INV>(src, dst, pl);                                                                                       \
    }
ZSH_KERNEL(zxc_shuffle2_kernel, 2u, false)
ZSH_KERNEL(zxc_shuffle4_kernel, 4u, false)
ZSH_KERNEL(zxc_shuffle8_kernel, 8u, false)
ZSH_KERNEL(zxc_unshuffle2_kernel, 2u, true)
ZSH_KERNEL(zxc_unshuffle4_kernel, 4u, true)
ZSH_KERNEL(zxc_unshuffle8_kernel, 8u, true)

// *d_result, once, behind the take session's end: its word as it is, except that a decoded size other than the one the caller
// planned with is not the archive the caller described. dst_size == 0: the empty-frame probe's answer as it is.
extern "C" __global__ void zxc_unshuffle_result_kernel(const int64_t* __restrict__ word, uint64_t dst_size, int64_t* __restrict__ d_result) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t r = *word;
    if (dst_size > 0 && r >= 0 && (uint64_t)r != dst_size) r = ZXC_ERROR_CORRUPT_DATA;
    *d_result = r;
}

namespace {

// One launch over n > 0 bytes; elem_size and unit were checked.
int sh_launch(const void* d_src, void* d_dst, uint64_t n, uint32_t E, uint32_t unit, bool inverse, hipStream_t st) {
    const zsh_plan_t pl = zsh_plan(n, E, unit);
    const dim3 grid = zd_copy_grid(pl.waves), block(256);
    const uint8_t* s = (const uint8_t*)d_src;
    uint8_t* d = (uint8_t*)d_dst;
    if (E == 2u) {
        if (inverse) hipLaunchKernelGGL(zxc_unshuffle2_kernel, grid, block, 0, st, s, d, pl);
        else hipLaunchKernelGGL(zxc_shuffle2_kernel, grid, block, 0, st, s, d, pl);
    } else if (E == 4u) {
        if (inverse) hipLaunchKernelGGL(zxc_unshuffle4_kernel, grid, block, 0, st, s, d, pl);
        else hipLaunchKernelGGL(zxc_shuffle4_kernel, grid, block, 0, st, s, d, pl);
    } else {
        if (inverse) hipLaunchKernelGGL(zxc_unshuffle8_kernel, grid, block, 0, st, s, d, pl);
        else hipLaunchKernelGGL(zxc_shuffle8_kernel, grid, block, 0, st, s, d, pl);
    }
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

int sh_call(const void* d_src, void* d_dst, uint64_t n, uint32_t elem_size, uint32_t unit, bool inverse, void* stream) {
    if (n > 0 && (!d_src || !d_dst)) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    if (!zsh_unit_ok(unit)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    if (n == 0) return ZXC_OK;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    return sh_launch(d_src, d_dst, n, elem_size, unit, inverse, (hipStream_t)stream);
}

// The chunk of an archive call: -> 1 and *piece when block size and max_piece allow one, else 0 (the session's begin then refuses
// the same arguments at their place in its order of errors).
int sh_piece(uint64_t total, uint64_t max_piece, uint64_t block_size, uint64_t* piece) {
    if (!zc_block_size_ok(block_size) || (max_piece > 0 && max_piece < block_size)) return 0;
    *piece = zsh_piece(total, max_piece, (uint32_t)block_size);
    return 1;
}
uint8_t* sh_behind(void* d_work, uint64_t session_bytes) { return (uint8_t*)zc_round_up((uint64_t)(uintptr_t)d_work + session_bytes, ZSH_STAGE_ALIGN); }

}  // namespace

extern "C" {

int zxc_mi355x_shuffle_device(const void* d_src, void* d_dst, uint64_t n, uint32_t elem_size, uint32_t unit, void* stream) {
    return sh_call(d_src, d_dst, n, elem_size, unit, false, stream);
}

int zxc_mi355x_unshuffle_device(const void* d_src, void* d_dst, uint64_t n, uint32_t elem_size, uint32_t unit, void* stream) {
    return sh_call(d_src, d_dst, n, elem_size, unit, true, stream);
}

uint64_t zxc_mi355x_compress_shuffle_device_work_size(uint64_t src_size, uint64_t max_piece, const zxc_compress_opts_t* opts,
                                                      uint32_t dict_size) {
    zd_copts_t o;
    uint64_t piece;
    if (zd_compress_opts(opts, &o) != ZXC_OK || !sh_piece(src_size, max_piece, o.block_size, &piece)) return 0u;
    const uint64_t session = zxc_mi355x_compress_append_dict_device_work_size(src_size, piece, opts, dict_size);
    return session ? session + ZSH_STAGE_ALIGN + piece : 0u;
}

int zxc_mi355x_compress_shuffle_device(const void* d_src, uint64_t src_size, uint32_t elem_size, void* d_dst, uint64_t dst_capacity,
                                       uint64_t max_piece, const zxc_compress_opts_t* opts, const zxc_dev_dict_t* dict, void* d_work,
                                       uint64_t work_size, int64_t* d_result, void* stream) {
    if ((src_size > 0 && !d_src) || !d_result) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    zxc_dev_cappend_t cs;
    zd_copts_t o;
    uint64_t piece = 0, session = 0;
    if (zd_compress_opts(opts, &o) == ZXC_OK && sh_piece(src_size, max_piece, o.block_size, &piece))
        session = zxc_mi355x_compress_append_dict_device_work_size(src_size, piece, opts, (dict && dict->size <= ZC_DICT_MAX) ? dict->size : 0u);
    // Without a chunk or a session size, begin is given the arguments as they are and refuses them at their place in its order;
    // with them, it is given its own part of the work area when the whole fits and none when it does not (ZXC_ERROR_MEMORY).
    const uint64_t given = session ? (work_size >= session + ZSH_STAGE_ALIGN + piece ? session : 0u) : work_size;
    int rc = zxc_mi355x_compress_begin_dict_device(&cs, d_dst, dst_capacity, src_size, session ? piece : max_piece, opts, dict, d_work, given, stream);
    if (rc != ZXC_OK) return rc;
    if (!session) return ZXC_ERROR_BAD_BLOCK_SIZE;  // (unreachable: begin refuses what the size functions refuse)
    uint8_t* stage = sh_behind(d_work, session);
    for (uint64_t at = 0; at < src_size && rc == ZXC_OK; at += piece) {
        const uint64_t n = src_size - at < piece ? src_size - at : piece;
        rc = sh_launch((const uint8_t*)d_src + at, stage, n, elem_size, o.block_size, false, (hipStream_t)stream);
        if (rc == ZXC_OK) rc = zxc_mi355x_compress_append_device(&cs, stage, n, stream);
    }
    return rc == ZXC_OK ? zxc_mi355x_compress_end_device(&cs, d_result, stream) : rc;
}

uint64_t zxc_mi355x_decompress_shuffle_device_work_size(uint64_t src_size, uint64_t dst_size, uint64_t max_piece, uint32_t block_size) {
    uint64_t piece;
    if (!sh_piece(dst_size, max_piece, block_size, &piece)) return 0u;
    const uint64_t session = zxc_mi355x_decompress_take_device_work_size(src_size, dst_size, piece, block_size);
    return session ? session + 2u * ZSH_STAGE_ALIGN + piece : 0u;
}

int zxc_mi355x_decompress_shuffle_device(const void* d_src, uint64_t src_size, void* d_dst, uint64_t dst_size, uint32_t elem_size,
                                         uint64_t max_piece, uint32_t block_size, const zxc_decompress_opts_t* opts,
                                         const zxc_dev_dict_t* dict, void* d_work, uint64_t work_size, int64_t* d_result, void* stream) {
    if ((dst_size > 0 && !d_dst) || !d_result) return ZXC_ERROR_NULL_INPUT;
    if (!zsh_elem_ok(elem_size)) return ZXC_ERROR_GPU_UNSUPPORTED;
    zxc_dev_dtake_t ds;
    uint64_t piece = 0, session = 0;
    if (sh_piece(dst_size, max_piece, block_size, &piece)) session = zxc_mi355x_decompress_take_device_work_size(src_size, dst_size, piece, block_size);
    const uint64_t given = session ? (work_size >= session + 2u * ZSH_STAGE_ALIGN + piece ? session : 0u) : work_size;  // (as in the compress call)
    int rc = zxc_mi355x_decompress_begin_dict_device(&ds, d_src, src_size, dst_size, session ? piece : max_piece, block_size, opts, dict, d_work,
                                                     given, stream);
    if (rc != ZXC_OK) return rc;
    if (!session) return ZXC_ERROR_BAD_BLOCK_SIZE;  // (unreachable: begin refuses what the size functions refuse)
    int64_t* word = (int64_t*)sh_behind(d_work, session);
    uint8_t* stage = (uint8_t*)word + ZSH_STAGE_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    for (uint64_t at = 0; at < dst_size && rc == ZXC_OK; at += piece) {
        const uint64_t n = dst_size - at < piece ? dst_size - at : piece;
        rc = zxc_mi355x_decompress_take_device(&ds, stage, n, stream);
        if (rc == ZXC_OK) rc = sh_launch(stage, (uint8_t*)d_dst + at, n, elem_size, block_size, true, st);
    }
    if (rc == ZXC_OK) rc = zxc_mi355x_decompress_end_device(&ds, word, stream);
    if (rc != ZXC_OK) return rc;
    hipLaunchKernelGGL(zxc_unshuffle_result_kernel, dim3(1), dim3(64), 0, st, (const int64_t*)word, dst_size, d_result);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}

}  // extern "C"
