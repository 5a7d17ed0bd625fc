/* zxc_shufflev.h — the rules of the byte-shuffle of a table of buffers (include/zxc_mi355x_shufflev.h, kernels and calls in
 * zxc_shufflev_device.hip) on top of zxc_shuffle.h and zxc_appendv.h: the scratch of the table scan, the entries a wavefront's
 * element side meets, and the fetch of a group's element bytes from the entries. Plain inline C that hipcc and a host C compiler
 * both take, so that the kernels and the CPU tests (tests/shuffle/shufflev_replay.h) run the same lines.
 *
 * The source is zxc_appendv.h's virtual one: X, the concatenation of the table's entries, total bytes; starts[r] is the offset of
 * entry r in X. A chunk is X[v, v + n) with v a multiple of the unit, so its units are X's and zsh_plan(n, E, unit) over it hands
 * out the groups zsh_plan over all of X would: which wavefront, turn and lane owns a group, where its planes go and what the last
 * wavefront moves a byte at a time are zxc_shuffle.h's, unchanged. Only the element side differs: group G's 16 E bytes are
 * X[v + 16 E G, + 16 E), read as E runs of 16 bytes. A run inside one entry is one 16-byte load at whatever alignment base + off
 * has; a run that crosses an entry boundary is put together in registers a byte at a time from consecutive entries, past empty
 * ones, whose base is not looked at. Exactly the bytes of the entries are read: nothing is promised readable behind an entry.
 *
 * The search. A wavefront narrows the entries once to those that meet its 8 KiB (zsv_wave_span: zav_find on wave-uniform
 * arguments), and every lane keeps a zav_cursor_t, the entry its last run ended in: a run that starts in that entry again needs no
 * search and no load of the table, which is every run but a few when the entries are large.
 *
 * Scratch of the scan, from its 256-byte aligned base: zav_shape_dict's shape with a dictionary, that is the control word,
 * starts[0 .. n_iov] and the tile words and no images, and behind it 256 bytes for the zap_ctl_t the scan folds into, which nobody
 * reads. With t = ceil(n_iov / 1024) and up256 rounding up to a multiple of 256 the size is
 *     768 + up256(8 x (n_iov + 1)) + up256(8 t) + up256(4 t)   <=   8 x (n_iov + 1) + 16 t + 4096 + 256. */
#ifndef ZXC_SHUFFLEV_H
#define ZXC_SHUFFLEV_H
#include "../../include/zxc_mi355x_shufflev.h"
#include "zxc_appendv.h"
#include "zxc_shuffle.h"

#ifdef __HIPCC__
#define ZSV_UNROLL _Pragma("unroll")
#else
#define ZSV_UNROLL
#endif

/* an entry's bytes: its base is an address in device memory (a global load in the kernels, not a flat one) */
#ifdef __HIP_DEVICE_COMPILE__
#define ZSV_ENTRY const __attribute__((address_space(1))) uint8_t*
#else
#define ZSV_ENTRY const uint8_t*
#endif

#define ZSV_SINK 256u /* behind the shape: the unread zap_ctl_t; in the archive call's work area the session's result word follows */

/* ---- the scratch: the shape zav_shape_dict gives any session with a dictionary (the block and piece sizes only size images) */
ZC_FN void zsv_shape(uint32_t n_iov, zav_shape_t* s) { (void)zav_shape_dict(n_iov, 4096u, 4096u, 1u, s); }
ZC_FN uint64_t zsv_scratch_size(uint32_t n_iov) {
    zav_shape_t s;
    zsv_shape(n_iov, &s);
    return s.bytes + ZSV_SINK;
}
/* the closed form the header states */
ZC_FN uint64_t zsv_scratch_bound(uint32_t n_iov) { return zav_scratch_bound_dict(n_iov, 4096u, 4096u, 1u) + ZSV_SINK; }

/* The work area of the archive call: [session | stage] are the sibling's `shuffle_ws` bytes (zxc_mi355x_compress_shuffle_device_
 * work_size), the table scratch starts on the next multiple of 256 counted from d_work, and 256 bytes for the session's result
 * word follow. 0 when the sibling gives 0. */
ZC_FN uint64_t zsv_work_size(uint64_t shuffle_ws, uint32_t n_iov) {
    return shuffle_ws ? zc_round_up(shuffle_ws, 256u) + zsv_scratch_size(n_iov) + 256u : 0u;
}

/* ---- the entries [e_lo, e_hi] that hold the element side of wavefront `wave` of the chunk X[v, v + n): X[v + 8 KiB wave, ...)
 * up to the chunk's end. For a valid table (starts[n_iov] = total >= v + n), n_iov > 0 and wave < zsh_plan(n, ..).waves. The
 * leftovers of the ragged last unit lie in the last wavefront's part. */
typedef struct zsv_span { uint32_t e_lo, e_hi; } zsv_span_t;
ZC_FN zsv_span_t zsv_wave_span(const uint64_t* starts, uint32_t n_iov, uint64_t v, uint64_t n, uint64_t wave) {
    const uint64_t lo = v + wave * ZSH_WAVE_BYTES, end = v + n, hi = end - lo < ZSH_WAVE_BYTES ? end : lo + ZSH_WAVE_BYTES;
    zsv_span_t s;
    s.e_lo = zav_find(starts, 0u, n_iov - 1u, lo);
    s.e_hi = zav_find(starts, s.e_lo, n_iov - 1u, hi - 1u);
    return s;
}

/* ---- the lane's cursor (zav_cursor_t: entry r is X[lo, hi) at base; lo == hi: none yet).
 * zsv_seek: seats it on the entry that holds x, one of [e_lo, e_hi]; nothing to do when it sits there already. */
ZC_FN void zsv_seek(zav_cursor_t* cur, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi) {
    if (x < cur->lo || x >= cur->hi) {
        cur->r = zav_find(starts, e_lo, e_hi, x);
        cur->lo = starts[cur->r]; cur->hi = starts[cur->r + 1u]; cur->base = iov[cur->r].base;
    }
}
/* X[x] for cur->lo <= x < total: walks on to the entry that holds x, past empty ones, whose base is not loaded */
ZC_FN uint32_t zsv_byte(zav_cursor_t* cur, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts) {
    if (x >= cur->hi) {
        do { cur->r++; cur->lo = cur->hi; cur->hi = starts[cur->r + 1u]; } while (x >= cur->hi);
        cur->base = iov[cur->r].base;
    }
    return ((ZSV_ENTRY)(uintptr_t)cur->base)[x - cur->lo];
}
/* e4[0, 4) = X[x, x + 16) as four little-endian dwords, x + 16 <= starts[e_hi + 1]. Reads exactly those 16 bytes. */
ZC_FN void zsv_fetch16(uint32_t* e4, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi,
                       zav_cursor_t* cur) {
    zsv_seek(cur, x, iov, starts, e_lo, e_hi);
    if (x + 16u <= cur->hi) {
        zav_u128_t v;
        __builtin_memcpy(&v, (ZSV_ENTRY)(uintptr_t)cur->base + (x - cur->lo), 16);
        e4[0] = (uint32_t)v.a; e4[1] = (uint32_t)(v.a >> 32); e4[2] = (uint32_t)v.b; e4[3] = (uint32_t)(v.b >> 32);
        return;
    }
    e4[0] = e4[1] = e4[2] = e4[3] = 0u;
    ZSV_UNROLL
    for (uint32_t k = 0; k < 16u; k++) e4[k >> 2] |= zsv_byte(cur, x + k, iov, starts) << (8u * (k & 3u));
}
/* the element side of a group: e[0, 4 E) = X[x, x + 16 E). E is a constant where the kernels call this, so the loop unrolls and
 * every index into e is one. */
ZC_FN void zsv_fetch_group(uint32_t* e, uint32_t E, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo,
                           uint32_t e_hi, zav_cursor_t* cur) {
    ZSV_UNROLL
    for (uint32_t j = 0; j < E; j++) zsv_fetch16(e + 4u * j, x + 16u * j, iov, starts, e_lo, e_hi, cur);
}
/* one of the ragged leftovers, X[x], through the same cursor */
ZC_FN uint8_t zsv_fetch_byte(uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi, zav_cursor_t* cur) {
    zsv_seek(cur, x, iov, starts, e_lo, e_hi);
    return (uint8_t)zsv_byte(cur, x, iov, starts);
}

/* ---- *d_status / *d_result, written once by the call's last kernel: the table's error when the scan found one (status: the
 * zav_ctl_t's), else `word`: 0 for the kernel call, what the session's end stored for the archive call. */
ZC_FN int64_t zsv_result(int status, int64_t word) { return status < 0 ? (int64_t)status : word; }
#endif
