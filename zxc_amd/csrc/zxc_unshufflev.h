/* zxc_unshufflev.h — the rules of the inverse byte-shuffle into a table of buffers (include/zxc_mi355x_unshufflev.h, kernels and
 * calls in zxc_unshufflev_device.hip) on top of zxc_shufflev.h and zxc_takev.h: the store of a group's element bytes into the
 * entries, and the word the call's last kernel writes. Plain inline C that hipcc and a host C compiler both take, so that the
 * kernels and the CPU tests (tests/shuffle/unshufflev_replay.h) run the same lines.
 *
 * The destination is zxc_takev.h's virtual one: Y, the concatenation of the table's entries, total bytes; starts[r] is the offset
 * of entry r in Y. A chunk is Y[v, v + n) with v a multiple of the unit, so its units are Y's and zsh_plan(n, E, unit) over it
 * hands out the groups zsh_plan over all of Y would. What carries over from zxc_shufflev.h as it is: the scratch (zsv_shape,
 * zsv_scratch_size), the entries a wavefront's element side meets (zsv_wave_span), the lane's cursor and its seat (zav_cursor_t,
 * zsv_seek); from zxc_shuffle.h the plan (zsh_plan, zsh_group, zsh_ragged_byte) and zsh_regs_unshuffle. So wavefront, turn and
 * lane own the groups they own in the gather kernels. The plane side is the contiguous source: E 16-byte loads per group, the
 * kernel's own. The element side is new: group G's 16 E bytes go to Y[v + 16 E G, + 16 E) as E runs of 16 bytes. A run inside
 * one entry is one 16-byte store at whatever alignment base + off has; a run that crosses an entry boundary is stored a byte at a
 * time into consecutive entries, past empty ones, whose base is not looked at. Exactly the bytes of the entries are written:
 * nothing is promised writable behind an entry. No pointer into an entry carries an aliasing claim: entries are told apart by
 * the table alone. */
#ifndef ZXC_UNSHUFFLEV_H
#define ZXC_UNSHUFFLEV_H
#include "../../include/zxc_mi355x_unshufflev.h"
#include "zxc_shufflev.h"
#include "zxc_takev.h"

/* an entry's bytes, writable: its base is an address in device memory (a global store in the kernels, not a flat one) */
#ifdef __HIP_DEVICE_COMPILE__
#define ZUV_ENTRY __attribute__((address_space(1))) uint8_t*
#else
#define ZUV_ENTRY uint8_t*
#endif

/* The work area of the archive call: [session | result word | stage] are the sibling's `shuffle_ws` bytes
 * (zxc_mi355x_decompress_shuffle_device_work_size, which holds the session's word already), and the table scratch starts on the
 * next multiple of 256 counted from d_work. 0 when the sibling gives 0. */
ZC_FN uint64_t zuv_work_size(uint64_t shuffle_ws, uint32_t n_iov) {
    return shuffle_ws ? zc_round_up(shuffle_ws, 256u) + zsv_scratch_size(n_iov) : 0u;
}

/* Y[x] = b for cur->lo <= x < total: walks on to the entry that holds x, past empty ones, whose base is not loaded */
ZC_FN void zuv_byte(zav_cursor_t* cur, uint64_t x, uint32_t b, const zxc_dev_iov_t* iov, const uint64_t* starts) {
    if (x >= cur->hi) {
        do { cur->r++; cur->lo = cur->hi; cur->hi = starts[cur->r + 1u]; } while (x >= cur->hi);
        cur->base = iov[cur->r].base;
    }
    ((ZUV_ENTRY)(uintptr_t)cur->base)[x - cur->lo] = (uint8_t)b;
}
/* Y[x, x + 16) = e4[0, 4) as four little-endian dwords, x + 16 <= starts[e_hi + 1]. Writes exactly those 16 bytes. */
ZC_FN void zuv_store16(const uint32_t* e4, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi,
                       zav_cursor_t* cur) {
    zsv_seek(cur, x, iov, starts, e_lo, e_hi);
    if (x + 16u <= cur->hi) {
        zav_u128_t v;
        v.a = (uint64_t)e4[0] | (uint64_t)e4[1] << 32; v.b = (uint64_t)e4[2] | (uint64_t)e4[3] << 32;
        __builtin_memcpy((ZUV_ENTRY)(uintptr_t)cur->base + (x - cur->lo), &v, 16);
        return;
    }
    ZSV_UNROLL
    for (uint32_t k = 0; k < 16u; k++) zuv_byte(cur, x + k, (e4[k >> 2] >> (8u * (k & 3u))) & 0xFFu, iov, starts);
}
/* the element side of a group: Y[x, x + 16 E) = e[0, 4 E). E is a constant where the kernels call this, so the loops unroll and
 * every index into e is one. A group that lies inside one entry, which is every group but a few when the entries are large, is
 * decided once and its E stores follow each other with no branch between them; else run by run. */
ZC_FN void zuv_store_group(const uint32_t* e, uint32_t E, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo,
                           uint32_t e_hi, zav_cursor_t* cur) {
    zsv_seek(cur, x, iov, starts, e_lo, e_hi);
    if (x + 16u * E <= cur->hi) {
        ZUV_ENTRY d = (ZUV_ENTRY)(uintptr_t)cur->base + (x - cur->lo);
        ZSV_UNROLL
        for (uint32_t j = 0; j < E; j++) {
            zav_u128_t v;
            v.a = (uint64_t)e[4u * j] | (uint64_t)e[4u * j + 1u] << 32; v.b = (uint64_t)e[4u * j + 2u] | (uint64_t)e[4u * j + 3u] << 32;
            __builtin_memcpy(d + 16u * j, &v, 16);
        }
        return;
    }
    ZSV_UNROLL
    for (uint32_t j = 0; j < E; j++) zuv_store16(e + 4u * j, x + 16u * j, iov, starts, e_lo, e_hi, cur);
}
/* one of the ragged leftovers, Y[x] = b, through the same cursor */
ZC_FN void zuv_store_byte(uint64_t x, uint32_t b, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi,
                          zav_cursor_t* cur) {
    zsv_seek(cur, x, iov, starts, e_lo, e_hi);
    zuv_byte(cur, x, b, iov, starts);
}

/* ---- *d_status / *d_result, written once by the call's last kernel. The table's status for this direction is takev's
 * (ztv_verdict of what the scan stored in the zav_ctl_t): it wins. Else `word`, 0 for the kernel call and what the take session's
 * end stored for the archive call, with the sibling's size check: a decoded size other than the `total` the caller planned with
 * is not the archive the caller described; total == 0: the empty-frame probe's answer as it is. */
ZC_FN int64_t zuv_result(int status, int64_t word, uint64_t total) {
    const int verdict = ztv_verdict(status);
    if (verdict < 0) return (int64_t)verdict;
    if (total > 0 && word >= 0 && (uint64_t)word != total) return ZXC_ERROR_CORRUPT_DATA;
    return word;
}
#endif
