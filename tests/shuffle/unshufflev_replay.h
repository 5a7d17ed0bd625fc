/* Test-only: zxc_mi355x_unshufflev_device and the chunks of zxc_mi355x_decompress_shufflev_device
 * (zxc_amd/csrc/zxc_unshufflev_device.hip) replayed on the host from the rules they run (zxc_amd/csrc/zxc_unshufflev.h on top of
 * zxc_shufflev.h, zxc_shuffle.h and zxc_takev.h): the scan in series (zav_scan_serial), then per chunk of `piece` bytes the
 * scatter-un-shuffle kernel's grid: for every wavefront the entries zsv_wave_span narrows the search to, 64 cursors, and for every
 * turn and lane the group zsh_group gives it, loaded from the planes of the contiguous source with 16-byte copies, transposed by
 * zsh_regs_unshuffle and stored into the entries by zuv_store_group; then the last wavefront's byte-wise leftovers through the
 * same cursors. Every store the plan makes is counted per byte of Y (a 16-byte run counts its 16 bytes, a leftover its one), so
 * that a byte of Y two lanes own, or none, shows even where the values agree; that a store writes the bytes it was counted for
 * and no others is what the canaries around every entry, the values and, in the sanitizer program, the end of every heap buffer
 * show. After a table error the replay, like the kernels, touches neither the source nor an entry.
 * uvr_check runs one table: every entry is a heap buffer of its own, exactly len bytes behind k < 16 alignment bytes (k walking
 * through 0 .. 15 from entry to entry) between UVR_CANARY pattern bytes (0 in the sanitizer program, where the buffer ENDS with
 * the entry and AddressSanitizer sees the first byte outside), an empty entry's base is 0 or 0x10 and never looked at, and the
 * expected bytes come from the index map zsh_index over the source alone. */
#ifndef UNSHUFFLEV_REPLAY_H
#define UNSHUFFLEV_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_unshufflev.h"

#ifndef UVR_CANARY
#define UVR_CANARY 32u
#endif

/* the kernel's grid over the chunk src[0, n) -> Y[v, v + n); hits[0, n) counts the stores of Y[v ..] */
static inline void uvr_kernel(const uint8_t* src, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, uint64_t v,
                              uint8_t* hits, uint64_t n, uint32_t E, uint32_t unit) {
    if (status < 0) return;
    const zsh_plan_t pl = zsh_plan(n, E, unit);
    for (uint64_t w = 0; w < pl.waves; w++) {
        const zsv_span_t sp = zsv_wave_span(starts, n_iov, v, n, w);
        zav_cursor_t cur[64];
        memset(cur, 0, sizeof cur);
        for (uint32_t turn = 0; turn < 8u / E; turn++)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                zsh_group_t g;
                uint32_t e[32], p[32];
                if (!zsh_group(&pl, w, turn, lane, &g)) continue;
                for (uint32_t k = 0; k < E; k++) memcpy(p + 4u * k, src + g.plane_at + (uint64_t)k * g.q, 16);
                zsh_regs_unshuffle(p, e, E);
                zuv_store_group(e, E, v + g.elem_at, iov, starts, sp.e_lo, sp.e_hi, &cur[lane]);
                for (uint32_t b = 0; b < 16u * E; b++) hits[g.elem_at + b]++;
            }
        if (w == pl.waves - 1u)
            for (uint32_t lane = 0; lane < 64u; lane++)
                for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                    uint64_t plain, shuffled;
                    zsh_ragged_byte(&pl, j, &plain, &shuffled);
                    zuv_store_byte(v + plain, src[shuffled], iov, starts, sp.e_lo, sp.e_hi, &cur[lane]);
                    hits[plain]++;
                }
    }
}

/* The call: the scan, then the chunks (piece: a multiple of unit, or 0 for one chunk, the kernel call) -> the scan's status.
 * Chunk `at` is read at src + at: where the archive call's stage comes from in the shuffle of Y. */
static inline int uvr_call(const uint8_t* src, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece,
                           uint8_t* hits) {
    uint64_t* starts = malloc(8u * ((size_t)n_iov + 1u));
    const int status = n_iov ? zav_scan_serial(iov, n_iov, total, starts) : 0;
    if (!piece) piece = total;
    for (uint64_t at = 0; at < total; at += piece)
        uvr_kernel(src + at, iov, starts, n_iov, status, at, hits + at, total - at < piece ? total - at : piece, E, unit);
    free(starts);
    return status;
}

/* ---- the entries as buffers of their own: [UVR_CANARY | a alignment bytes | len | UVR_CANARY], all pattern bytes */
static inline uint8_t uvr_pat(uint64_t i) { return (uint8_t)(1u + i % 251u); }
typedef struct uvr_dst {
    zxc_dev_iov_t* iov;
    uint8_t** raw;
    uint64_t* lead; /* bytes in front of the entry in its buffer */
    uint32_t n;
} uvr_dst_t;
static inline uvr_dst_t uvr_entries(const uint64_t* lens, uint32_t n_iov, uint32_t a0) {
    uvr_dst_t d;
    d.n = n_iov;
    d.iov = malloc(sizeof(zxc_dev_iov_t) * ((size_t)n_iov + 1u));
    d.raw = malloc(sizeof(uint8_t*) * ((size_t)n_iov + 1u));
    d.lead = malloc(sizeof(uint64_t) * ((size_t)n_iov + 1u));
    for (uint32_t r = 0; r < n_iov; r++) {
        const uint32_t a = (a0 + r) & 15u; /* (malloc's result is 16-byte aligned; UVR_CANARY is a multiple of 16) */
        d.raw[r] = NULL;
        d.lead[r] = UVR_CANARY + a;
        d.iov[r].len = lens[r];
        d.iov[r].base = (r & 1u) ? 0u : 0x10u;
        if (lens[r]) {
            const uint64_t size = d.lead[r] + lens[r] + UVR_CANARY;
            d.raw[r] = malloc(size);
            for (uint64_t i = 0; i < size; i++) d.raw[r][i] = uvr_pat(i + r);
            d.iov[r].base = (uint64_t)(uintptr_t)(d.raw[r] + d.lead[r]);
        }
    }
    return d;
}
/* nothing around the entries changed; with `untouched`, nothing inside them either */
static inline int uvr_entries_ok(const uvr_dst_t* d, int untouched) {
    for (uint32_t r = 0; r < d->n; r++) {
        if (!d->raw[r]) continue;
        const uint64_t lo = d->lead[r], hi = lo + d->iov[r].len, size = hi + UVR_CANARY;
        for (uint64_t i = 0; i < size; i++)
            if ((i < lo || i >= hi || untouched) && d->raw[r][i] != uvr_pat(i + r)) return 0;
    }
    return 1;
}
static inline void uvr_release(uvr_dst_t* d) {
    for (uint32_t r = 0; r < d->n; r++) free(d->raw[r]);
    free(d->raw); free(d->iov); free(d->lead);
    d->raw = NULL; d->iov = NULL; d->lead = NULL;
}

/* One valid table over the source y[0, total), total = the sum of lens -> 0, or which check failed. out (may be NULL): receives
 * the entries' bytes, concatenated. */
static inline int uvr_check(const uint8_t* y, const uint64_t* lens, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece,
                            uint32_t a0, uint8_t* out) {
    uvr_dst_t dst = uvr_entries(lens, n_iov, a0);
    uint8_t* hits = calloc(total ? total : 1u, 1);
    int rc = 0;
    if (uvr_call(y, dst.iov, n_iov, total, E, unit, piece, hits) != 0) rc = 1;
    for (uint64_t p = 0; p < total && !rc; p++) if (hits[p] != 1u) rc = 2;             /* every byte of Y stored once */
    if (!rc && !uvr_entries_ok(&dst, 0)) rc = 3;                                        /* nothing outside the entries */
    uint64_t p = 0;
    for (uint32_t r = 0; r < n_iov; r++)
        for (uint64_t i = 0; i < lens[r]; i++, p++) {
            const uint8_t got = dst.raw[r][dst.lead[r] + i];
            if (!rc && got != y[zsh_index(p, total, E, unit)]) rc = 4;                   /* the definition's value */
            if (out) out[p] = got;
        }
    free(hits);
    uvr_release(&dst);
    return rc;
}

/* A table the scan refuses: the promise is `promised`, entry `null_at` (< n_iov, or ~0 for none) gets a zero base. With
 * entries_gone the entries are freed before the call (the sanitizer program: a store into one is a use after free).
 * -> the call's status word (zuv_result), or a positive number when an entry was touched */
static inline int uvr_check_bad(const uint8_t* y, const uint64_t* lens, uint32_t n_iov, uint64_t promised, uint32_t null_at, uint32_t E,
                                uint32_t unit, uint64_t piece, int entries_gone) {
    uvr_dst_t dst = uvr_entries(lens, n_iov, 3u);
    uint8_t* hits = calloc(promised ? promised : 1u, 1);
    if (null_at < n_iov) dst.iov[null_at].base = 0u;
    if (entries_gone)
        for (uint32_t r = 0; r < n_iov; r++) { free(dst.raw[r]); dst.raw[r] = NULL; }
    int rc = (int)zuv_result(uvr_call(y, dst.iov, n_iov, promised, E, unit, piece, hits), 0, 0u);
    if (rc >= 0) rc = 1;
    else if (!uvr_entries_ok(&dst, 1)) rc = 2;
    for (uint64_t p = 0; p < promised && rc < 0; p++) if (hits[p]) rc = 3;
    free(hits);
    uvr_release(&dst);
    return rc;
}
#endif
