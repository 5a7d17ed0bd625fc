/* Test-only: zxc_mi355x_shufflev_device and the chunks of zxc_mi355x_compress_shufflev_device (zxc_amd/csrc/zxc_shufflev_device.hip)
 * replayed on the host from the rules they run (zxc_amd/csrc/zxc_shufflev.h on top of zxc_shuffle.h and zxc_appendv.h): the scan
 * in series (zav_scan_serial), then per chunk of `piece` bytes the gather-shuffle kernel's grid: for every wavefront the entries
 * zsv_wave_span narrows the search to, 64 cursors, and for every turn and lane the group zsh_group gives it, fetched from the
 * entries by zsv_fetch_group, transposed by zsh_regs_shuffle and stored with 16-byte copies; then the last wavefront's byte-wise
 * leftovers through the same cursors. Every byte written is counted, so that a byte two lanes write, or none, shows even where the
 * values agree. After a table error the replay, like the kernels, touches neither an entry nor the destination.
 * svr_check runs one table: every entry is a heap buffer of its own that ENDS with the entry (exactly len bytes behind k < 16
 * alignment bytes, k walking through 0 .. 15 from entry to entry), an empty entry's base is 0 or 0x10 and never looked at, the
 * destination lies between SVR_CANARY pattern bytes (0 in the sanitizer program, where AddressSanitizer sees the first byte
 * outside), and the expected bytes come from the index map zsh_index over the concatenation alone. */
#ifndef SHUFFLEV_REPLAY_H
#define SHUFFLEV_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_shufflev.h"

#ifndef SVR_CANARY
#define SVR_CANARY 32u
#endif

/* the kernel's grid over the chunk X[v, v + n) -> dst[0, n); hits[0, n) counts the writes */
static inline void svr_kernel(const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, uint64_t v, uint8_t* dst,
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
                zsv_fetch_group(e, E, v + g.elem_at, iov, starts, sp.e_lo, sp.e_hi, &cur[lane]);
                zsh_regs_shuffle(e, p, E);
                for (uint32_t k = 0; k < E; k++) {
                    const uint64_t at = g.plane_at + (uint64_t)k * g.q;
                    memcpy(dst + at, p + 4u * k, 16);
                    for (uint32_t b = 0; b < 16u; b++) hits[at + b]++;
                }
            }
        if (w == pl.waves - 1u)
            for (uint32_t lane = 0; lane < 64u; lane++)
                for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                    uint64_t plain, shuffled;
                    zsh_ragged_byte(&pl, j, &plain, &shuffled);
                    dst[shuffled] = zsv_fetch_byte(v + plain, iov, starts, sp.e_lo, sp.e_hi, &cur[lane]);
                    hits[shuffled]++;
                }
    }
}

/* The call: the scan, then the chunks (piece: a multiple of unit, or 0 for one chunk, the kernel call) -> the table's status.
 * Chunk `at` goes to dst + at: where the archive call's stage ends up in the shuffle of X. */
static inline int svr_call(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece, uint8_t* dst,
                           uint8_t* hits) {
    uint64_t* starts = malloc(8u * ((size_t)n_iov + 1u));
    const int status = n_iov ? zav_scan_serial(iov, n_iov, total, starts) : 0;
    if (!piece) piece = total;
    for (uint64_t at = 0; at < total; at += piece)
        svr_kernel(iov, starts, n_iov, status, at, dst + at, hits + at, total - at < piece ? total - at : piece, E, unit);
    free(starts);
    return status;
}

/* ---- the entries of x[0, sum of lens) as buffers of their own */
typedef struct svr_src {
    zxc_dev_iov_t* iov;
    uint8_t** raw;
    uint32_t n;
} svr_src_t;
static inline svr_src_t svr_entries(const uint8_t* x, const uint64_t* lens, uint32_t n_iov, uint32_t a0) {
    svr_src_t s;
    uint64_t at = 0;
    s.n = n_iov;
    s.iov = malloc(sizeof(zxc_dev_iov_t) * ((size_t)n_iov + 1u));
    s.raw = malloc(sizeof(uint8_t*) * ((size_t)n_iov + 1u));
    for (uint32_t r = 0; r < n_iov; r++) {
        const uint32_t a = (a0 + r) & 15u; /* (malloc's result is 16-byte aligned) */
        s.raw[r] = NULL;
        s.iov[r].len = lens[r];
        s.iov[r].base = (r & 1u) ? 0u : 0x10u;
        if (lens[r]) {
            s.raw[r] = malloc(a + lens[r]);
            memset(s.raw[r], 0xA5, a);
            memcpy(s.raw[r] + a, x + at, lens[r]);
            s.iov[r].base = (uint64_t)(uintptr_t)(s.raw[r] + a);
        }
        at += lens[r];
    }
    return s;
}
static inline void svr_release(svr_src_t* s) {
    for (uint32_t r = 0; r < s->n; r++) free(s->raw[r]);
    free(s->raw); free(s->iov);
    s->raw = NULL; s->iov = NULL;
}

static inline uint8_t svr_pat(uint64_t i) { return (uint8_t)(1u + i % 251u); }
typedef struct svr_dst { uint8_t *raw, *at, *hits; uint64_t n, size; } svr_dst_t;
static inline svr_dst_t svr_dst(uint64_t n, uint32_t align) {
    svr_dst_t d;
    d.n = n;
    d.size = SVR_CANARY + align + n + SVR_CANARY;
    d.raw = malloc(d.size ? d.size : 1u);
    for (uint64_t i = 0; i < d.size; i++) d.raw[i] = svr_pat(i);
    d.at = d.raw + SVR_CANARY + align;
    d.hits = calloc(n ? n : 1u, 1);
    return d;
}
/* every byte of [0, n) written `want` times, nothing around them changed */
static inline int svr_dst_ok(const svr_dst_t* d, uint8_t want) {
    const uint64_t lo = (uint64_t)(d->at - d->raw);
    for (uint64_t i = 0; i < d->n; i++) if (d->hits[i] != want) return 0;
    for (uint64_t i = 0; i < lo; i++) if (d->raw[i] != svr_pat(i)) return 0;
    for (uint64_t i = lo + d->n; i < d->size; i++) if (d->raw[i] != svr_pat(i)) return 0;
    if (!want) for (uint64_t i = lo; i < lo + d->n; i++) if (d->raw[i] != svr_pat(i)) return 0;
    return 1;
}
static inline void svr_dst_free(svr_dst_t* d) { free(d->hits); free(d->raw); }

/* One valid table over x[0, total), total = the sum of lens -> 0, or which check failed. out (may be NULL): receives the result. */
static inline int svr_check(const uint8_t* x, const uint64_t* lens, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece,
                            uint32_t a0, uint32_t dst_align, uint8_t* out) {
    svr_src_t src = svr_entries(x, lens, n_iov, a0);
    svr_dst_t dst = svr_dst(total, dst_align);
    int rc = 0;
    if (svr_call(src.iov, n_iov, total, E, unit, piece, dst.at, dst.hits) != 0) rc = 1;
    if (!rc && !svr_dst_ok(&dst, 1u)) rc = 2;                                          /* every byte written once, none outside */
    for (uint64_t p = 0; p < total && !rc; p++) if (dst.at[zsh_index(p, total, E, unit)] != x[p]) rc = 3; /* the definition's value */
    if (out) memcpy(out, dst.at, total);
    svr_dst_free(&dst);
    svr_release(&src);
    return rc;
}

/* A table the scan refuses: the promise is `promised`, entry `null_at` (< n_iov, or ~0 for none) gets a zero base. With
 * entries_gone the entries are freed before the call (the sanitizer program: a read of one is a use after free).
 * -> the status, or a positive number when an entry or the destination was touched */
static inline int svr_check_bad(const uint8_t* x, const uint64_t* lens, uint32_t n_iov, uint64_t promised, uint32_t null_at, uint32_t E,
                                uint32_t unit, uint64_t piece, int entries_gone) {
    svr_src_t src = svr_entries(x, lens, n_iov, 3u);
    svr_dst_t dst = svr_dst(promised, 5u);
    if (null_at < n_iov) src.iov[null_at].base = 0u;
    if (entries_gone)
        for (uint32_t r = 0; r < n_iov; r++) { free(src.raw[r]); src.raw[r] = NULL; }
    int rc = svr_call(src.iov, n_iov, promised, E, unit, piece, dst.at, dst.hits);
    if (rc >= 0) rc = 1;
    else if (!svr_dst_ok(&dst, 0u)) rc = 2;
    svr_dst_free(&dst);
    svr_release(&src);
    return rc;
}
#endif
