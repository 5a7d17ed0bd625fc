/* Test-only: the shuffle kernels of zxc_amd/csrc/zxc_shuffle_device.hip replayed on the host from the rules they run
 * (zxc_amd/csrc/zxc_shuffle.h): for every wavefront, turn and lane the group zsh_group gives it, moved with 16-byte copies at
 * whatever alignment the buffers have and transposed by zsh_regs_shuffle / zsh_regs_unshuffle, then the last wavefront's byte-wise
 * leftovers. Every byte written is counted, so that a byte two lanes write, or none, shows even where the values agree.
 * shr_check runs one (n, E, unit, source alignment, destination alignment): source and destination are heap buffers of their own
 * with SHR_CANARY pattern bytes in front and behind (0 in the sanitizer program, where the allocation ends with the data and
 * AddressSanitizer sees the first byte outside), the expected bytes come from the index map zsh_index alone, and un-shuffle must
 * give the source back. */
#ifndef SHUFFLE_REPLAY_H
#define SHUFFLE_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_shuffle.h"

#ifndef SHR_CANARY
#define SHR_CANARY 32u
#endif

static inline void shr_put16(uint8_t* dst, uint8_t* hits, uint64_t at, const uint32_t* v) {
    memcpy(dst + at, v, 16);
    for (uint32_t b = 0; b < 16u; b++) hits[at + b]++;
}

/* dst[0, n) from src[0, n) as the kernel's grid moves it; hits[0, n) counts the writes */
static inline void shr_replay(const uint8_t* src, uint8_t* dst, uint8_t* hits, uint64_t n, uint32_t E, uint32_t unit, int inverse) {
    const zsh_plan_t pl = zsh_plan(n, E, unit);
    for (uint64_t w = 0; w < pl.waves; w++) {
        for (uint32_t turn = 0; turn < 8u / E; turn++)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                zsh_group_t g;
                uint32_t e[32], p[32];
                if (!zsh_group(&pl, w, turn, lane, &g)) continue;
                if (!inverse) {
                    for (uint32_t j = 0; j < E; j++) memcpy(e + 4u * j, src + g.elem_at + 16u * j, 16);
                    zsh_regs_shuffle(e, p, E);
                    for (uint32_t k = 0; k < E; k++) shr_put16(dst, hits, g.plane_at + (uint64_t)k * g.q, p + 4u * k);
                } else {
                    for (uint32_t k = 0; k < E; k++) memcpy(p + 4u * k, src + g.plane_at + (uint64_t)k * g.q, 16);
                    zsh_regs_unshuffle(p, e, E);
                    for (uint32_t j = 0; j < E; j++) shr_put16(dst, hits, g.elem_at + 16u * j, e + 4u * j);
                }
            }
        if (w == pl.waves - 1u)
            for (uint32_t lane = 0; lane < 64u; lane++)
                for (uint32_t j = lane; j < pl.ragged; j += 64u) {
                    uint64_t plain, shuffled;
                    zsh_ragged_byte(&pl, j, &plain, &shuffled);
                    if (!inverse) { dst[shuffled] = src[plain]; hits[shuffled]++; }
                    else { dst[plain] = src[shuffled]; hits[plain]++; }
                }
    }
}

/* the definition: dst[zsh_index(p)] = src[p], or its inverse */
static inline void shr_by_index(const uint8_t* src, uint8_t* dst, uint64_t n, uint32_t E, uint32_t unit, int inverse) {
    for (uint64_t p = 0; p < n; p++) {
        const uint64_t s = zsh_index(p, n, E, unit);
        if (!inverse) dst[s] = src[p];
        else dst[p] = src[s];
    }
}

typedef struct shr_buf { uint8_t *raw, *at; uint64_t size; } shr_buf_t;
static inline uint8_t shr_pat(uint64_t i) { return (uint8_t)(1u + i % 251u); }
static inline shr_buf_t shr_alloc(uint64_t n, uint32_t align) {
    shr_buf_t b;
    /* 16-byte aligned start (malloc's), then the canary (a multiple of 16) and `align` more pattern bytes in front of the data */
    b.size = SHR_CANARY + align + n + SHR_CANARY;
    b.raw = malloc(b.size ? b.size : 1u);
    for (uint64_t i = 0; i < b.size; i++) b.raw[i] = shr_pat(i);
    b.at = b.raw + SHR_CANARY + align;
    return b;
}
static inline int shr_guards_ok(const shr_buf_t* b, uint64_t n) {
    for (uint64_t i = 0; i < (uint64_t)(b->at - b->raw); i++) if (b->raw[i] != shr_pat(i)) return 0;
    for (uint64_t i = (uint64_t)(b->at - b->raw) + n; i < b->size; i++) if (b->raw[i] != shr_pat(i)) return 0;
    return 1;
}

/* -> 0, or which check failed */
static inline int shr_check(uint64_t n, uint32_t E, uint32_t unit, uint32_t src_align, uint32_t dst_align, uint32_t seed) {
    shr_buf_t src = shr_alloc(n, src_align), dst = shr_alloc(n, dst_align), back = shr_alloc(n, src_align ^ 9u);
    uint8_t *want = malloc(n ? n : 1u), *hits = calloc(n ? n : 1u, 1), *keep = malloc(n ? n : 1u);
    int rc = 0;
    for (uint64_t i = 0; i < n; i++) src.at[i] = (uint8_t)((i * 2654435761u + seed) >> 13);
    memcpy(keep, src.at, n);
    shr_by_index(src.at, want, n, E, unit, 0);
    shr_replay(src.at, dst.at, hits, n, E, unit, 0);
    for (uint64_t i = 0; i < n && !rc; i++) if (hits[i] != 1u) rc = 1;             /* every byte written once */
    if (!rc && memcmp(dst.at, want, n)) rc = 2;                                       /* ... with the definition's value */
    if (!rc && (!shr_guards_ok(&dst, n) || !shr_guards_ok(&src, n) || memcmp(src.at, keep, n))) rc = 3;
    memset(hits, 0, n);
    shr_replay(dst.at, back.at, hits, n, E, unit, 1);
    for (uint64_t i = 0; i < n && !rc; i++) if (hits[i] != 1u) rc = 4;
    if (!rc && memcmp(back.at, keep, n)) rc = 5;                                      /* un-shuffle(shuffle(x)) == x */
    if (!rc && (!shr_guards_ok(&back, n) || !shr_guards_ok(&dst, n))) rc = 6;
    free(keep); free(hits); free(want); free(back.raw); free(dst.raw); free(src.raw);
    return rc;
}
#endif
