/* Test-only: one session of zxc_amd/csrc/zxc_append.h replayed on the host the way the entry points and kernels of
 * zxc_append_device.hip run it, over heap buffers of exactly the sizes the session is promised (every append's source is a heap
 * copy of exactly its n bytes), so that a sanitizer sees any read or write outside them. The encoder is a stand-in: block k of the
 * archive is whatever the caller says block k is (its bytes and size: the slot and size an encode launch leaves). Every job's
 * input is checked against the source the caller names: the bytes the job would read are the bytes of its block, and a job that
 * reads the append's source where it lies keeps its 32-byte over-read inside the piece.
 * Shared by append_shim.c (loaded by tests/test_compress_append_device_cpu.py) and append_san_main.c (a program of its own). */
#ifndef APPEND_REPLAY_H
#define APPEND_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_append.h"
#include "../container/stored_archive.h"

#define RP_BAD_PLAN (-1000) /* the replay's own verdict: a plan that breaks one of its promises */

typedef struct rp_session {
    zap_shape_t sh;
    zap_ctl_t ctl;
    uint8_t* area[2 + 1]; /* two carry areas, the stage area: block_size + ZAP_PAD bytes each */
    zxc_enc_job_t* jobs;
    uint32_t *sizes, *seek;
    uint64_t* offsets;
    uint8_t* slots;
    uint32_t cur, bs, stride;
    int checksum, seekable, bad;
    uint64_t total, cap, max_piece;
    uint8_t* dst;
    /* the stand-in encoder and the source it is checked against */
    const uint8_t* src;       /* the whole source, total bytes */
    const uint8_t* blocks;    /* the archive's blocks back to back */
    const uint32_t* blk_size; /* ... and their sizes */
    const uint64_t* blk_at;   /* ... and where each starts in `blocks` */
    uint32_t n_blocks;
} rp_session_t;

static int rp_begin(rp_session_t* s, uint64_t max_total, uint64_t max_piece, uint32_t bs, int checksum, int seekable, uint8_t* dst, uint64_t cap) {
    s->bs = bs; s->stride = 2u * bs + 512u; s->checksum = checksum; s->seekable = seekable; s->cur = 0; s->bad = 0; s->total = 0;
    s->cap = cap; s->max_piece = max_piece; s->dst = dst;
    const int rc = zap_shape(max_total, max_piece, bs, s->stride, seekable, &s->sh);
    if (rc != 0) return rc;
    for (int a = 0; a < 3; a++) s->area[a] = malloc((size_t)bs + ZAP_PAD);
    s->jobs = malloc(s->sh.J * sizeof(zxc_enc_job_t));
    s->sizes = malloc(s->sh.J * 4u);
    s->offsets = malloc(s->sh.J * 8u);
    s->slots = malloc((size_t)s->sh.J * s->stride);
    s->seek = malloc(seekable && s->sh.nb_max ? s->sh.nb_max * 4u : 1u);
    zap_begin(&s->ctl);
    return 0;
}
static void rp_free(rp_session_t* s) {
    for (int a = 0; a < 3; a++) free(s->area[a]);
    free(s->jobs); free(s->sizes); free(s->offsets); free(s->slots); free(s->seek);
}
static uint8_t* rp_area(rp_session_t* s, uint32_t area) {
    return area == ZAP_CARRY ? s->area[s->cur] : area == ZAP_NEXT ? s->area[s->cur ^ 1u] : s->area[2];
}

/* The stand-in encoder on job j of a piece, the archive's block k: its input is `len` bytes at `in`, which must be the source's
 * bytes of block k; block k's bytes go to slot j and its size to sizes[j]. -> 0 (and `bad`) when the input is not block k's. */
static int rp_encode_job(rp_session_t* s, uint32_t j, uint64_t k, const uint8_t* in, uint32_t len) {
    if (k >= s->n_blocks || memcmp(in, s->src + k * s->bs, len) != 0) { s->bad = 1; return 0; }
    memcpy(s->slots + (size_t)j * s->stride, s->blocks + s->blk_at[k], s->blk_size[k] <= s->stride ? s->blk_size[k] : s->stride);
    s->sizes[j] = s->blk_size[k];
    return 1;
}
/* the back half of a piece of nb > 0 blocks (ap_back): the tiles pass, the advance, scatter and gather */
static void rp_back(rp_session_t* s, uint32_t nb) {
    uint64_t sum = 0;
    uint32_t hash = 0, bad = 0;
    zap_piece_totals(s->sizes, s->slots, s->stride, nb, s->bs, s->checksum, &sum, &hash, &bad);
    uint64_t run = s->ctl.off;
    if (!zap_advance(&s->ctl, nb, sum, hash, bad, s->cap, s->checksum, s->seekable)) return;
    for (uint32_t b = 0; b < nb; b++) {
        s->offsets[b] = run;
        run += s->sizes[b];
        if (s->seekable) s->seek[s->ctl.first + b] = s->sizes[b];
        memcpy(s->dst + s->offsets[b], s->slots + (size_t)b * s->stride, s->sizes[b]);
    }
}
/* the cut of ap_pieces: *m = the bytes of the next piece of a call with `left` bytes to go. -> 0 (and `bad`) when the cut breaks a
 * promise: some bytes, no more than are left or max_piece, and every piece but a call's last ends on a block boundary */
static int rp_next_piece(rp_session_t* s, uint64_t left, uint64_t* m) {
    const uint32_t carry = (uint32_t)(s->total % s->bs);
    *m = zap_piece_len(carry, left, s->max_piece, s->bs);
    if (*m == 0 || *m > left || *m > s->max_piece || (*m < left && (carry + *m) % s->bs != 0)) { s->bad = 1; return 0; }
    return 1;
}

/* one piece, the plain front end: src = exactly the piece's p->n bytes (NULL for the plan of `end`) */
static void rp_piece(rp_session_t* s, const uint8_t* src, const zap_piece_t* p) {
    for (int c = 0; c < 3; c++) { /* the prep kernel */
        const zap_copy_t cp = p->cp[c];
        if (cp.area == ZAP_SRC) continue;
        uint8_t* d = rp_area(s, cp.area) + cp.at;
        memcpy(d, src + cp.from, cp.len);
        memset(d + cp.len, 0, ZAP_PAD);
    }
    if (p->nb > s->sh.J) { s->bad = 1; return; }
    const uint64_t first_block = s->total / s->bs; /* blocks in front of this piece */
    for (uint32_t j = 0; j < p->nb; j++) { /* the job table and the encode launch */
        const zap_src_t js = zap_job(p, j);
        const uint8_t* in = (js.area == ZAP_SRC ? src : rp_area(s, js.area)) + js.off;
        if (js.area == ZAP_SRC && js.off + js.len + ZAP_OVERREAD > p->n) s->bad = 1; /* the over-read would leave the piece */
        if (js.area != ZAP_SRC) { /* ... and in an area it meets the padding */
            for (uint32_t k = 0; k < ZAP_OVERREAD; k++) if (in[js.len + k] != 0) s->bad = 1;
        }
        rp_encode_job(s, j, first_block + j, in, js.len);
    }
    if (p->nb) rp_back(s, p->nb);
}

/* the loop of zxc_mi355x_compress_append_device: the next n bytes of the source */
static void rp_append(rp_session_t* s, uint64_t n) {
    uint8_t* mine = malloc(n ? n : 1u); /* exactly the append's bytes */
    memcpy(mine, s->src + s->total, n);
    const uint8_t* src = mine;
    uint64_t left = n, m;
    while (left && rp_next_piece(s, left, &m)) {
        uint8_t* piece = malloc(m); /* ... and exactly the piece's */
        memcpy(piece, src, m);
        zap_piece_t p;
        zap_plan_piece((uint32_t)(s->total % s->bs), m, s->bs, &p);
        rp_piece(s, piece, &p);
        free(piece);
        s->total += m; /* (rp_piece counted the blocks in front of the piece from the old total) */
        if (p.swap) s->cur ^= 1u;
        src += m; left -= m;
    }
    free(mine);
}
/* zxc_mi355x_compress_end_device -> the result word (RP_BAD_PLAN when the replay met a broken promise) */
static int64_t rp_end(rp_session_t* s) {
    zap_piece_t p;
    zap_plan_end((uint32_t)(s->total % s->bs), s->bs, &p);
    if (p.nb) rp_piece(s, NULL, &p);
    zap_finish(&s->ctl, s->dst, s->cap, s->total, s->bs, s->checksum, s->seekable);
    const uint64_t nb = s->total / s->bs + (s->total % s->bs != 0);
    if (s->seekable) for (uint64_t b = 0; b < nb; b++) zap_put_seek_entry(&s->ctl, s->dst, s->seek, b);
    return s->bad ? RP_BAD_PLAN : s->ctl.status;
}

/* A whole session: begin, the appends of lens[0 .. n_lens) (their sum is total), end. dst: cap bytes. */
static inline int64_t rp_session(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                          uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, uint32_t n_lens,
                          uint64_t max_piece, uint8_t* dst, uint64_t cap) {
    rp_session_t s;
    memset(&s, 0, sizeof s);
    s.src = src; s.blocks = blocks; s.blk_at = blk_at; s.blk_size = blk_size; s.n_blocks = n_blocks;
    const int rc = rp_begin(&s, total, max_piece, bs, checksum, seekable, dst, cap);
    if (rc != 0) return rc;
    for (uint32_t i = 0; i < n_lens; i++) rp_append(&s, lens[i]);
    const int64_t r = s.total == total ? rp_end(&s) : RP_BAD_PLAN;
    rp_free(&s);
    return r;
}

/* The promises of one plan, for a piece of n > 0 bytes behind `carry`: -> 0, or the number of the promise it breaks. */
static inline int rp_plan_check(uint32_t carry, uint64_t n, uint32_t bs) {
    zap_piece_t p;
    zap_plan_piece(carry, n, bs, &p);
    if (p.nb != (carry + n) / bs || p.tail != (carry + n) % bs) return 1;
    if (p.n_staged > 2u) return 2;
    if (p.n_direct && p.first + (uint64_t)p.n_direct * bs + ZAP_OVERREAD > n) return 3; /* the last direct job's over-read */
    /* every source byte once: the copies and the run of direct jobs, in source order, tile [0, n) */
    uint64_t lo[4], hi[4];
    int k = 0;
    for (int c = 0; c < 3; c++) {
        if (p.cp[c].area == ZAP_SRC) continue;
        if ((uint64_t)p.cp[c].at + p.cp[c].len + ZAP_PAD > (uint64_t)bs + ZAP_PAD) return 4; /* the copy and its padding fit the area */
        lo[k] = p.cp[c].from; hi[k] = p.cp[c].from + p.cp[c].len; k++;
    }
    lo[k] = p.first; hi[k] = p.first + (uint64_t)p.n_direct * bs; k++;
    uint64_t at = 0;
    for (int done = 0; done < k; done++) { /* the interval that starts where the last ended (empty ones anywhere) */
        int found = -1;
        for (int i = 0; i < k; i++) if (lo[i] == at && hi[i] > lo[i]) found = i;
        if (found < 0) break;
        at = hi[found];
    }
    uint64_t sum = 0;
    for (int i = 0; i < k; i++) sum += hi[i] - lo[i];
    if (at != n || sum != n) return 5;
    /* the jobs: the carried block first and whole, then the direct run, then the staged blocks inside the staged copy */
    for (uint32_t j = 0; j < p.nb; j++) {
        const zap_src_t s = zap_job(&p, j);
        if (s.len != bs) return 6;
        if (s.area == ZAP_CARRY && !(j == 0 && carry && p.cp[0].area == ZAP_CARRY && p.cp[0].at == carry && p.cp[0].at + p.cp[0].len == bs)) return 7;
        if (s.area == ZAP_SRC && s.off + bs + ZAP_OVERREAD > n) return 8;
        if (s.area == ZAP_STAGE && !(p.cp[1].area == ZAP_STAGE && s.off + bs <= p.cp[1].len)) return 9;
        if (s.area == ZAP_NEXT) return 10;
    }
    if (p.nb == 0 && !(p.cp[0].area == ZAP_CARRY && p.cp[0].at == carry && p.cp[0].len == n && !p.swap)) return 11;
    if (p.nb && !(p.swap && p.cp[2].area == ZAP_NEXT && p.cp[2].at == 0 && p.cp[2].len == p.tail)) return 12;
    return 0;
}
/* ---- the archive the stand-in encoder must give: rp_stored_archive of tests/container/stored_archive.h */
#endif
