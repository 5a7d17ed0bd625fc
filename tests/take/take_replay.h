/* Test-only: one session of zxc_amd/csrc/zxc_take.h replayed on the host the way the entry points and kernels of
 * zxc_take_device.hip run it, over heap buffers of exactly the sizes the session is promised, so that a sanitizer sees any read
 * or write outside them. The container stages are the real ones of zxc_container.h (head, seek plan or walk, events, verdict).
 * The decoder is a stand-in: block i of the chain decodes to the bytes and the status the caller names; it copies them to where
 * the job says and then scribbles 32 bytes behind them, as the decoders' 16-byte stores may, so that a wrong copy order or a
 * wrong direct rule shows in the pieces. A job of size 0 is answered with an error status and nothing is written.
 * Shared by take_shim.c (loaded by tests/test_decompress_take_device_cpu.py) and take_san_main.c (a program of its own). */
#ifndef TAKE_REPLAY_H
#define TAKE_REPLAY_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_takev.h" /* zxc_take.h, and the chunk of a takev for the shared loop */

#define TR_BAD_PLAN (-1000) /* the replay's own verdict: a plan that breaks one of its promises */
#define TR_SCRIBBLE 0xEEu
#define TR_CANARY 0xC3u
#define TR_GUARD 64u /* canary bytes in front of and behind a piece */

typedef struct tr_session {
    zt_shape_t sh;
    zc_ctl_t ctl;
    zxc_dev_job_t *jobs, *cjobs;
    int32_t* status;
    uint8_t *carry[2], *slots;
    int64_t carry_block[2]; /* the block each carry slot holds (-1: none) */
    uint8_t* decoded;       /* per job of the capacity: how often it was decoded */
    uint32_t cur, bs, tables;
    uint64_t pos, cap, max_piece;
    int bad;
    const uint8_t* src;
    uint64_t src_size;
    /* the stand-in decoder: what block i of the chain decodes to */
    const uint8_t* blk_bytes;  /* the blocks' decoded bytes back to back */
    const uint64_t* blk_at;    /* ... where each starts */
    const int32_t* blk_status; /* ... and its status: the decoded size or the error (for the table the head picks) */
    uint32_t n_blocks;
} tr_session_t;

/* begin: the shape, the work area, and the container stages of zxc_mi355x_decompress_device in series */
static int tr_begin(tr_session_t* s, const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, int want_verify,
                    int use_table, int have_dict, uint32_t dict_id) {
    s->src = src; s->src_size = src_size; s->cap = cap; s->max_piece = max_piece; s->bs = bs; s->tables = 1u + (want_verify ? 1u : 0u);
    s->cur = 0; s->pos = 0; s->bad = 0; s->carry_block[0] = s->carry_block[1] = -1;
    if (src_size < ZC_FILE_HDR + ZC_FOOTER) return ZXC_ERROR_SRC_TOO_SMALL;
    const int rc = zt_shape(cap, max_piece, bs, &s->sh);
    if (rc != 0) return rc;
    const uint32_t nj = s->sh.n_jobs;
    s->jobs = calloc((size_t)2u * nj, sizeof(zxc_dev_job_t));
    s->status = malloc((size_t)2u * nj * 4u);
    for (uint32_t i = 0; i < 2u * nj; i++) s->status[i] = 0x7FFFFFFF; /* a status nobody wrote */
    s->cjobs = malloc((size_t)2u * s->sh.J * sizeof(zxc_dev_job_t));
    s->carry[0] = malloc(s->sh.slot_stride);
    s->carry[1] = malloc(s->sh.slot_stride);
    s->slots = malloc((size_t)s->sh.J * s->sh.slot_stride);
    s->decoded = calloc(nj, 1);
    zc_head_dict(src, src_size, cap, bs, want_verify, nj, &s->ctl, have_dict, dict_id);
    if (cap > 0 && !s->ctl.final) {
        zxc_dev_job_t* tab = s->jobs + (size_t)s->ctl.sel * nj;
        if (!(use_table && zc_seek_plan(src, bs, nj, &s->ctl, tab))) {
            memset(tab, 0, (size_t)nj * sizeof *tab);
            zc_walk(src, src_size, bs, nj, nj, &s->ctl, tab);
        }
    }
    return 0;
}
static void tr_free(tr_session_t* s) {
    free(s->jobs); free(s->status); free(s->cjobs); free(s->carry[0]); free(s->carry[1]); free(s->slots); free(s->decoded);
}

/* the stand-in for one job of the decode launch: -> its status */
static int32_t tr_decode(tr_session_t* s, const zxc_dev_job_t* job, uint64_t block, uint8_t* out) {
    if (job->comp_size == 0) return ZXC_ERROR_SRC_TOO_SMALL; /* an empty job: nothing read, nothing written */
    if (block >= s->n_blocks || job->out_len != s->bs) { s->bad = 1; return ZXC_ERROR_CORRUPT_DATA; }
    const int32_t st = s->blk_status[block];
    const uint32_t n = st > 0 ? ((uint32_t)st < s->bs ? (uint32_t)st : s->bs) : 0u;
    memcpy(out, s->blk_bytes + s->blk_at[block], n);
    memset(out + n, TR_SCRIBBLE, ZT_SPILL);
    return st;
}

/* plan kernel and decode launches of one chunk; d: where the chunk's first byte goes */
static void tr_chunk_decode(tr_session_t* s, uint8_t* d, const zt_chunk_t* c, uint64_t room) {
    const uint32_t nj = s->sh.n_jobs, J = s->sh.J;
    if (c->nb > J || c->first + c->nb > nj) { s->bad = 1; return; }
    for (uint32_t tb = 0; tb < s->tables; tb++)
        for (uint32_t j = 0; j < c->nb; j++) s->cjobs[(size_t)tb * J + j] = s->jobs[(size_t)tb * nj + c->first + j];
    for (uint32_t tb = 0; tb < s->tables; tb++)
        for (uint32_t j = 0; j < c->nb; j++) {
            const zt_place_t p = zt_job_place(c, j);
            uint8_t* out;
            if (p.kind == ZT_DIRECT) {
                out = d + p.at;
                if (((uintptr_t)out & 15u) != 0 || p.at + s->bs + ZT_SPILL > room || p.at + s->bs > c->n) s->bad = 1;
            } else if (p.kind == ZT_SLOT) {
                if (p.slot >= J) { s->bad = 1; continue; }
                out = s->slots + (size_t)p.slot * s->sh.slot_stride;
            } else {
                out = s->carry[p.slot];
                if (p.slot != (c->cur ^ 1u)) s->bad = 1;
                s->carry_block[p.slot] = (int64_t)(c->first + j);
            }
            s->status[(size_t)tb * nj + c->first + j] = tr_decode(s, &s->cjobs[(size_t)tb * J + j], c->first + j, out);
            if (tb == 0 && s->decoded[c->first + j]++ != 0) s->bad = 1; /* every block once */
        }
}
/* ... and its copies, behind them */
static void tr_chunk_copy(tr_session_t* s, uint8_t* d, const zt_chunk_t* c) {
    if (s->ctl.final) return;
    const int32_t* st = s->status + (size_t)s->ctl.sel * s->sh.n_jobs;
    for (uint32_t k = 0; k < c->nb + 1u; k++) {
        const zt_copy_t cp = zt_copy(c, k);
        if (cp.kind == ZT_NONE) continue;
        if (cp.kind == ZT_CARRY && s->carry_block[cp.slot] != (int64_t)cp.block) { s->bad = 1; continue; } /* the slot last written */
        if (cp.to + cp.len > c->n || cp.from + cp.len > s->bs) { s->bad = 1; continue; }
        if (cp.block >= s->ctl.found) continue;
        const uint32_t n = zt_copy_bytes(&cp, st[cp.block], s->bs);
        const uint8_t* from = (cp.kind == ZT_SLOT ? s->slots + (size_t)cp.slot * s->sh.slot_stride : s->carry[cp.slot]) + cp.from;
        memcpy(d + cp.to, from, n);
    }
}

/* The chunk loop of tk_chunks (zxc_take_device.hip): the next n bytes, to d or (vchunk != NULL) into the table of a takev, whose
 * front end (plan, decode, copy of one chunk over the virtual destination vd) is takev_replay.h's. */
typedef void (*tr_vchunk_fn)(tr_session_t* s, const ztv_chunk_t* c, const void* vd);
static void tr_chunks(tr_session_t* s, uint8_t* d, tr_vchunk_fn vchunk, const void* vd, uint64_t n) {
    uint64_t left = n, v = 0;
    while (left) {
        const uint64_t m = zt_chunk_len(s->pos, left, s->max_piece, s->bs);
        if (m == 0 || m > left || m > s->max_piece || (m < left && (s->pos + m) % s->bs != 0)) { s->bad = 1; break; }
        ztv_chunk_t c;
        if (vchunk) {
            ztv_plan_chunk(s->pos, m, s->bs, s->cur, v, &c);
            vchunk(s, &c, vd);
        } else {
            zt_plan_chunk(s->pos, m, left, (uint32_t)((uintptr_t)(d + v) & 15u), s->bs, s->cur, &c.c);
            tr_chunk_decode(s, d + v, &c.c, left);
            tr_chunk_copy(s, d + v, &c.c);
        }
        zt_advance(&c.c, &s->pos, &s->cur);
        v += m; left -= m;
    }
}
/* zxc_mi355x_decompress_take_device: the next n bytes to d[0, n) -> ZXC_OK or the synchronous error */
static int tr_take(tr_session_t* s, uint8_t* d, uint64_t n) {
    if (n > s->cap - s->pos) return ZXC_ERROR_OVERFLOW;
    tr_chunks(s, d, NULL, NULL, n);
    return ZXC_OK;
}
/* zxc_mi355x_decompress_end_device -> the result word (TR_BAD_PLAN when the replay met a broken promise) */
static int64_t tr_end(tr_session_t* s) {
    if (s->pos < s->cap) return TR_BAD_PLAN; /* (the caller of the replay takes everything) */
    const uint32_t nj = s->sh.n_jobs;
    if (s->cap > 0) {
        zt_chunk_t c;
        zt_plan_extra(nj - 1u, s->bs, s->cur, &c);
        tr_chunk_decode(s, NULL, &c, 0);
        for (uint32_t i = 0; i < nj; i++) if (s->decoded[i] != 1) s->bad = 1;
        if (!s->ctl.final) {
            const int32_t* st = s->status + (size_t)s->ctl.sel * nj;
            for (uint32_t i = 0; i < s->ctl.found; i++) {
                const int32_t ev = zc_block_event(i, st[i], s->ctl.found, s->ctl.done, s->bs, s->cap);
                if (ev != 0 && zc_event_key(i, ev) < s->ctl.event) s->ctl.event = zc_event_key(i, ev);
            }
        }
    }
    const int32_t last = (!s->ctl.final && s->ctl.found) ? s->status[(size_t)s->ctl.sel * nj + s->ctl.found - 1u] : 0;
    const int64_t r = zc_verdict(&s->ctl, last, s->bs);
    return s->bad ? TR_BAD_PLAN : r;
}

/* A heap buffer for n bytes with at least TR_GUARD canary bytes in front and behind, its first byte at an address that is
 * `align` mod 16 -> that byte; *raw is what to free. And whether a canary around d[0, n) changed. */
static uint8_t* tr_guarded(uint64_t n, uint32_t align, uint8_t** raw) {
    *raw = malloc(TR_GUARD + 16u + n + TR_GUARD + 16u);
    memset(*raw, TR_CANARY, TR_GUARD + 16u + n + TR_GUARD + 16u);
    return (uint8_t*)(((uintptr_t)*raw + TR_GUARD + 15u) & ~(uintptr_t)15u) + (align & 15u);
}
static int tr_guards_changed(const uint8_t* raw, const uint8_t* d, uint64_t n) {
    int bad = 0;
    for (const uint8_t* p = raw; p < d; p++) if (*p != TR_CANARY) bad = 1;
    for (const uint8_t* p = d + n; p < raw + TR_GUARD + 16u + n + TR_GUARD + 16u; p++) if (*p != TR_CANARY) bad = 1;
    return bad;
}

/* A whole session: begin, the takes of lens[0 .. n_lens) (their sum is cap), end. Every piece is a heap buffer of its own with
 * at least TR_GUARD canary bytes in front and behind, its first byte at an address that is `align` mod 16 (the sanitizer program
 * also hands tr_take buffers of exactly n bytes). out[0, cap) receives the pieces' bytes concatenated. -> the result word, or
 * TR_BAD_PLAN also when a canary changed. */
static int64_t tr_session(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, int want_verify, int use_table,
                          int have_dict, uint32_t dict_id, const uint8_t* blk_bytes, const uint64_t* blk_at, const int32_t* blk_status,
                          uint32_t n_blocks, const uint64_t* lens, uint32_t n_lens, uint32_t align, uint8_t* out) {
    tr_session_t s;
    memset(&s, 0, sizeof s);
    s.blk_bytes = blk_bytes; s.blk_at = blk_at; s.blk_status = blk_status; s.n_blocks = n_blocks;
    const int rc = tr_begin(&s, src, src_size, cap, max_piece, bs, want_verify, use_table, have_dict, dict_id);
    if (rc != 0) return rc;
    uint64_t at = 0;
    int canary_bad = 0;
    for (uint32_t i = 0; i < n_lens; i++) {
        const uint64_t n = lens[i];
        uint8_t* raw;
        uint8_t* d = tr_guarded(n, align, &raw);
        if (tr_take(&s, d, n) != ZXC_OK) s.bad = 1;
        canary_bad |= tr_guards_changed(raw, d, n);
        if (at + n <= cap) memcpy(out + at, d, n);
        at += n;
        free(raw);
    }
    const int64_t r = (s.pos == cap && at == cap) ? tr_end(&s) : TR_BAD_PLAN;
    tr_free(&s);
    return canary_bad ? TR_BAD_PLAN : r;
}

/* The promises of one chunk's plan, for n > 0 bytes at position pos of a take with room >= n bytes left, delivered to an address
 * that is `align` mod 16, with J = max_piece / bs + 2: -> 0, or the number of the promise it breaks. */
static int tr_plan_check(uint64_t pos, uint64_t n, uint64_t room, uint32_t align, uint32_t bs, uint64_t max_piece) {
    zt_chunk_t c;
    zt_plan_chunk(pos, n, room, align & 15u, bs, 0u, &c);
    const uint64_t J = max_piece / bs + 2u;
    if (c.nb != c.whole + (c.tail ? 1u : 0u) || (uint64_t)c.head + (uint64_t)c.whole * bs + c.tail != n) return 1;
    if (c.nb > J || c.whole - c.n_direct > J) return 2; /* jobs and slots of a chunk */
    if (c.head && (c.head_at != pos % bs || c.head_at + c.head > bs)) return 3;
    if (!c.head && c.nb && pos % bs != 0) return 3;
    if (c.nb && c.first != (pos + c.head) / bs) return 4;
    if (c.swap != (c.tail ? 1u : 0u)) return 5;
    /* every byte of d[0, n) once: the head copy, then per job a direct block or a copy, in order */
    uint64_t at = 0;
    for (uint32_t k = 0; k < c.nb + 1u; k++) {
        const zt_copy_t cp = zt_copy(&c, k);
        if (k > 0) {
            const zt_place_t p = zt_job_place(&c, k - 1u);
            if (p.kind == ZT_DIRECT) {
                if (cp.kind != ZT_NONE || p.at != at) return 6;
                if (((align + p.at) & 15u) != 0 || p.at + bs + ZT_SPILL > room || p.at + bs > n) return 7; /* the direct rule */
                at += bs;
                continue;
            }
            if (p.kind == ZT_SLOT && (cp.kind != ZT_SLOT || cp.slot != p.slot || cp.slot >= J || cp.len != bs || cp.from != 0)) return 8;
            if (p.kind == ZT_CARRY && (cp.kind != ZT_CARRY || cp.slot != 1u || cp.len != c.tail || cp.from != 0 || k != c.nb)) return 9;
            if (cp.block != c.first + k - 1u) return 10;
            /* a whole block that could go straight does: aligned, and its slot + 32 inside the take */
            if (p.kind == ZT_SLOT && ((align + cp.to) & 15u) == 0 && cp.to + bs + ZT_SPILL <= room) return 11;
        } else if (cp.kind != ZT_NONE && (cp.kind != ZT_CARRY || cp.slot != 0u || cp.from != c.head_at || cp.len != c.head || cp.block != pos / bs)) return 12;
        if (cp.kind == ZT_NONE) continue;
        if (cp.to != at) return 13;
        at += cp.len;
    }
    if (at != n) return 14;
    return 0;
}
#endif
