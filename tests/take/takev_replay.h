/* Test-only: zxc_mi355x_decompress_takev_device replayed on the host the way its entry point and the kernels of
 * zxc_take_device.hip run it (zxc_amd/csrc/zxc_takev.h), on top of the session of take_replay.h, so that take and takev mix in one
 * session: the scan in series, the fold of the verdict, and per chunk the plan of every job (ztv_job_place), the stand-in decoder
 * of take_replay.h, which scribbles 32 bytes behind every block, and the copy of every (copy, 8 KiB, lane): a range inside one
 * entry as one copy (zd_copy_chunk is the take session's, not under test), a range that meets an entry boundary through
 * ztv_scatter_lane for every lane. The decode launch's base is the slots' address, so that the out_off of a block decoded in its
 * entry wraps modulo 2^64 as on the device whenever the entry lies below.
 * Shared by takev_shim.c (loaded by tests/test_decompress_takev_device_cpu.py) and takev_san_main.c (a program of its own). */
#ifndef TAKEV_REPLAY_H
#define TAKEV_REPLAY_H
#include "take_replay.h"

/* plan kernel and decode launches of one chunk */
static void tvr_chunk_decode(tr_session_t* s, const ztv_chunk_t* c, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov,
                             int verdict, ztv_place_t* places) {
    const uint32_t nj = s->sh.n_jobs, J = s->sh.J;
    const zt_chunk_t* z = &c->c;
    const uint64_t out_base = (uint64_t)(uintptr_t)s->slots;
    if (z->nb > J || z->first + z->nb > nj || z->n_direct != 0) { s->bad = 1; return; }
    for (uint32_t j = 0; j < z->nb; j++) {
        const uint64_t slot_j = (uint64_t)(uintptr_t)(s->slots + (size_t)j * s->sh.slot_stride);
        if (verdict < 0 || s->ctl.final) { /* every job empty; neither the table nor an entry is read */
            const zxc_dev_job_t empty = {0u, slot_j - out_base, 0u, s->bs};
            const ztv_place_t none = {ZT_NONE, 0u, 0u};
            for (uint32_t tb = 0; tb < s->tables; tb++) s->cjobs[(size_t)tb * J + j] = empty;
            places[j] = none;
            continue;
        }
        uint64_t addr = 0;
        places[j] = ztv_job_place(c, j, iov, starts, n_iov, (uint64_t)(uintptr_t)s->carry[0], (uint64_t)(uintptr_t)s->carry[1],
                                  (uint64_t)(uintptr_t)s->slots, s->sh.slot_stride, &addr);
        const ztv_place_t rec = places[j];
        if (rec.r >= n_iov) { s->bad = 1; continue; }
        if (rec.kind == ZT_DIRECT) { /* the promise of the in-place rule: aligned, the block and the spill inside that one entry */
            const uint64_t off = addr - iov[rec.r].base;
            if ((addr & 15u) != 0 || j >= z->whole || addr < iov[rec.r].base || off + s->bs + ZT_SPILL > iov[rec.r].len) s->bad = 1;
        } else if (rec.kind == ZT_SLOT) {
            if (j >= z->whole || addr != slot_j) s->bad = 1;
        } else if (rec.kind == ZT_CARRY) {
            if (j != z->whole || addr != (uint64_t)(uintptr_t)s->carry[z->cur ^ 1u]) s->bad = 1;
        } else s->bad = 1;
        for (uint32_t tb = 0; tb < s->tables; tb++) {
            zxc_dev_job_t job = s->jobs[(size_t)tb * nj + z->first + j];
            job.out_off = addr - out_base;
            s->cjobs[(size_t)tb * J + j] = job;
        }
    }
    for (uint32_t tb = 0; tb < s->tables; tb++)
        for (uint32_t j = 0; j < z->nb; j++) {
            const zxc_dev_job_t* job = &s->cjobs[(size_t)tb * J + j];
            if ((job->out_off & 15u) != 0) s->bad = 1;
            if (j == z->whole) s->carry_block[z->cur ^ 1u] = (int64_t)(z->first + j);
            s->status[(size_t)tb * nj + z->first + j] = tr_decode(s, job, z->first + j, (uint8_t*)(uintptr_t)(out_base + job->out_off));
            if (tb == 0 && s->decoded[z->first + j]++ != 0) s->bad = 1; /* every block once */
        }
}
/* ... and its copy kernel behind them: every (copy, 8 KiB, lane) */
static void tvr_chunk_copy(tr_session_t* s, const ztv_chunk_t* c, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int verdict,
                           const ztv_place_t* places) {
    if (verdict < 0 || s->ctl.final) return;
    const zt_chunk_t* z = &c->c;
    const int32_t* st = s->status + (size_t)s->ctl.sel * s->sh.n_jobs;
    for (uint32_t k = 0; k < z->nb + 1u; k++)
        for (uint32_t ch = 0; ch < s->sh.copy_chunks; ch++)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const zt_copy_t cp = zt_copy(z, k);
                if (cp.kind == ZT_NONE) continue;
                if (cp.kind == ZT_CARRY && s->carry_block[cp.slot] != (int64_t)cp.block) { s->bad = 1; continue; } /* the slot last written */
                if (cp.to + cp.len > z->n || cp.from + cp.len > s->bs) { s->bad = 1; continue; }
                if (cp.block >= s->ctl.found) continue;
                const ztv_place_t* rec = k ? places + (k - 1u) : NULL;
                if (rec && rec->kind != cp.kind) { if (rec->kind != ZT_DIRECT) s->bad = 1; continue; }
                const uint32_t n = zt_copy_bytes(&cp, st[cp.block], s->bs);
                if (n == 0 || (uint64_t)ch * ZT_COPY_CHUNK >= (uint64_t)n + 15u) continue;
                const ztv_copy_t o = ztv_copy_place(c, &cp, n, rec, iov, starts, n_iov);
                const uint8_t* from = (cp.kind == ZT_SLOT ? s->slots + (size_t)cp.slot * s->sh.slot_stride : s->carry[cp.slot]) + cp.from;
                if (o.one) {
                    if (ch == 0 && lane == 0) memcpy((uint8_t*)(uintptr_t)o.d, from, n);
                    continue;
                }
                ztv_scatter_lane(from, n, o.y, ch, lane, iov, starts, o.e_lo, n_iov);
            }
}

/* The front end tr_chunks calls per chunk of a takev: the table, what the call's scan left, the verdict, the place records. */
typedef struct tvr_dst {
    const zxc_dev_iov_t* iov;
    const uint64_t* starts;
    uint32_t n_iov;
    int verdict;
    ztv_place_t* places;
} tvr_dst_t;
static void tvr_chunk(tr_session_t* s, const ztv_chunk_t* c, const void* dst) {
    const tvr_dst_t* vd = dst;
    tvr_chunk_decode(s, c, vd->iov, vd->starts, vd->n_iov, vd->verdict, vd->places);
    tvr_chunk_copy(s, c, vd->iov, vd->starts, vd->n_iov, vd->verdict, vd->places);
}

/* zxc_mi355x_decompress_takev_device behind its pointer checks: the next `total` bytes into the table -> ZXC_OK or the
 * synchronous error. The table lies in host memory here; starts and the place records are heap buffers of exactly the sizes the
 * scratch gives them. */
static int tvr_takev(tr_session_t* s, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total) {
    if (n_iov == 0 && total > 0) return ZXC_ERROR_DST_TOO_SMALL;
    if (total > s->cap - s->pos) return ZXC_ERROR_OVERFLOW;
    ztv_shape_t vsh;
    if (ztv_shape(n_iov, s->max_piece, s->bs, &vsh) != 0 || vsh.J != s->sh.J) { s->bad = 1; return ZXC_ERROR_NULL_INPUT; }
    if (n_iov == 0) return ZXC_OK;
    uint64_t* starts = malloc(((size_t)n_iov + 1u) * 8u);
    ztv_place_t* places = malloc((size_t)vsh.J * sizeof *places);
    const tvr_dst_t vd = {iov, starts, n_iov, ztv_scan_serial(iov, n_iov, total, starts), places};
    ztv_fold(&s->ctl, vd.verdict);
    tr_chunks(s, NULL, tvr_chunk, &vd, total);
    free(places); free(starts);
    return ZXC_OK;
}

/* A whole session that mixes take and takev: begin, the calls, end. Call i delivers the next sum of lens[at_i .. at_i + cnt_i)
 * bytes: cnt_i == 0xFFFFFFFF is a take of lens[at_i] bytes (at_i advances by one), else a takev over a table of those cnt_i
 * entries. Every entry and every piece is a heap buffer of its own with at least TR_GUARD canary bytes in front and behind, its
 * first byte at an address that is `align` mod 16 (align >= 16: entry e at (e * 7) mod 16). out[0, cap) receives the bytes
 * concatenated. -> the result word, or TR_BAD_PLAN also when a canary changed. */
#define TVR_TAKE 0xFFFFFFFFu
static int64_t tvr_session(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, int want_verify, int use_table,
                           int have_dict, uint32_t dict_id, const uint8_t* blk_bytes, const uint64_t* blk_at, const int32_t* blk_status,
                           uint32_t n_blocks, const uint64_t* lens, const uint32_t* calls, uint32_t n_calls, uint32_t align, uint8_t* out) {
    tr_session_t s;
    memset(&s, 0, sizeof s);
    s.blk_bytes = blk_bytes; s.blk_at = blk_at; s.blk_status = blk_status; s.n_blocks = n_blocks;
    const int rc = tr_begin(&s, src, src_size, cap, max_piece, bs, want_verify, use_table, have_dict, dict_id);
    if (rc != 0) return rc;
    uint64_t at = 0;
    uint32_t e = 0;
    int canary_bad = 0;
    for (uint32_t i = 0; i < n_calls; i++) {
        const uint32_t cnt = calls[i] == TVR_TAKE ? 1u : calls[i];
        uint8_t** raw = malloc(((size_t)cnt + 1u) * sizeof *raw);
        zxc_dev_iov_t* iov = malloc(((size_t)cnt + 1u) * sizeof *iov);
        uint64_t total = 0;
        for (uint32_t r = 0; r < cnt; r++) {
            const uint64_t n = lens[e + r];
            const uint32_t a = align >= 16u ? ((e + r) * 7u) & 15u : align;
            iov[r].base = (uint64_t)(uintptr_t)tr_guarded(n, a, &raw[r]);
            iov[r].len = n;
            total += n;
        }
        if (calls[i] == TVR_TAKE) { if (tr_take(&s, (uint8_t*)(uintptr_t)iov[0].base, total) != ZXC_OK) s.bad = 1; }
        else if (tvr_takev(&s, iov, cnt, total) != ZXC_OK) s.bad = 1;
        for (uint32_t r = 0; r < cnt; r++) {
            uint8_t* d = (uint8_t*)(uintptr_t)iov[r].base;
            const uint64_t n = iov[r].len;
            canary_bad |= tr_guards_changed(raw[r], d, n);
            if (at + n <= cap) memcpy(out + at, d, n);
            at += n;
            free(raw[r]);
        }
        e += cnt;
        free(iov); free(raw);
    }
    const int64_t r = (s.pos == cap && at == cap) ? tr_end(&s) : TR_BAD_PLAN;
    tr_free(&s);
    return canary_bad ? TR_BAD_PLAN : r;
}

/* The in-place rule against a plain walk over the entries: a call of n_iov entries (bases and lengths given; a base of 0 stands
 * for "not looked at": only legal with len 0) at decoded position pos, cut into chunks of at most max_piece. For every whole block
 * of every chunk: it goes direct exactly when its first byte's address is 16-byte aligned and the block and 32 bytes more lie
 * inside the entry that a linear walk finds for its first byte; else to slot j. -> 0, or (block number + 1) << 8 | the promise. */
static uint64_t tvr_rule_check(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t pos, uint64_t max_piece, uint32_t bs) {
    uint64_t* starts = malloc(((size_t)n_iov + 1u) * 8u);
    uint64_t total = 0, bad = 0;
    for (uint32_t r = 0; r < n_iov; r++) total += iov[r].len;
    if (ztv_scan_serial(iov, n_iov, total, starts) != 0) { free(starts); return 1; }
    uint64_t left = total, v = 0;
    uint32_t cur = 0;
    while (left && !bad) {
        const uint64_t m = zt_chunk_len(pos, left, max_piece, bs);
        ztv_chunk_t c;
        ztv_plan_chunk(pos, m, bs, cur, v, &c);
        if (c.c.nb + 1u > max_piece / bs + 2u) bad = 2;
        for (uint32_t j = 0; j < c.c.nb && !bad; j++) {
            uint64_t addr = 0;
            const ztv_place_t rec = ztv_job_place(&c, j, iov, starts, n_iov, 0x1000u, 0x2000u, 0x100000u, bs + ZT_SLOT_PAD, &addr);
            const uint64_t y = v + c.c.head + (uint64_t)j * bs;
            uint32_t r = 0;
            uint64_t lo = 0;
            while (lo + iov[r].len <= y) lo += iov[r++].len; /* the plain walk: the entry that holds byte y */
            const uint64_t key = (c.c.first + j + 1u) << 8;
            if (rec.r != r) { bad = key | 3u; break; }
            if (j == c.c.whole) { if (rec.kind != ZT_CARRY || addr != (c.c.cur ? 0x1000u : 0x2000u)) bad = key | 4u; continue; }
            const int fits = ((iov[r].base + (y - lo)) & 15u) == 0 && (y - lo) + bs + 32u <= iov[r].len;
            if (fits && (rec.kind != ZT_DIRECT || addr != iov[r].base + (y - lo))) bad = key | 5u; /* one that could go direct does */
            if (!fits && (rec.kind != ZT_SLOT || addr != 0x100000u + (uint64_t)j * (bs + ZT_SLOT_PAD))) bad = key | 6u;
        }
        zt_advance(&c.c, &pos, &cur);
        v += m; left -= m;
    }
    free(starts);
    return bad;
}
#endif
