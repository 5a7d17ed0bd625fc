/* Test-only: zxc_mi355x_compress_appendv_dict_device replayed on the host on top of append_dict_replay.h and appendv_replay.h, the
 * way the entry point and the kernels of zxc_append_device.hip run it: the scan of the table into a scratch that holds no images
 * (zav_shape_dict), the chunk loop, per chunk the launches over at most `chunk` jobs with every workgroup and thread of
 * zav_prep_images (the very lines zxc_appendv_images_kernel runs), the stand-in encoder over the images, the predicated back half.
 * A chunk that completes no block goes through zav_prep, as on the device. Every entry of a table is a heap buffer of exactly its
 * length, the table, the scratch and the image area heap buffers of exactly their sizes, so a sanitizer sees any read or write
 * outside them. Every image is checked before the stand-in encoder runs: the dictionary in front, the bytes of its block behind.
 * Shared by appendv_dict_shim.c (loaded by tests/test_compress_appendv_dict_device_cpu.py) and appendv_dict_san_main.c. */
#ifndef APPENDV_DICT_REPLAY_H
#define APPENDV_DICT_REPLAY_H
#include "append_dict_replay.h"
#include "appendv_replay.h"

typedef struct rpvd_stats {
    rpv_stats_t v;       /* images: jobs the stand-in encoder took; carried: those that began in the carry area; bytes_read: by it */
    uint64_t max_chunks; /* the most launches one chunk of a call took */
    uint64_t tails;      /* tail workgroups run */
    uint64_t unused;     /* unused jobs met (after a table error) */
} rpvd_stats_t;

/* One chunk behind its plan, the front end of a dictionary session's appendv (ap_piece with a virtual source). */
static void rpvd_chunk(rpd_session_t* d, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, const zav_chunk_t* c,
                       rpvd_stats_t* st) {
    rp_session_t* s = &d->r;
    const zap_piece_t* p = &c->p;
    uint8_t *carry = s->area[s->cur], *next = s->area[s->cur ^ 1u];
    if (!p->nb) { /* joins the carry: zxc_appendv_prep_kernel as it is, one workgroup, no image */
        for (uint32_t t = 0; t < RPV_THREADS; t++) zav_prep(iov, starts, n_iov, status, c, 0u, t, RPV_THREADS, carry, next, NULL, 0u, s->jobs);
        return;
    }
    if (p->nb > s->sh.J || p->n_staged || p->cp[0].area != ZAP_SRC || p->cp[1].area != ZAP_SRC || p->cp[2].area != ZAP_NEXT) { s->bad = 1; return; }
    const uint64_t first_block = s->total / s->bs, image = d->shi.image;
    uint64_t chunks = 0;
    for (uint32_t j0 = 0; j0 < p->nb; j0 += d->chunk, chunks++) {
        const uint32_t n = p->nb - j0 < d->chunk ? p->nb - j0 : d->chunk, groups = n + (j0 == 0 ? 1u : 0u);
        memset(s->jobs + j0, 0xEE, n * sizeof(zxc_enc_job_t)); /* every job of the launch must be written */
        memset(d->images, 0xEE, (size_t)n * image);
        for (uint32_t w = 0; w < groups; w++) /* zxc_appendv_images_kernel */
            for (uint32_t t = 0; t < RPV_THREADS; t++)
                zav_prep_images(iov, starts, n_iov, status, c, j0, n, w, t, RPV_THREADS, d->dict, d->dict_size, carry, next, d->images, s->jobs);
        if (j0 == 0 && status >= 0) { /* the tail and its padding, once */
            st->tails++;
            if (memcmp(next, s->src + s->total + p->n - p->tail, p->tail) != 0) s->bad = 1;
            for (uint32_t k = 0; k < ZAP_PAD; k++) if (next[p->tail + k] != 0) s->bad = 1;
        }
        if (j0 != 0) { /* a later launch has no workgroup n, and the rule gives one nothing to do: the tail area stays */
            memset(next, 0xEE, (size_t)p->tail + ZAP_PAD);
            for (uint32_t t = 0; t < RPV_THREADS; t++)
                zav_prep_images(iov, starts, n_iov, status, c, j0, n, n, t, RPV_THREADS, d->dict, d->dict_size, carry, next, d->images, s->jobs);
            for (uint32_t k = 0; k < p->tail + ZAP_PAD; k++) if (next[k] != 0xEE) s->bad = 1;
            if (status >= 0) { /* (put back what the first launch left) */
                memcpy(next, s->src + s->total + p->n - p->tail, p->tail);
                memset(next + p->tail, 0, ZAP_PAD);
            }
        }
        for (uint32_t w = 0; w < n; w++) { /* the encode launch over jobs + j0, slots + j0 x stride, sizes + j0 */
            const zxc_enc_job_t job = s->jobs[j0 + w];
            if (status < 0) { /* the unused job, and nothing built */
                if (job.src_off != 0 || job.len != 0 || job.pad != 0 || d->images[w * image] != 0xEE) s->bad = 1;
                st->unused++;
                continue;
            }
            const uint8_t* in = d->images + job.src_off;
            const uint64_t k = first_block + j0 + w;
            if (job.src_off != w * image || job.len != s->bs) { s->bad = 1; continue; }
            if (job.src_off + d->dict_size + job.len + ZAP_OVERREAD > (uint64_t)n * image + ZC_IMAGE_PAD) s->bad = 1; /* the over-read */
            /* the image, before the stand-in encoder runs: [dict | the block's bytes] */
            if (k >= s->n_blocks || memcmp(in, d->dict, d->dict_size) != 0 || memcmp(in + d->dict_size, s->src + k * s->bs, s->bs) != 0) {
                s->bad = 1;
                s->sizes[j0 + w] = 0;
                continue;
            }
            rpv_touch(in, (uint64_t)d->dict_size + job.len, &st->v);
            st->v.images++;
            if (p->carry && j0 + w == 0) st->v.carried++;
            if (!rp_encode_job(s, j0 + w, k, in + d->dict_size, job.len)) s->sizes[j0 + w] = 0;
        }
    }
    if (chunks > st->max_chunks) st->max_chunks = chunks;
    if (status >= 0) rp_back(s, p->nb); /* the advance is not run after a table error; scatter and gather see the session's error */
}

/* zxc_mi355x_compress_appendv_dict_device behind its synchronous checks: the table iov[0 .. n_iov) (host addresses) and the
 * caller's promise `total`. -> the table's verdict. */
static int rpvd_appendv_table(rpd_session_t* d, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, rpvd_stats_t* st) {
    rp_session_t* s = &d->r;
    zav_shape_t vsh;
    if (zav_shape_dict(n_iov, s->max_piece, s->bs, d->dict_size, &vsh) != 0 || n_iov == 0) { s->bad = 1; return 0; }
    if (vsh.bytes > zav_scratch_bound_dict(n_iov, s->max_piece, s->bs, d->dict_size)) s->bad = 1;
    uint8_t* alloc = malloc(RPV_ODD + vsh.bytes + RPV_CANARY_BYTES); /* scratch_size bytes at an odd address, a canary behind them */
    memset(alloc, RPV_CANARY, RPV_ODD + vsh.bytes + RPV_CANARY_BYTES);
    uint8_t* sb = (uint8_t*)zc_round_up((uint64_t)(uintptr_t)(alloc + RPV_ODD), 256u);
    if (sb + vsh.bytes - 256u > alloc + RPV_ODD + vsh.bytes) s->bad = 1; /* the layout fits scratch_size from any alignment */
    if (vsh.o_tile_flags + 4ull * vsh.n_tiles > vsh.bytes - 256u) s->bad = 1;
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + vsh.o_starts);
    vctl->status = zav_scan_serial(iov, n_iov, total, starts); /* the three scan kernels */
    vctl->sum = starts[n_iov];
    zav_fold_status(&s->ctl, vctl->status);
    uint64_t left = total, v = 0, m;
    while (left && rp_next_piece(s, left, &m)) {
        zav_chunk_t c;
        zap_plan_piece_images((uint32_t)(s->total % s->bs), m, s->bs, &c.p); /* ap_pieces: the plan of a dictionary session */
        c.v = v;
        rpvd_chunk(d, iov, starts, n_iov, vctl->status, &c, st);
        s->total += m;
        if (c.p.swap) s->cur ^= 1u;
        v += m; left -= m;
    }
    for (uint32_t k = 0; k < RPV_CANARY_BYTES; k++) if (alloc[RPV_ODD + vsh.bytes + k] != RPV_CANARY) s->bad = 1;
    for (uint32_t k = 0; k < RPV_ODD; k++) if (alloc[k] != RPV_CANARY) s->bad = 1;
    const int status = vctl->status;
    free(alloc);
    return status;
}

/* An appendv_dict of the next sum(lens) bytes of the session's source: entry r is a heap copy of exactly lens[r] bytes; an empty
 * entry has a base that must not be looked at (0, or an address nothing lies at). */
static void rpvd_appendv(rpd_session_t* d, const uint64_t* lens, uint32_t n_iov, rpvd_stats_t* st) {
    rp_session_t* s = &d->r;
    uint64_t total = 0;
    for (uint32_t r = 0; r < n_iov; r++) total += lens[r];
    if (n_iov == 0) return; /* (total == 0: ZXC_OK, nothing enqueued) */
    zxc_dev_iov_t* iov = malloc(n_iov * sizeof *iov); /* exactly the table */
    uint64_t at = s->total;
    for (uint32_t r = 0; r < n_iov; r++) {
        iov[r].len = lens[r];
        iov[r].base = (r & 1u) ? 0u : 0x10u;
        if (lens[r]) {
            uint8_t* e = malloc(lens[r]);
            memcpy(e, s->src + at, lens[r]);
            iov[r].base = (uint64_t)(uintptr_t)e;
            at += lens[r];
        }
    }
    if (rpvd_appendv_table(d, iov, n_iov, total, st) != 0) s->bad = 1; /* a valid table */
    for (uint32_t r = 0; r < n_iov; r++) if (lens[r]) free((void*)(uintptr_t)iov[r].base);
    free(iov);
}

/* A whole dictionary session: begin, then call i appends lens[at_i .. at_i + counts[i]) bytes: counts[i] > 0: one appendv_dict
 * over that many entries; counts[i] == 0: one plain append of lens[at_i] bytes (which takes one length). Then end. chunk: jobs per
 * launch (0: the shape's). */
static int64_t rpvd_session(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                            uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, const uint32_t* counts,
                            uint32_t n_calls, uint64_t max_piece, uint8_t* dst, uint64_t cap, const uint8_t* dict, uint32_t dict_size,
                            uint32_t dict_id, uint32_t chunk, rpvd_stats_t* st) {
    rpd_session_t d;
    memset(&d, 0, sizeof d);
    d.r.src = src; d.r.blocks = blocks; d.r.blk_at = blk_at; d.r.blk_size = blk_size; d.r.n_blocks = n_blocks;
    const int rc = rpd_begin(&d, total, max_piece, bs, checksum, seekable, dst, cap, dict, dict_size, dict_id, chunk);
    if (rc != 0) return rc;
    for (uint32_t i = 0; i < n_calls; i++) {
        if (counts[i]) { rpvd_appendv(&d, lens, counts[i], st); lens += counts[i]; }
        else { rpd_append(&d, lens[0]); lens += 1; }
    }
    const int64_t r = d.r.total == total ? rpd_end(&d) : RP_BAD_PLAN;
    rpd_free(&d);
    return r;
}

/* ---- the cut sets: the calls of one session over `total` bytes of blocks of bs. lens[] and, per call, counts[] (0: a plain
 * append of one length). Both arrays hold total + 4096 elements. -> 0 for a pattern past the last. */
#define RPVD_PATTERNS 9
static uint32_t rpvd_rnd_state;
static uint32_t rpvd_rnd(void) { rpvd_rnd_state = rpvd_rnd_state * 1664525u + 1013904223u; return rpvd_rnd_state >> 8; }
static int rpvd_calls(int pattern, uint64_t total, uint32_t bs, uint64_t* lens, uint32_t* n_lens, uint32_t* counts, uint32_t* n_calls,
                      uint64_t* max_piece) {
    uint64_t left = total;
    uint32_t nl = 0, nc = 0;
    *max_piece = total > bs ? total : bs;
#define ENTRY(n) do { uint64_t n_ = (n); if (n_ > left) n_ = left; lens[nl++] = n_; left -= n_; } while (0)
#define APPEND(n) do { ENTRY(n); counts[nc++] = 0; } while (0)
#define TABLE(first) do { if (nl > (first)) counts[nc++] = nl - (first); } while (0)
    if (pattern == 0) { ENTRY(total); counts[nc++] = 1; }                 /* one entry, no carry, one chunk over everything */
    else if (pattern == 1 || pattern == 2 || pattern == 3) {              /* the entry lengths, behind a carry of 0, 1, bs - 1 */
        const uint32_t carry = pattern == 1 ? 0u : pattern == 2 ? 1u : bs - 1u;
        if (carry) APPEND(carry);
        const uint32_t first = nl;
        const uint64_t each[] = {0u, 1u, 3u, 15u, 16u, 17u, 0u, bs - 1u, bs, bs + 1u, 0u, 0u, 17u, 16u, 15u, bs + 1u, bs, bs - 1u, 3u, 1u, 0u};
        for (unsigned i = 0; i < sizeof each / sizeof each[0]; i++) ENTRY(each[i]);
        for (uint32_t i = 0; i < 3000u && left; i++) ENTRY(1u);             /* thousands of 1-byte entries */
        ENTRY(left); lens[nl++] = 0;
        TABLE(first);
        if (pattern == 3) *max_piece = 2ull * bs;
    } else if (pattern == 4) {                                            /* call boundaries inside a block, on a boundary, one to either side */
        uint32_t first = nl;
        ENTRY(bs / 3u); ENTRY(7u); TABLE(first);                            /* ends inside a block */
        first = nl; ENTRY(1u); ENTRY(0u); ENTRY(2u); TABLE(first);          /* wholly inside one block */
        first = nl; ENTRY(bs - bs / 3u - 10u); TABLE(first);                /* ends on a block boundary */
        first = nl; ENTRY(bs); ENTRY(1u); TABLE(first);                     /* ends one byte behind one */
        first = nl; ENTRY(bs - 2u); TABLE(first);                           /* ... one byte in front of one */
        APPEND(1u);                                                         /* a plain append completes the block */
        first = nl; ENTRY(bs - 1u); TABLE(first);
        APPEND(2u);                                                         /* ... and one crosses the boundary */
        first = nl; ENTRY(2u * bs - 1u); TABLE(first);
        first = nl; ENTRY(3u); ENTRY(left); TABLE(first);
        *max_piece = 2ull * bs;
    } else if (pattern == 5 || pattern == 6) {                            /* append, appendv_dict, append, ...: a carry each */
        for (int call = 0; left; call++) {
            if (call % 2 == 0) APPEND(1u + rpvd_rnd() % (bs + bs / 2u));
            else {
                const uint32_t first = nl;
                uint64_t want = bs / 3u + rpvd_rnd() % (3u * bs);
                while (left && want) { uint64_t n = rpvd_rnd() % 3u ? rpvd_rnd() % 40u : rpvd_rnd() % (2u * bs); if (n > want) n = want; want -= n; ENTRY(n); }
                TABLE(first);
            }
        }
        *max_piece = pattern == 5 ? 2ull * bs : bs;
    } else if (pattern == 7) {                                            /* one table of random entries: one chunk, many launches */
        APPEND(5u);
        const uint32_t first = nl;
        lens[nl++] = 0;
        while (left) { const uint32_t k = rpvd_rnd() % 5u; ENTRY(k == 0 ? 0u : k == 1 ? 1u + rpvd_rnd() % 7u : k == 2 ? rpvd_rnd() % bs : rpvd_rnd() % (3u * bs + 9u)); }
        lens[nl++] = 0;
        TABLE(first);
    } else if (pattern == 8) {                                            /* two tables back to back, the second all tiny */
        uint32_t first = nl;
        ENTRY(total / 2u + 17u); ENTRY(0u); TABLE(first);
        first = nl;
        while (left) ENTRY(1u + rpvd_rnd() % 7u);
        TABLE(first);
        *max_piece = 2ull * bs + 100u;
    } else return 0;
#undef TABLE
#undef APPEND
#undef ENTRY
    if (left) return 0;
    *n_lens = nl; *n_calls = nc;
    return 1;
}

/* comp: an archive as rpd_cut takes it; data: its total decoded bytes. One session per cut set (rpvd_calls), with room behind the archive; every
 * other one also with a capacity of exactly the archive and of one byte less: the archive byte for byte, the pattern intact
 * everywhere outside it. chunk: jobs per launch (0: the shape's). -> the number of sessions, or minus the line that failed.
 * *all adds up what the sessions saw. */
static int64_t rpvd_check_archive(const uint8_t* comp, uint64_t comp_size, const uint8_t* data, uint64_t total, const uint8_t* dict,
                                  uint32_t dict_size, uint32_t seed, uint32_t chunk, rpvd_stats_t* all) {
    rpd_arc_t a;
    int64_t result = rpd_cut(comp, comp_size, total, &a);
    uint64_t* lens = malloc((total + 4096u) * 8u);
    uint32_t* counts = malloc((total + 4096u) * 4u);
    rpvd_rnd_state = seed;
    for (int pattern = 0; pattern < RPVD_PATTERNS && result >= 0; pattern++) {
        uint32_t n_lens = 0, n_calls = 0;
        uint64_t max_piece = 0;
        if (!rpvd_calls(pattern, total, a.bs, lens, &n_lens, counts, &n_calls, &max_piece)) { result = -__LINE__; break; }
        for (int run = 0; run < (pattern % 2 ? 3 : 1) && result >= 0; run++) {
            const uint64_t cap = run == 0 ? comp_size + 33u : comp_size - (uint64_t)(run - 1), room = run == 0 ? comp_size + 97u : cap + 64u;
            uint8_t* dst = malloc(room);
            memset(dst, RPD_CANARY, room);
            rpvd_stats_t st;
            memset(&st, 0, sizeof st);
            const int64_t rc = rpvd_session(data, total, a.blocks, a.blk_at, a.blk_size, a.nb, a.bs, (int)a.ck, a.seekable, lens, counts, n_calls,
                                            max_piece, dst, cap, dict, dict_size, a.id, chunk, &st);
            int line = 0;
            if (run < 2) {
                if (!(rc == (int64_t)comp_size && memcmp(dst, comp, comp_size) == 0)) line = __LINE__;
                for (uint64_t i = comp_size; i < room && !line; i++) if (dst[i] != RPD_CANARY) line = __LINE__;
            } else {
                if (rc != ZXC_ERROR_DST_TOO_SMALL) line = __LINE__;
                for (uint64_t i = cap; i < room && !line; i++) if (dst[i] != RPD_CANARY) line = __LINE__; /* nothing at or past the capacity */
            }
            if (st.unused) line = __LINE__;
            free(dst);
            all->v.images += st.v.images; all->v.carried += st.v.carried; all->v.bytes_read += st.v.bytes_read; all->tails += st.tails;
            if (st.max_chunks > all->max_chunks) all->max_chunks = st.max_chunks;
            result = line ? -line : result + 1;
        }
    }
    free(counts); free(lens); rpd_arc_free(&a);
    return result;
}

/* Archives of stored blocks (rp_stored_archive) with a dictionary header: both block sizes, checksum, seekable, dictionaries of
 * 1, 100, 4099 and 65535 bytes, and with chunk != 0 that many jobs per launch. -> the number of sessions, or minus a line. */
static int64_t rpvd_selftest(uint32_t chunk, rpvd_stats_t* all) {
    const uint32_t bss[2] = {4096u, 65536u}, dsz[4] = {1u, 100u, 4099u, 65535u};
    int64_t sessions = 0;
    uint32_t r = 4242u;
    for (int b = 0; b < 2; b++)
        for (int flags = 0; flags < 4; flags += b ? 3 : 1) { /* (64 KiB blocks: neither, and both) */
            const uint32_t bs = bss[b], D = dsz[(2 * b + flags) & 3];
            const int checksum = flags & 1, seekable = flags >> 1;
            const uint64_t totals[5] = {1, bs - 1u, bs + 33u, 7ull * bs + 5u, bs == 4096u ? 40ull * bs - 3u : 5ull * bs - 1u};
            uint8_t* dict = malloc(D);
            for (uint32_t i = 0; i < D; i++) dict[i] = (uint8_t)(i * 7u + 3u);
            for (int t = 0; t < 5; t++) {
                const uint64_t total = totals[t];
                const uint32_t id = 0xD1C70000u + (uint32_t)t + 16u * (uint32_t)flags;
                uint8_t* data = malloc(total);
                for (uint64_t i = 0; i < total; i++) { r = r * 1664525u + 1013904223u; data[i] = (uint8_t)(r >> 13); }
                rp_archive_t a;
                const int built = rp_stored_archive(data, total, bs, checksum, seekable, 1, id, &a);
                const int64_t rc = built ? rpvd_check_archive(a.comp, a.size, data, total, dict, D, 7u + (uint32_t)t, chunk, all) : -__LINE__;
                rp_archive_free(&a); free(data);
                if (rc < 0) { free(dict); return rc; }
                sessions += rc;
            }
            free(dict);
        }
    return sessions;
}

/* ---- a table that breaks a rule, in front of, inside or behind good calls. The session: an appendv_dict of `before` bytes in
 * entries of 1000 (before > 0), the bad table iov[0 .. n_iov) with bases nothing lies at and the promise `promised`, an
 * appendv_dict of `after` bytes (after > 0, with before + promised a multiple of bs) and, where the total is one too, end. small_cap: the capacity is 64 bytes, so a `before` of a block or more leaves the
 * session in ZXC_ERROR_DST_TOO_SMALL in front of the bad table. -> the session's status behind the bad call, which must also be
 * its status behind the last call (RP_BAD_PLAN when a job of the bad call was not the unused job, a byte was read by the encoder
 * during it, anything was written to the destination behind it, or a promise broke); *table_status: the table's verdict. */
static int64_t rpvd_session_bad_table(uint32_t bs, uint32_t dict_size, uint64_t before, const zxc_dev_iov_t* iov, uint32_t n_iov,
                                      uint64_t promised, uint64_t after, int checksum, int seekable, uint64_t max_piece, uint32_t chunk,
                                      int small_cap, int* table_status) {
    const uint64_t total = before + promised + after;
    uint8_t *src = malloc(total), *dict = malloc(dict_size);
    uint32_t r = 77u + bs + dict_size;
    for (uint64_t i = 0; i < total; i++) { r = r * 1664525u + 1013904223u; src[i] = (uint8_t)(r >> 11); }
    for (uint32_t i = 0; i < dict_size; i++) dict[i] = (uint8_t)(i * 5u + 1u);
    rp_archive_t a;
    int64_t status = RP_BAD_PLAN;
    if (!rp_stored_archive(src, total, bs, checksum, seekable, 1, 0xD1C7BADu, &a)) { free(src); free(dict); return status; }
    const uint64_t cap = small_cap ? 64u : a.size;
    uint8_t *dst = malloc(cap + 64u), *snap = malloc(cap + 64u);
    memset(dst, RPD_CANARY, cap + 64u);
    rpd_session_t d;
    rpvd_stats_t st;
    memset(&d, 0, sizeof d);
    memset(&st, 0, sizeof st);
    d.r.src = src; d.r.blocks = a.blocks; d.r.blk_at = a.blk_at; d.r.blk_size = a.blk_size; d.r.n_blocks = a.nb;
    if (rpd_begin(&d, total, max_piece, bs, checksum, seekable, dst, cap, dict, dict_size, 0xD1C7BADu, chunk) == 0) {
        uint64_t* lens = malloc((total / 1000u + 2u) * 8u);
        uint32_t n = 0;
        for (uint64_t left = before; left; n++) { lens[n] = left < 1000u ? left : 1000u; left -= lens[n]; }
        if (n) rpvd_appendv(&d, lens, n, &st);
        const int64_t held = d.r.ctl.status;
        const uint64_t read_before = st.v.bytes_read, jobs_before = st.v.images, blocks_bad = (before % bs + promised) / bs;
        memcpy(snap, dst, cap + 64u);
        *table_status = rpvd_appendv_table(&d, iov, n_iov, promised, &st);
        status = d.r.ctl.status;
        int ok = !d.r.bad && st.v.bytes_read == read_before && st.v.images == jobs_before && st.unused == blocks_bad &&
                 d.r.total == before + promised && memcmp(snap, dst, cap + 64u) == 0;
        if (status != (held < 0 ? held : *table_status)) ok = 0;
        /* good calls behind it: they run (the device cannot tell the host), nothing reaches the destination, the status stays. The
         * bad call's tail was never gathered, so what waits in the carry area behind it is not the source's: the stand-in encoder,
         * which checks its input against the source, can follow only from a block boundary on. */
        if ((before + promised) % bs == 0) {
            n = 0;
            for (uint64_t left = after; left; n++) { lens[n] = left < 1000u ? left : 1000u; left -= lens[n]; }
            if (n) rpvd_appendv(&d, lens, n, &st);
            if (d.r.bad || d.r.ctl.status != status || memcmp(snap, dst, cap + 64u) != 0 || d.r.total != total) ok = 0;
            if (total % bs == 0 && (rpd_end(&d) != status || memcmp(snap, dst, cap + 64u) != 0)) ok = 0;
        } else if (after) ok = 0; /* (the caller's case is not one the replay can follow) */
        if (!ok) status = RP_BAD_PLAN;
        free(lens);
        rpd_free(&d);
    }
    free(snap); free(dst); rp_archive_free(&a); free(src); free(dict);
    return status;
}
#endif
