/* Test-only: the dictionary session of zxc_amd/csrc/zxc_append.h (zxc_mi355x_compress_begin_dict_device) replayed on the host the
 * way the entry points and kernels of zxc_append_device.hip run it, on top of append_replay.h: the images-mode plan of every piece,
 * per chunk the [dict | block] images built from the one or two places zap_job_images names and the job table that points at them,
 * the tail copy, then the sibling's advance, scatter and gather, and the finish with the dictionary flag and id. Every buffer is a
 * heap block of exactly the size the session is promised (every piece's source a copy of exactly its bytes, the image area exactly
 * min(J, C) images + ZC_IMAGE_PAD), so that a sanitizer sees any read or write outside them. The encoder is a stand-in: block k of
 * the archive is whatever the caller says block k is. Every job's image is checked: the dictionary in front, the bytes of its
 * block behind it, and the encoder's over-read inside the image area.
 * Shared by append_dict_shim.c (loaded by tests/test_compress_append_dict_device_cpu.py) and append_dict_san_main.c. */
#ifndef APPEND_DICT_REPLAY_H
#define APPEND_DICT_REPLAY_H
#include "append_replay.h"

#define RPD_CANARY 0xC3u

typedef struct rpd_session {
    rp_session_t r;
    zap_shape_images_t shi;
    uint8_t* images;
    const uint8_t* dict;
    uint32_t dict_size, dict_id, chunk; /* chunk: jobs per encode launch (the shape's, or a smaller one to cross chunks cheaply) */
} rpd_session_t;

static int rpd_begin(rpd_session_t* s, uint64_t max_total, uint64_t max_piece, uint32_t bs, int checksum, int seekable, uint8_t* dst,
                     uint64_t cap, const uint8_t* dict, uint32_t dict_size, uint32_t dict_id, uint32_t chunk) {
    const int rc = zap_shape_images(max_total, max_piece, bs, 2u * bs + 512u, seekable, dict_size, &s->shi);
    if (rc != 0) return rc;
    if (rp_begin(&s->r, max_total, max_piece, bs, checksum, seekable, dst, cap) != 0) return RP_BAD_PLAN;
    if (s->shi.bytes - 256u < s->shi.o_images + (uint64_t)s->shi.chunk_jobs * s->shi.image + ZC_IMAGE_PAD) s->r.bad = 1;
    s->chunk = chunk && chunk < s->shi.chunk_jobs ? chunk : s->shi.chunk_jobs;
    s->images = malloc((size_t)s->chunk * s->shi.image + ZC_IMAGE_PAD);
    s->dict = dict; s->dict_size = dict_size; s->dict_id = dict_id;
    return 0;
}
static void rpd_free(rpd_session_t* s) {
    free(s->images);
    rp_free(&s->r);
}

/* one piece of the images-mode plan, the images front end: src = exactly the piece's p->n bytes (NULL for the plan of `end`) */
static void rpd_piece(rpd_session_t* d, const uint8_t* src, const zap_piece_t* p) {
    rp_session_t* s = &d->r;
    if (!p->nb) { rp_piece(s, src, p); return; } /* joins the carry: the prep kernel as it is */
    if (p->nb > s->sh.J || p->n_staged || p->cp[0].area != ZAP_SRC || p->cp[1].area != ZAP_SRC) { s->bad = 1; return; }
    const uint64_t first_block = s->total / s->bs, image = d->shi.image;
    for (uint32_t j0 = 0; j0 < p->nb; j0 += d->chunk) {
        const uint32_t n = p->nb - j0 < d->chunk ? p->nb - j0 : d->chunk;
        for (uint32_t w = 0; w < n; w++) { /* zxc_append_images_kernel, workgroup w */
            const zap_src2_t js = zap_job_images(p, j0 + w);
            uint8_t* at = d->images + w * image;
            memcpy(at, d->dict, d->dict_size);
            at += d->dict_size;
            for (int k = 0; k < 2; k++) {
                const zap_src_t g = js.seg[k];
                if (g.area != ZAP_SRC && g.area != ZAP_CARRY) s->bad = 1;
                if (g.len) memcpy(at, (g.area == ZAP_CARRY ? rp_area(s, ZAP_CARRY) : src) + g.off, g.len);
                at += g.len;
            }
            const zxc_enc_job_t job = {w * image, js.seg[0].len + js.seg[1].len, 0u};
            s->jobs[j0 + w] = job;
        }
        if (j0 == 0 && p->cp[2].area == ZAP_NEXT) { /* ... and the workgroup behind them: the tail */
            uint8_t* t = rp_area(s, ZAP_NEXT) + p->cp[2].at;
            memcpy(t, src + p->cp[2].from, p->cp[2].len);
            memset(t + p->cp[2].len, 0, ZAP_PAD);
        } else if (p->cp[2].area != ZAP_SRC && p->cp[2].area != ZAP_NEXT) s->bad = 1;
        for (uint32_t w = 0; w < n; w++) { /* the encode launch over jobs + j0, slots + j0 x stride, sizes + j0 */
            const zxc_enc_job_t job = s->jobs[j0 + w];
            const uint8_t* in = d->images + job.src_off;
            const uint64_t k = first_block + j0 + w;
            if (job.src_off + d->dict_size + job.len + ZAP_OVERREAD > (uint64_t)n * image + ZC_IMAGE_PAD) s->bad = 1; /* the over-read */
            if (job.len == 0 || job.len > s->bs || (j0 + w + 1u < p->nb && job.len != s->bs)) s->bad = 1;
            if (memcmp(in, d->dict, d->dict_size) != 0 || !rp_encode_job(s, j0 + w, k, in + d->dict_size, job.len)) {
                s->bad = 1;
                s->sizes[j0 + w] = 0;
            }
        }
    }
    rp_back(s, p->nb);
}

/* the loop of zxc_mi355x_compress_append_device in a dictionary session: the next n bytes of the source */
static void rpd_append(rpd_session_t* d, uint64_t n) {
    rp_session_t* s = &d->r;
    uint64_t left = n, at = s->total, m;
    while (left && rp_next_piece(s, left, &m)) {
        uint8_t* piece = malloc(m); /* exactly the piece's bytes */
        memcpy(piece, s->src + at, m);
        zap_piece_t p;
        zap_plan_piece_images((uint32_t)(s->total % s->bs), m, s->bs, &p);
        rpd_piece(d, piece, &p);
        free(piece);
        s->total += m;
        if (p.swap) s->cur ^= 1u;
        at += m; left -= m;
    }
}
static int64_t rpd_end(rpd_session_t* d) {
    rp_session_t* s = &d->r;
    zap_piece_t p;
    zap_plan_end((uint32_t)(s->total % s->bs), s->bs, &p);
    if (p.nb) rpd_piece(d, NULL, &p);
    zap_finish_dict(&s->ctl, s->dst, s->cap, s->total, s->bs, s->checksum, s->seekable, 1, d->dict_id);
    const uint64_t nb = s->total / s->bs + (s->total % s->bs != 0);
    if (s->seekable) for (uint64_t b = 0; b < nb; b++) zap_put_seek_entry(&s->ctl, s->dst, s->seek, b);
    return s->bad ? RP_BAD_PLAN : s->ctl.status;
}

/* A whole dictionary session: begin, the appends of lens[0 .. n_lens) (their sum is total), end. dst: cap bytes. */
static int64_t rpd_session(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                           uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, uint32_t n_lens,
                           uint64_t max_piece, uint8_t* dst, uint64_t cap, const uint8_t* dict, uint32_t dict_size, uint32_t dict_id,
                           uint32_t chunk) {
    rpd_session_t d;
    memset(&d, 0, sizeof d);
    d.r.src = src; d.r.blocks = blocks; d.r.blk_at = blk_at; d.r.blk_size = blk_size; d.r.n_blocks = n_blocks;
    const int rc = rpd_begin(&d, total, max_piece, bs, checksum, seekable, dst, cap, dict, dict_size, dict_id, chunk);
    if (rc != 0) return rc;
    for (uint32_t i = 0; i < n_lens; i++) rpd_append(&d, lens[i]);
    const int64_t r = d.r.total == total ? rpd_end(&d) : RP_BAD_PLAN;
    rpd_free(&d);
    return r;
}

/* The promises of one images-mode plan, for a piece of n > 0 bytes behind `carry`: -> 0, or the number of the promise it breaks. */
static int rpd_plan_check(uint32_t carry, uint64_t n, uint32_t bs) {
    zap_piece_t p, q;
    zap_plan_piece_images(carry, n, bs, &p);
    zap_plan_piece(carry, n, bs, &q);
    if (p.nb != q.nb || p.tail != q.tail || p.nb != (carry + n) / bs || p.tail != (carry + n) % bs || p.swap != q.swap || p.first != q.first) return 1;
    if (p.n_staged != 0 || p.cp[1].area != ZAP_SRC) return 2;
    uint8_t* seen = calloc(n, 1); /* how often each source byte is read */
    int rc = 0;
    if (p.nb == 0) { /* the bytes join the carry */
        if (!(p.cp[0].area == ZAP_CARRY && p.cp[0].at == carry && p.cp[0].len == n && p.cp[0].from == 0 && !p.swap && p.cp[2].area == ZAP_SRC)) rc = 3;
        else memset(seen, 1, n);
    } else {
        if (p.cp[0].area != ZAP_SRC) rc = 4; /* the head is delivered to job 0, not copied */
        if (!(p.swap && p.cp[2].area == ZAP_NEXT && p.cp[2].at == 0 && p.cp[2].len == p.tail && p.cp[2].from + p.tail == n)) rc = 5;
        else for (uint32_t i = 0; i < p.tail; i++) seen[p.cp[2].from + i]++;
        if (p.n_direct != p.nb - (carry ? 1u : 0u)) rc = 6; /* every whole block direct, whatever lies behind it */
        for (uint32_t j = 0; j < p.nb && !rc; j++) {
            const zap_src2_t s = zap_job_images(&p, j);
            if (s.seg[0].len + s.seg[1].len != bs) rc = 7;
            if (carry && j == 0) {
                if (!(s.seg[0].area == ZAP_CARRY && s.seg[0].off == 0 && s.seg[0].len == carry && s.seg[1].area == ZAP_SRC && s.seg[1].off == 0)) rc = 8;
            } else if (!(s.seg[0].area == ZAP_SRC && s.seg[1].len == 0)) rc = 9;
            for (int k = 0; k < 2 && !rc; k++) {
                if (s.seg[k].area != ZAP_SRC) continue;
                if (s.seg[k].off + s.seg[k].len > n) { rc = 10; break; }
                for (uint32_t i = 0; i < s.seg[k].len; i++) seen[s.seg[k].off + i]++;
            }
        }
    }
    for (uint64_t i = 0; i < n && !rc; i++) if (seen[i] != 1) rc = 11; /* once each: by one job segment or by the tail copy */
    free(seen);
    if (rc) return rc;
    /* `end` behind this piece: the carry area alone */
    if (p.tail) {
        zap_plan_end(p.tail, bs, &q);
        const zap_src2_t s = zap_job_images(&q, 0);
        if (!(q.nb == 1 && s.seg[0].area == ZAP_CARRY && s.seg[0].off == 0 && s.seg[0].len == p.tail && s.seg[1].len == 0)) return 12;
    }
    return 0;
}

/* ---- a complete archive with a dictionary header, cut into its blocks and put together again */
static uint32_t rpd_rnd_state;
static uint32_t rpd_rnd(void) { rpd_rnd_state = rpd_rnd_state * 1664525u + 1013904223u; return rpd_rnd_state >> 8; }

/* the blocks of a complete, regular archive whose header carries a dictionary id (one block per block_size bytes of `total`), cut
 * out one behind the other, with what the header says and whether a seek table follows. -> 0, or minus the line that failed */
typedef struct rpd_arc {
    uint8_t* blocks;
    uint64_t* blk_at;
    uint32_t *blk_size, nb, bs, ck, id;
    int seekable;
} rpd_arc_t;
static int rpd_cut(const uint8_t* comp, uint64_t comp_size, uint64_t total, rpd_arc_t* a) {
    uint32_t lg = 0;
    memset(a, 0, sizeof *a);
    if (comp_size < ZC_FILE_HDR + ZC_BLK_HDR + ZC_FOOTER || zc_file_header(comp, &lg, &a->ck, &a->id) != ZXC_OK || !(comp[6] & 0x40u)) return -__LINE__;
    a->bs = 1u << lg;
    const uint64_t nb64 = total / a->bs + (total % a->bs != 0);
    a->blocks = malloc(comp_size);
    a->blk_at = malloc((nb64 + 1u) * 8u);
    a->blk_size = malloc((nb64 + 1u) * 4u);
    uint64_t at = ZC_FILE_HDR, used = 0;
    int line = 0;
    for (;;) {
        if (at + ZC_BLK_HDR > comp_size) { line = -__LINE__; break; }
        const uint64_t w = zc_rd64(comp + at);
        if (!zc_blk_hdr_ok(w)) { line = -__LINE__; break; }
        if (zc_blk_type(w) == ZC_BLK_EOF) break;
        const uint32_t sz = ZC_BLK_HDR + zc_blk_csz(w) + 4u * a->ck;
        if (a->nb >= nb64 || at + sz > comp_size) { line = -__LINE__; break; }
        a->blk_at[a->nb] = used; a->blk_size[a->nb] = sz;
        memcpy(a->blocks + used, comp + at, sz);
        used += sz; at += sz; a->nb++;
    }
    if (!line && (a->nb != nb64 || zc_rd64(comp + comp_size - ZC_FOOTER) != total)) line = -__LINE__; /* one block per block_size bytes */
    a->seekable = !line && comp_size - at > ZC_BLK_HDR + ZC_FOOTER;
    return line;
}
static void rpd_arc_free(rpd_arc_t* a) { free(a->blocks); free(a->blk_at); free(a->blk_size); }

/* one session over these cuts with room behind the archive: the archive byte for byte, the pattern intact everywhere outside it;
 * with `exact` also with a capacity of exactly the archive, and of one byte less: -> 0, or the line that failed */
static int rpd_check_cuts(const uint8_t* comp, uint64_t comp_size, const uint8_t* data, uint64_t total, const uint8_t* blocks,
                          const uint64_t* blk_at, const uint32_t* blk_size, uint32_t nb, uint32_t bs, int checksum, int seekable,
                          const uint64_t* lens, uint32_t n_lens, uint64_t max_piece, const uint8_t* dict, uint32_t dict_size,
                          uint32_t dict_id, uint32_t chunk, int exact) {
    uint8_t* dst = malloc(comp_size + 97u);
    memset(dst, RPD_CANARY, comp_size + 97u);
    int64_t rc = rpd_session(data, total, blocks, blk_at, blk_size, nb, bs, checksum, seekable, lens, n_lens, max_piece, dst,
                             comp_size + 33u, dict, dict_size, dict_id, chunk);
    int line = (rc == (int64_t)comp_size && memcmp(dst, comp, comp_size) == 0) ? 0 : __LINE__;
    for (uint64_t i = comp_size; i < comp_size + 97u && !line; i++) if (dst[i] != RPD_CANARY) line = __LINE__;
    free(dst);
    for (int short_by = 0; short_by < 2 && exact && !line; short_by++) {
        const uint64_t cap = comp_size - (uint64_t)short_by;
        dst = malloc(cap + 64u);
        memset(dst, RPD_CANARY, cap + 64u);
        rc = rpd_session(data, total, blocks, blk_at, blk_size, nb, bs, checksum, seekable, lens, n_lens, max_piece, dst, cap, dict,
                         dict_size, dict_id, chunk);
        if (short_by == 0 && !(rc == (int64_t)comp_size && memcmp(dst, comp, comp_size) == 0)) line = __LINE__;
        if (short_by == 1 && rc != ZXC_ERROR_DST_TOO_SMALL) line = __LINE__;
        for (uint64_t i = cap; i < cap + 64u && !line; i++) if (dst[i] != RPD_CANARY) line = __LINE__; /* nothing at or past the capacity */
        free(dst);
    }
    return line;
}

/* comp: a complete, regular archive whose header carries a dictionary id; data: its total decoded bytes. Sessions with a cut at
 * every byte boundary of the first block (dense == 0: every one within 70 bytes of its ends, every 97th between, of a large block some 40), and random cuts
 * (zero-length appends among them) with pieces shorter than the appends. -> the number of cut sets, or minus the line that failed. */
static int64_t rpd_check_archive(const uint8_t* comp, uint64_t comp_size, const uint8_t* data, uint64_t total, const uint8_t* dict,
                                 uint32_t dict_size, uint32_t seed, int dense) {
    rpd_arc_t a;
    int64_t result = rpd_cut(comp, comp_size, total, &a);
    const uint32_t bs = a.bs;
    uint64_t* lens = malloc((total / 7u + 64u) * 8u);
    rpd_rnd_state = seed;
    const uint64_t first = total < bs ? total : bs;
    for (uint64_t c = 0; c <= first && result >= 0; c += (dense || c < 70u || c + 70u >= first) ? 1u : first > 8192u ? first / 41u : 97u) {
        lens[0] = c; lens[1] = total - c;
        const int line = rpd_check_cuts(comp, comp_size, data, total, a.blocks, a.blk_at, a.blk_size, a.nb, bs, (int)a.ck, a.seekable, lens,
                                        2u, total > bs ? total : bs, dict, dict_size, a.id, 0u, c % 256u == 0);
        result = line ? -line : result + 1;
    }
    for (int k = 0; k < 12 && result >= 0; k++) {
        uint32_t n_lens = 0;
        uint64_t left = total;
        while (left || n_lens == 0) {
            const uint32_t kind = rpd_rnd() % 5u;
            uint64_t n = kind == 0 ? 0u : kind == 1 ? 1u : kind == 2 ? rpd_rnd() % bs : kind == 3 ? bs : rpd_rnd() % (3u * bs + 9u);
            if (n > left) n = left;
            lens[n_lens++] = n;
            left -= n;
            if (n_lens >= total / 7u + 60u) { lens[n_lens++] = left; left = 0; }
        }
        lens[n_lens++] = 0;
        const uint64_t mp[3] = {bs, 2ull * bs, 3ull * bs + 100u};
        const int line = rpd_check_cuts(comp, comp_size, data, total, a.blocks, a.blk_at, a.blk_size, a.nb, bs, (int)a.ck, a.seekable, lens,
                                        n_lens, mp[k % 3], dict, dict_size, a.id, k % 2 ? 2u : 0u, 1);
        result = line ? -line : result + 1;
    }
    free(lens); rpd_arc_free(&a);
    return result;
}

/* Archives of stored blocks (rp_stored_archive, the stand-in encoder of append_san_main.c) with a dictionary header, of several
 * blocks: both block sizes, checksum, seekable, dictionaries of 1 and 4099 bytes. -> the number of cut sets, or minus a line. */
static int64_t rpd_selftest(void) {
    const uint32_t bss[2] = {4096u, 65536u}, dsz[2] = {1u, 4099u};
    int64_t sets = 0;
    uint32_t r = 99u;
    for (int b = 0; b < 2; b++)
        for (int flags = 0; flags < 4; flags += b ? 3 : 1) { /* (64 KiB blocks: neither, and both) */
            const uint32_t bs = bss[b], D = dsz[(b + flags) & 1];
            const int checksum = flags & 1, seekable = flags >> 1;
            const uint64_t totals[5] = {0, 1, bs, 3ull * bs + 5u, bs == 4096u ? 70ull * bs - 3u : 2ull * bs + 1u};
            uint8_t* dict = malloc(D);
            for (uint32_t i = 0; i < D; i++) dict[i] = (uint8_t)(i * 7u + 3u);
            for (int t = 0; t < 5; t++) {
                const uint64_t total = totals[t];
                const uint32_t id = 0xD1C70000u + (uint32_t)t + 16u * (uint32_t)flags;
                uint8_t* data = malloc(total ? total : 1u);
                for (uint64_t i = 0; i < total; i++) { r = r * 1664525u + 1013904223u; data[i] = (uint8_t)(r >> 13); }
                rp_archive_t a;
                const int built = rp_stored_archive(data, total, bs, checksum, seekable, 1, id, &a);
                int64_t rc = built ? rpd_check_archive(a.comp, a.size, data, total, dict, D, 7u + (uint32_t)t, 0) : -__LINE__;
                rp_archive_free(&a); free(data);
                if (rc < 0) { free(dict); return rc; }
                sets += rc;
            }
            free(dict);
        }
    return sets;
}
#endif
