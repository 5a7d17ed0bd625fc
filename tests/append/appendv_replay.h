/* Test-only: zxc_mi355x_compress_appendv_device replayed on the host on top of append_replay.h, the way the entry point and the
 * kernels of zxc_append_device.hip run it with the rules of zxc_amd/csrc/zxc_appendv.h: the scan of the table, the chunk loop, per
 * chunk the prep of every workgroup and thread (zav_prep, the very lines the kernel runs), the stand-in encoder, the predicated
 * advance, scatter and gather. Every entry of a table is a heap buffer of exactly its length, the table and the scratch are heap
 * buffers of exactly their sizes (the scratch with a canary behind scratch_size), so a sanitizer sees any read or write outside
 * them. The stand-in encoder reads len + 32 bytes of every job that is encoded where it lies and len + 64 of every image or carry
 * area, as the encoder may, and checks what it read against the source the caller names.
 * Shared by appendv_shim.c (loaded by tests/test_compress_appendv_device_cpu.py) and appendv_san_main.c (a program of its own). */
#ifndef APPENDV_REPLAY_H
#define APPENDV_REPLAY_H
#include "append_replay.h"
#include "../../zxc_amd/csrc/zxc_appendv.h"

#define RPV_THREADS 64u    /* threads of a replayed workgroup (>= ZAP_PAD) */
#define RPV_CANARY 0x5Au
#define RPV_CANARY_BYTES 64u
#define RPV_ODD 3u         /* the scratch starts this far into its allocation: any alignment */

/* what the stand-in encoder saw, for the tests */
typedef struct rpv_stats {
    uint64_t in_place, images, carried; /* jobs encoded where they lie, from an image, from the carry area */
    uint64_t bytes_read;                /* by the stand-in encoder, over-reads included */
} rpv_stats_t;

static volatile uint8_t rpv_sink;
/* the encoder may read these bytes: touch every one (a sanitizer sees an over-read) */
static void rpv_touch(const uint8_t* p, uint64_t n, rpv_stats_t* st) {
    uint8_t x = 0;
    for (uint64_t i = 0; i < n; i++) x ^= p[i];
    rpv_sink = x;
    st->bytes_read += n;
}

/* One chunk behind its plan, the appendv front end (ap_piece with a virtual source). status: the table's verdict. */
static void rpv_chunk(rp_session_t* s, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, const zav_chunk_t* c,
                      uint8_t* images, uint32_t image, rpv_stats_t* st) {
    const zap_piece_t* p = &c->p;
    if (p->nb > s->sh.J) { s->bad = 1; return; }
    uint8_t *carry = s->area[s->cur], *next = s->area[s->cur ^ 1u];
    for (uint32_t w = 0; w < zav_groups(c); w++) /* the prep kernel */
        for (uint32_t t = 0; t < RPV_THREADS; t++)
            zav_prep(iov, starts, n_iov, status, c, w, t, RPV_THREADS, carry, next, images, image, s->jobs);
    if (!p->nb) return;
    const uint64_t first_block = s->total / s->bs; /* blocks in front of this chunk */
    for (uint32_t j = 0; j < p->nb; j++) { /* the encode launch over the job table */
        const zxc_enc_job_t job = s->jobs[j];
        if (job.len == 0) continue; /* an unused job: its slot and size stay */
        if (status < 0 || job.len != s->bs) { s->bad = 1; continue; }
        const uint8_t* in = (const uint8_t*)(uintptr_t)job.src_off;
        const int is_image = in >= images && in < images + (uint64_t)s->sh.J * image, is_carry = in == carry;
        if (is_image || is_carry) {
            rpv_touch(in, (uint64_t)job.len + ZAP_PAD, st);
            for (uint32_t k = 0; k < ZAP_PAD; k++) if (in[job.len + k] != 0) s->bad = 1; /* the padding behind a gathered block */
            if (is_image && ((uintptr_t)in & 255u)) s->bad = 1;
            if (is_image) st->images++; else st->carried++;
        } else {
            rpv_touch(in, (uint64_t)job.len + ZAP_OVERREAD, st); /* inside one entry, or the sanitizer reports it */
            st->in_place++;
        }
        rp_encode_job(s, j, first_block + j, in, job.len);
    }
    if (status >= 0) rp_back(s, p->nb); /* the advance is not run after a table error; scatter and gather see the session's error */
}

/* zxc_mi355x_compress_appendv_device behind its synchronous checks: the table iov[0 .. n_iov) (host addresses) and the caller's
 * promise `total`. -> the table's verdict. */
static int rpv_appendv_table(rp_session_t* s, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, rpv_stats_t* st) {
    zav_shape_t vsh;
    if (zav_shape(n_iov, s->max_piece, s->bs, &vsh) != 0 || n_iov == 0) { s->bad = 1; return 0; }
    uint8_t* alloc = malloc(RPV_ODD + vsh.bytes + RPV_CANARY_BYTES); /* scratch_size bytes at an odd address, a canary behind them */
    memset(alloc, RPV_CANARY, RPV_ODD + vsh.bytes + RPV_CANARY_BYTES);
    uint8_t* sb = (uint8_t*)zc_round_up((uint64_t)(uintptr_t)(alloc + RPV_ODD), 256u);
    if (sb + vsh.bytes - 256u > alloc + RPV_ODD + vsh.bytes) s->bad = 1; /* the layout fits scratch_size from any alignment */
    zav_ctl_t* vctl = (zav_ctl_t*)sb;
    uint64_t* starts = (uint64_t*)(sb + vsh.o_starts);
    vctl->status = zav_scan_serial(iov, n_iov, total, starts); /* the three scan kernels */
    vctl->sum = starts[n_iov];
    zav_fold_status(&s->ctl, vctl->status);
    uint64_t left = total, v = 0, m;
    while (left && rp_next_piece(s, left, &m)) {
        zav_chunk_t c;
        zav_plan_chunk((uint32_t)(s->total % s->bs), m, s->bs, v, &c);
        rpv_chunk(s, iov, starts, n_iov, vctl->status, &c, sb + vsh.o_images, vsh.image, st);
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

/* An appendv of the next sum(lens) bytes of the session's source: entry r is a heap copy of exactly lens[r] bytes; an empty entry
 * has a base that must not be looked at (0, or an address nothing lies at). */
static void rpv_appendv(rp_session_t* s, const uint64_t* lens, uint32_t n_iov, rpv_stats_t* st) {
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
    if (rpv_appendv_table(s, iov, n_iov, total, st) != 0) s->bad = 1; /* a valid table */
    for (uint32_t r = 0; r < n_iov; r++) if (lens[r]) free((void*)(uintptr_t)iov[r].base);
    free(iov);
}

/* A whole session: begin, then call i appends lens[at_i .. at_i + counts[i]) bytes: counts[i] > 0: one appendv over that many
 * entries; counts[i] == 0: one plain append of lens[at_i] bytes (which takes one length). Then end. */
static int64_t rpv_session(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                           uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, const uint32_t* counts,
                           uint32_t n_calls, uint64_t max_piece, uint8_t* dst, uint64_t cap, rpv_stats_t* st) {
    rp_session_t s;
    memset(&s, 0, sizeof s);
    memset(st, 0, sizeof *st);
    s.src = src; s.blocks = blocks; s.blk_at = blk_at; s.blk_size = blk_size; s.n_blocks = n_blocks;
    const int rc = rp_begin(&s, total, max_piece, bs, checksum, seekable, dst, cap);
    if (rc != 0) return rc;
    for (uint32_t i = 0; i < n_calls; i++) {
        if (counts[i]) { rpv_appendv(&s, lens, counts[i], st); lens += counts[i]; }
        else { rp_append(&s, lens[0]); lens += 1; }
    }
    const int64_t r = s.total == total ? rp_end(&s) : RP_BAD_PLAN;
    rp_free(&s);
    return r;
}

/* A session of one plain append of `before` < block_size bytes (they wait in the carry area) and then an appendv over a table that
 * breaks a rule: iov as given, with bases nothing lies at, since no entry of such a table may be read; `promised` is the caller's
 * total, which the chunk loop follows as ever. -> the session's status behind the call (RP_BAD_PLAN when a job was encoded, a byte
 * was read or a promise broke); *table_status: the table's verdict. Nothing is written to dst. */
static int64_t rpv_session_bad_table(const uint8_t* src, uint64_t before, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t promised,
                                     uint32_t bs, int checksum, int seekable, uint64_t max_piece, uint8_t* dst, uint64_t cap,
                                     int* table_status) {
    rp_session_t s;
    rpv_stats_t st;
    memset(&s, 0, sizeof s);
    memset(&st, 0, sizeof st);
    s.src = src; s.n_blocks = 0; /* the stand-in encoder has no block to give: none may be asked for */
    const int rc = rp_begin(&s, before + promised, max_piece, bs, checksum, seekable, dst, cap);
    if (rc != 0) return rc;
    if (before < bs) rp_append(&s, before); else s.bad = 1;
    *table_status = rpv_appendv_table(&s, iov, n_iov, promised, &st);
    const int64_t status = (s.bad || st.bytes_read != 0 || s.total != before + promised) ? RP_BAD_PLAN : s.ctl.status;
    rp_free(&s);
    return status;
}
#endif
