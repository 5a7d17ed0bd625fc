/* Stand-alone program (its own main, not loaded into anything) that replays sessions mixing zxc_mi355x_compress_append_device and
 * zxc_mi355x_compress_appendv_device the way the entry points and kernels of zxc_append_device.hip run them (appendv_replay.h),
 * over heap buffers of exactly the sizes a call is promised: every entry of a table is a malloc of exactly its length, so an
 * over-read of one byte behind an entry is a report. The encoder is a stand-in (every block a stored block of the source's bytes,
 * with a trailer when checksums are on) that reads len + 32 bytes of every in-place job and len + 64 of every image; the archive
 * it must give is rp_stored_archive's. Tables: one entry, random entries with empty ones anywhere, runs of
 * 1-7-byte entries that span several blocks, entries that end 31 / 32 / 33 bytes behind a block boundary, calls that alternate
 * with plain appends and leave a carry each, chunk loops with max_piece of one and two blocks; tables that break each rule.
 * Built by tests/test_compress_appendv_device_cpu.py with -fsanitize=address,undefined. Prints "APPENDV OK <sessions>", exits 0. */
#include "../container/san_util.h"

#include "appendv_replay.h"

#define CANARY 0xC3u
#define PATTERNS 8

static int sessions = 0;
static uint64_t in_place = 0, images = 0;

/* the calls of one session over `total` bytes: lens[] and, per call, counts[] (0: a plain append of one length) */
static void calls(int pattern, uint64_t total, uint32_t bs, uint64_t* lens, uint32_t* n_lens, uint32_t* counts, uint32_t* n_calls,
                  uint64_t* max_piece) {
    uint64_t left = total;
    uint32_t nl = 0, nc = 0;
    *max_piece = total > bs ? total : bs;
#define ENTRY(n) do { uint64_t n_ = (n); if (n_ > left) n_ = left; lens[nl++] = n_; left -= n_; } while (0)
    if (pattern == 0) { ENTRY(total); counts[nc++] = 1; }                                  /* one entry */
    else if (pattern == 1 || pattern == 2) {                                               /* random entries, empty ones anywhere */
        lens[nl++] = 0;
        while (left) { const uint32_t k = rnd() % 5u; ENTRY(k == 0 ? 0u : k == 1 ? rnd() % 8u : k == 2 ? rnd() % bs : rnd() % (3u * bs + 9u)); }
        lens[nl++] = 0;
        counts[nc++] = nl;
        if (pattern == 2) *max_piece = bs;                                                  /* ... as a loop of one-block chunks */
    } else if (pattern == 3) {                                                              /* 1-7 bytes each, over 2.5 blocks, then the rest */
        uint64_t tiny = 0;
        while (left && tiny < 2u * bs + bs / 2u) { const uint64_t n = 1u + rnd() % 7u; tiny += n; ENTRY(n); }
        ENTRY(left);
        counts[nc++] = nl;
        *max_piece = 2ull * bs;
    } else if (pattern == 4) {                                                              /* ends 31 / 32 / 33 behind a boundary */
        ENTRY(bs + 31u); ENTRY(bs + 1u); ENTRY(bs + 1u); ENTRY(2u * bs - 33u + 32u); ENTRY(left);
        counts[nc++] = nl;
    } else if (pattern == 5 || pattern == 6) {                                              /* append, appendv, append, appendv: a carry each */
        for (int call = 0; left; call++) {
            if (call % 2 == 0) { ENTRY(1u + rnd() % (bs + bs / 2u)); counts[nc++] = 0; }
            else {
                const uint32_t first = nl;
                uint64_t want = bs / 3u + rnd() % (3u * bs);
                while (left && want) { uint64_t n = rnd() % 3u ? rnd() % 40u : rnd() % (2u * bs); if (n > want) n = want; want -= n; ENTRY(n); }
                counts[nc++] = nl - first;
            }
        }
        *max_piece = pattern == 5 ? 2ull * bs : bs;
    } else {                                                                                /* two tables back to back, the second all tiny */
        ENTRY(total / 2u + 17u); ENTRY(0u); counts[nc++] = 2;
        const uint32_t first = nl;
        while (left) ENTRY(1u + rnd() % 7u);
        if (nl > first) counts[nc++] = nl - first;
        *max_piece = 2ull * bs + 100u;
    }
#undef ENTRY
    CHECK(left == 0);
    *n_lens = nl; *n_calls = nc;
}

/* one source: its stored blocks and the archive they make (rp_stored_archive), and sessions over the patterns */
static void run(uint32_t bs, uint64_t total, int checksum, int seekable) {
    uint8_t* src = malloc(total ? total : 1);
    for (uint64_t i = 0; i < total; i++) src[i] = (uint8_t)(rnd() >> 5);
    rp_archive_t a;
    CHECK(rp_stored_archive(src, total, bs, checksum, seekable, 0, 0u, &a));
    const uint64_t size = a.size;

    uint64_t* lens = malloc((total + 4096u) * 8u);
    uint32_t* counts = malloc((total + 4096u) * 4u);
    for (int pattern = 0; pattern < PATTERNS; pattern++) {
        uint32_t n_lens = 0, n_calls = 0;
        uint64_t max_piece = 0;
        calls(pattern, total, bs, lens, &n_lens, counts, &n_calls, &max_piece);
        for (int short_by = 0; short_by < 2; short_by++) {
            const uint64_t cap = size - (uint64_t)short_by;
            uint8_t* dst = malloc(cap); /* exactly the capacity */
            memset(dst, CANARY, cap);
            rpv_stats_t st;
            const int64_t rc = rpv_session(src, total, a.blocks, a.blk_at, a.blk_size, a.nb, bs, checksum, seekable, lens, counts, n_calls, max_piece, dst,
                                           cap, &st);
            if (short_by == 0) CHECK(rc == (int64_t)size && memcmp(dst, a.comp, size) == 0);
            else CHECK(rc == ZXC_ERROR_DST_TOO_SMALL);
            in_place += st.in_place; images += st.images;
            free(dst);
            sessions++;
        }
    }
    free(counts); free(lens); rp_archive_free(&a); free(src);
}

/* tables that break a rule: the verdict, its precedence, the sticky status, and that nothing is read, encoded or written */
static void bad_tables(void) {
    const uint32_t bs = 4096u;
    const uint64_t nowhere = 0x10u; /* a base nothing lies at */
    uint8_t src[100];
    memset(src, 7, sizeof src);
    const struct { zxc_dev_iov_t iov[4]; uint32_t n; uint64_t promised; int want; } cases[] = {
        {{{nowhere, 3u * bs}, {nowhere, 5u}, {0u, 0u}, {nowhere, bs}}, 4, 4u * bs + 6u, ZXC_ERROR_SRC_TOO_SMALL},  /* one below */
        {{{nowhere, 3u * bs}, {nowhere, 5u}, {0u, 0u}, {nowhere, bs}}, 4, 4u * bs + 4u, ZXC_ERROR_OVERFLOW},       /* one above */
        {{{nowhere, 1u}, {nowhere, 3u * bs + 1u}, {0u, 0u}, {0u, 0u}}, 4, 3u * bs, ZXC_ERROR_OVERFLOW},            /* an entry longer than total */
        {{{nowhere, 1ull << 63}, {nowhere, 1ull << 63}, {nowhere, 5u}, {0u, 0u}}, 4, 1ull << 63, ZXC_ERROR_OVERFLOW}, /* a sum past 2^64 */
        {{{nowhere, bs}, {0u, 1u}, {nowhere, bs}, {0u, 0u}}, 4, 2u * bs + 1u, ZXC_ERROR_NULL_INPUT},                 /* a zero base with a length */
        {{{nowhere, ~0ull}, {0u, 1u}, {nowhere, bs}, {0u, 0u}}, 4, 2u * bs, ZXC_ERROR_NULL_INPUT},                   /* ... in front of every other error */
        {{{nowhere, bs}, {0u, 7u}, {0u, 0u}, {0u, 0u}}, 2, 3u * bs, ZXC_ERROR_NULL_INPUT},
    };
    for (unsigned i = 0; i < sizeof cases / sizeof cases[0]; i++)
        for (uint64_t max_piece = bs; max_piece <= 8ull * bs; max_piece *= 8u)
            for (uint32_t before = 0; before <= 100u; before += 100u) {
                const uint64_t promised = cases[i].promised; /* (the replay follows the promise chunk by chunk: only where it is small) */
                uint8_t* dst = malloc(64);
                memset(dst, CANARY, 64);
                int verdict = 0;
                if (promised <= 64ull * bs) {
                    const int64_t rc = rpv_session_bad_table(src, before, cases[i].iov, cases[i].n, promised, bs, 1, 1, max_piece, dst, 64, &verdict);
                    CHECK(verdict == cases[i].want && rc == cases[i].want);
                    for (int k = 0; k < 64; k++) CHECK(dst[k] == CANARY);
                    sessions++;
                } else {
                    uint64_t starts[5];
                    CHECK(zav_scan_serial(cases[i].iov, cases[i].n, promised, starts) == cases[i].want);
                }
                free(dst);
            }
    /* an error the session has stays; a valid table changes nothing */
    zap_ctl_t c;
    zap_begin(&c);
    zav_fold_status(&c, 0); CHECK(c.status == 0);
    zav_fold_status(&c, ZXC_ERROR_SRC_TOO_SMALL); CHECK(c.status == ZXC_ERROR_SRC_TOO_SMALL);
    zav_fold_status(&c, ZXC_ERROR_NULL_INPUT); CHECK(c.status == ZXC_ERROR_SRC_TOO_SMALL);
    zav_fold_status(&c, 0); CHECK(c.status == ZXC_ERROR_SRC_TOO_SMALL);
}

int main(void) {
    rnd_state = 8765u;
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++) {
                const uint32_t bs = bss[b];
                const uint64_t totals[] = {1, bs - 1u, bs + 33u, 7ull * bs + 5u, bs == 4096u ? 40ull * bs - 3u : 5ull * bs - 1u};
                for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(bs, totals[i], checksum, seekable);
            }
    bad_tables();
    CHECK(in_place > 0 && images > 0);
    printf("APPENDV OK %d\n", sessions);
    return 0;
}
