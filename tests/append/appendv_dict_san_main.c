/* Stand-alone program (its own main, not loaded into anything) that replays dictionary sessions mixing
 * zxc_mi355x_compress_append_device and zxc_mi355x_compress_appendv_dict_device the way the entry points and kernels of
 * zxc_append_device.hip run them (appendv_dict_replay.h), over heap buffers of exactly the sizes a call is promised: every entry
 * of a table is a malloc of exactly its length, so an over-read of one byte behind an entry is a report, and the image area is
 * exactly its images and ZC_IMAGE_PAD. Archives of stored blocks with a dictionary header (rpvd_selftest: both block sizes,
 * dictionaries of 1, 100, 4099 and 65535 bytes, the cut sets of rpvd_calls), once with the shape's jobs per launch and once with
 * two, so that a chunk takes three launches and more; tables that break each rule in front of, inside and behind good calls; and
 * for every triple of arguments <archive> <decoded bytes> <dictionary content> that archive under the same cut sets.
 * Built by tests/test_compress_appendv_dict_device_cpu.py with -fsanitize=address,undefined.
 * Prints "APPENDV DICT OK <sessions>" and exits 0. */
#include "../container/san_util.h"

#include "appendv_dict_replay.h"

static uint8_t* slurp(const char* path, uint64_t* n) {
    FILE* f = fopen(path, "rb");
    CHECK(f != NULL);
    CHECK(fseek(f, 0, SEEK_END) == 0);
    const long size = ftell(f);
    CHECK(size >= 0 && fseek(f, 0, SEEK_SET) == 0);
    uint8_t* p = malloc(size ? (size_t)size : 1u); /* exactly the file's bytes */
    CHECK(fread(p, 1, (size_t)size, f) == (size_t)size);
    fclose(f);
    *n = (uint64_t)size;
    return p;
}

/* tables that break a rule: the verdict, its precedence, the sticky status, and that nothing is read, encoded or written */
static int bad_tables(void) {
    const uint32_t bs = 4096u;
    const uint64_t nowhere = 0x10u; /* a base nothing lies at */
    const struct { zxc_dev_iov_t iov[4]; uint32_t n; uint64_t promised; int want; } cases[] = {
        {{{nowhere, 3u * bs}, {nowhere, 5u}, {0u, 0u}, {nowhere, bs}}, 4, 4u * bs + 6u, ZXC_ERROR_SRC_TOO_SMALL},  /* one below */
        {{{nowhere, 3u * bs}, {nowhere, 5u}, {0u, 0u}, {nowhere, bs}}, 4, 4u * bs + 4u, ZXC_ERROR_OVERFLOW},       /* one above */
        {{{nowhere, 1u}, {nowhere, 3u * bs + 1u}, {0u, 0u}, {0u, 0u}}, 4, 3u * bs, ZXC_ERROR_OVERFLOW},            /* an entry longer than total */
        {{{nowhere, 1ull << 63}, {nowhere, 1ull << 63}, {nowhere, 5u}, {0u, 0u}}, 4, 2u * bs, ZXC_ERROR_OVERFLOW}, /* a sum past 2^64 */
        {{{nowhere, bs}, {0u, 1u}, {nowhere, bs}, {0u, 0u}}, 4, 2u * bs + 1u, ZXC_ERROR_NULL_INPUT},                 /* a zero base with a length */
        {{{nowhere, ~0ull}, {0u, 1u}, {nowhere, bs}, {0u, 0u}}, 4, 2u * bs, ZXC_ERROR_NULL_INPUT},                   /* ... in front of every other error */
        {{{nowhere, bs}, {0u, 7u}, {0u, 0u}, {0u, 0u}}, 2, 3u * bs, ZXC_ERROR_NULL_INPUT},
    };
    const uint32_t dicts[] = {1u, 4099u};
    int sessions = 0;
    for (unsigned i = 0; i < sizeof cases / sizeof cases[0]; i++)
        for (uint64_t max_piece = bs; max_piece <= 8ull * bs; max_piece *= 8u)
            for (int place = 0; place < 5; place++) {
                /* in front of good calls, inside them, behind them (with a carry of 100 and of none), and behind an error */
                const uint64_t promised = cases[i].promised, pad = (bs - promised % bs) % bs;
                const uint64_t before = place == 0 ? 0u : place == 3 ? 100u : place == 4 ? 2u * bs : bs + pad;
                const uint64_t after = place == 0 ? (pad ? 0u : 3u * bs) : place == 1 ? 2u * bs : 0u;
                int verdict = 0;
                const int64_t rc = rpvd_session_bad_table(bs, dicts[(i + (unsigned)place) & 1u], before, cases[i].iov, cases[i].n, promised, after, 1, 1,
                                                          max_piece, place == 1 ? 2u : 0u, place == 4, &verdict);
                CHECK(verdict == cases[i].want);
                CHECK(rc == (place == 4 ? ZXC_ERROR_DST_TOO_SMALL : cases[i].want));
                sessions++;
            }
    return sessions;
}

int main(int argc, char** argv) {
    rpvd_stats_t all;
    memset(&all, 0, sizeof all);
    int64_t sessions = rpvd_selftest(0u, &all);
    if (sessions < 0) { fprintf(stderr, "appendv_dict_replay.h:%lld failed\n", (long long)-sessions); return 1; }
    CHECK(all.v.images > 0 && all.v.carried > 0 && all.tails > 0 && all.max_chunks == 1);
    const int64_t small = rpvd_selftest(2u, &all); /* two jobs per launch */
    if (small < 0) { fprintf(stderr, "appendv_dict_replay.h:%lld failed (two jobs per launch)\n", (long long)-small); return 1; }
    CHECK(all.max_chunks >= 3);
    sessions += small;
    for (int a = 1; a + 2 < argc; a += 3) {
        uint64_t nc, nd, nx;
        uint8_t *comp = slurp(argv[a], &nc), *data = slurp(argv[a + 1], &nd), *dict = slurp(argv[a + 2], &nx);
        const int64_t rc = rpvd_check_archive(comp, nc, data, nd, dict, (uint32_t)nx, 11u + (uint32_t)a, 0u, &all);
        if (rc < 0) { fprintf(stderr, "%s: appendv_dict_replay.h:%lld failed\n", argv[a], (long long)-rc); return 1; }
        sessions += rc;
        free(dict); free(data); free(comp);
    }
    sessions += bad_tables();
    printf("APPENDV DICT OK %lld\n", (long long)sessions);
    return 0;
}
