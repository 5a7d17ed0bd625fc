/* Stand-alone program (its own main, not loaded into anything) that replays zxc_mi355x_shufflev_device and the chunks of
 * zxc_mi355x_compress_shufflev_device the way their grids run (shufflev_replay.h, from the rules of zxc_amd/csrc/zxc_shufflev.h),
 * where every entry is a heap buffer that ends with its last byte and the destination one that ends with `total` (SVR_CANARY 0:
 * only the alignment's k < 16 bytes lie in front), so that AddressSanitizer and UBSan see any read behind or in front of an entry,
 * a read of an empty entry's base, a 16-byte run taken whole where it crosses into the next entry, a search that leaves the table,
 * and any store outside [0, total). Element sizes 2, 4 and 8, unit 4096, the sizes of the shuffle tests, as one chunk and in
 * chunks of two units; the cuts: one entry, multiples of 16 E, entries of 16 E + 1 bytes (the boundary drifts through every byte
 * of a group), entries of 1 to 7 bytes, empty entries first, doubled in the middle and last, more than 1024 entries (a second
 * tile of the scan), a mix of the append tests' lengths, a cut on a unit boundary and one on a chunk boundary; the first entry's
 * alignment walks through 0 .. 15 from run to run. Then the tables the scan refuses, with the entries freed before the call: a
 * read of one is a use after free.
 * Built by tests/test_compress_shufflev_device_cpu.py with -fsanitize=address,undefined. Prints "SHUFFLEV OK <runs>", exits 0. */
#define SVR_CANARY 0u
#include "../container/san_util.h"

#include "shufflev_replay.h"

#define MAX_ENTRIES 40000u
static uint64_t lens[MAX_ENTRIES];
static int n_checked = 0;

static uint32_t push(uint32_t n, uint64_t* left, uint64_t want) {
    CHECK(n < MAX_ENTRIES);
    lens[n] = want < *left ? want : *left;
    *left -= lens[n];
    return n + 1u;
}

/* cut `kind` of T bytes -> the number of entries in lens[] */
static uint32_t cut(uint32_t kind, uint64_t T, uint32_t E) {
    static const uint64_t mix[] = {0, 1, 3, 31, 32, 33, 4095, 4096, 4097, 4096 + 31, 4096 + 32, 2 * 4096 + 33, 3 * 4096 + 5};
    uint64_t left = T;
    uint32_t n = 0;
    switch (kind) {
    case 0: return push(n, &left, T);
    case 1: while (left) n = push(n, &left, 16u * E * (1u + rnd() % 40u)); return n;
    case 2: while (left) n = push(n, &left, 16u * E + 1u); return n;
    case 3: while (left) n = push(n, &left, 1u + rnd() % 7u); return n;
    case 4:
        n = push(n, &left, 0); n = push(n, &left, T / 3u); n = push(n, &left, 0); n = push(n, &left, 0);
        n = push(n, &left, left); return push(n, &left, 0);
    case 5: for (uint32_t r = 0; r < 1100u; r++) n = push(n, &left, T / 1100u + (r < T % 1100u)); return n;
    case 6: while (left) n = push(n, &left, mix[rnd() % 13u]); return n;
    case 7: n = push(n, &left, 4096); return push(n, &left, left);
    default: n = push(n, &left, 8192); return push(n, &left, left);
    }
}

int main(void) {
    const uint32_t Es[] = {2u, 4u, 8u};
    rnd_state = 77u;
    uint8_t* x = malloc(9u * 4096u + 1000u);
    for (uint32_t i = 0; i < 9u * 4096u + 1000u; i++) x[i] = (uint8_t)((i * 2654435761u + 12345u) >> 13);
    for (int e = 0; e < 3; e++) {
        const uint32_t E = Es[e];
        const uint64_t sizes[] = {0, 1, E - 1u, E, E + 1u, 4095, 4096, 4097, 2u * 4096u + 3u * E + 1u, 9u * 4096u + 1000u};
        for (unsigned s = 0; s < sizeof sizes / sizeof sizes[0]; s++)
            for (uint32_t kind = 0; kind < 9u; kind++)
                for (uint64_t piece = 0; piece <= 8192u; piece += 8192u) {
                    const uint32_t n = cut(kind, sizes[s], E);
                    CHECK(svr_check(x, lens, n, sizes[s], E, 4096u, piece, (uint32_t)n_checked & 15u, ((uint32_t)n_checked * 7u + 3u) & 15u, NULL) == 0);
                    n_checked++;
                }
        /* no table at all, and a table of empty entries, over nothing */
        CHECK(svr_check(x, lens, 0u, 0u, E, 4096u, 0u, 0u, 0u, NULL) == 0);
        /* the tables the scan refuses: nothing of an entry (freed) or of the destination is touched */
        const uint64_t bad[] = {4096u + 7u, 3u * 4096u, 50u, 0u, 2u * 4096u + 1u};
        const uint64_t sum = 6u * 4096u + 58u;
        for (uint64_t piece = 0; piece <= 8192u; piece += 8192u) {
            CHECK(svr_check_bad(x, bad, 5u, sum + 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_SRC_TOO_SMALL);
            CHECK(svr_check_bad(x, bad, 5u, sum - 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_OVERFLOW);
            CHECK(svr_check_bad(x, bad, 5u, bad[1] - 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_OVERFLOW);
            CHECK(svr_check_bad(x, bad, 5u, sum, 2u, E, 4096u, piece, 1) == ZXC_ERROR_NULL_INPUT);
            n_checked += 4;
        }
    }
    /* the scratch: the exact form inside the stated bound, growing with the table */
    for (uint32_t n = 0; n < 5000u; n += 7u) CHECK(zsv_scratch_size(n) <= zsv_scratch_bound(n) && zsv_scratch_size(n) >= 8ull * (n + 1u) + 768u);
    CHECK(zsv_scratch_size(0xFFFFFFFFu) <= zsv_scratch_bound(0xFFFFFFFFu));
    CHECK(zsv_work_size(0u, 5u) == 0u && zsv_work_size(1000u, 5u) == 1024u + zsv_scratch_size(5u) + 256u);
    free(x);
    printf("SHUFFLEV OK %d\n", n_checked);
    return 0;
}
