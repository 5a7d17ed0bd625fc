/* Stand-alone program (its own main, not loaded into anything) that replays zxc_mi355x_unshufflev_device and the chunks of
 * zxc_mi355x_decompress_shufflev_device the way their grids run (unshufflev_replay.h, from the rules of
 * zxc_amd/csrc/zxc_unshufflev.h), where every entry is a heap buffer that ends with its last byte (UVR_CANARY 0: only the
 * alignment's k < 16 bytes lie in front) and the source one that ends with `total`, so that AddressSanitizer and UBSan see any
 * store behind or in front of an entry, a look at an empty entry's base, a 16-byte run stored whole where it crosses into the next
 * entry, a search that leaves the table, and any load outside the source. Element sizes 2, 4 and 8, unit 4096, the sizes of the
 * shuffle tests, as one chunk and in chunks of two units; the cuts: one entry, multiples of 16 E, entries of 16 E + 1 bytes (the
 * boundary drifts through every byte of a group), entries of 1 to 7 bytes, empty entries first, doubled in the middle and last,
 * more than 1024 entries (a second tile of the scan), a mix of the append tests' lengths, a cut on a unit boundary and one on a
 * chunk boundary; the first entry's alignment walks through 0 .. 15 from run to run. Then the tables the scan refuses, with the
 * entries freed before the call: a store into one is a use after free.
 * Built by tests/test_decompress_shufflev_device_cpu.py with -fsanitize=address,undefined. Prints "UNSHUFFLEV OK <runs>", exits 0. */
#define UVR_CANARY 0u
#include "../container/san_util.h"

#include "unshufflev_replay.h"

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
    const uint32_t biggest = 9u * 4096u + 1000u;
    rnd_state = 78u;
    uint8_t* bytes = malloc(biggest);
    for (uint32_t i = 0; i < biggest; i++) bytes[i] = (uint8_t)((i * 2654435761u + 12345u) >> 13);
    for (int e = 0; e < 3; e++) {
        const uint32_t E = Es[e];
        const uint64_t sizes[] = {0, 1, E - 1u, E, E + 1u, 4095, 4096, 4097, 2u * 4096u + 3u * E + 1u, biggest};
        for (unsigned s = 0; s < sizeof sizes / sizeof sizes[0]; s++) {
            uint8_t* y = malloc(sizes[s] ? sizes[s] : 1u); /* the source ends with its last byte */
            memcpy(y, bytes, sizes[s]);
            for (uint32_t kind = 0; kind < 9u; kind++)
                for (uint64_t piece = 0; piece <= 8192u; piece += 8192u) {
                    const uint32_t n = cut(kind, sizes[s], E);
                    CHECK(uvr_check(y, lens, n, sizes[s], E, 4096u, piece, (uint32_t)n_checked & 15u, NULL) == 0);
                    n_checked++;
                }
            free(y);
        }
        /* no table at all over nothing */
        CHECK(uvr_check(bytes, lens, 0u, 0u, E, 4096u, 0u, 0u, NULL) == 0);
        /* the tables the scan refuses: nothing of an entry (freed) is touched; the status is the read direction's */
        const uint64_t bad[] = {4096u + 7u, 3u * 4096u, 50u, 0u, 2u * 4096u + 1u};
        const uint64_t sum = 6u * 4096u + 58u;
        for (uint64_t piece = 0; piece <= 8192u; piece += 8192u) {
            CHECK(uvr_check_bad(bytes, bad, 5u, sum + 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_DST_TOO_SMALL);
            CHECK(uvr_check_bad(bytes, bad, 5u, sum - 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_OVERFLOW);
            CHECK(uvr_check_bad(bytes, bad, 5u, bad[1] - 1u, ~0u, E, 4096u, piece, 1) == ZXC_ERROR_OVERFLOW);
            CHECK(uvr_check_bad(bytes, bad, 5u, sum, 2u, E, 4096u, piece, 1) == ZXC_ERROR_NULL_INPUT);
            n_checked += 4;
        }
    }
    /* the work area and the result word */
    CHECK(zuv_work_size(0u, 5u) == 0u && zuv_work_size(1000u, 5u) == 1024u + zsv_scratch_size(5u));
    CHECK(zuv_result(ZXC_ERROR_SRC_TOO_SMALL, 7, 7u) == ZXC_ERROR_DST_TOO_SMALL && zuv_result(0, 7, 8u) == ZXC_ERROR_CORRUPT_DATA);
    CHECK(zuv_result(0, 7, 7u) == 7 && zuv_result(0, 9, 0u) == 9 && zuv_result(0, ZXC_ERROR_BAD_HEADER, 8u) == ZXC_ERROR_BAD_HEADER);
    free(bytes);
    printf("UNSHUFFLEV OK %d\n", n_checked);
    return 0;
}
