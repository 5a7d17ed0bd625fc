/* Stand-alone program (its own main, not loaded into anything) that replays the shuffle and un-shuffle kernels of
 * zxc_shuffle_device.hip the way their grid runs them (shuffle_replay.h, from the rules of zxc_amd/csrc/zxc_shuffle.h), where source
 * and destination are heap buffers that end with their last byte (SHR_CANARY 0: only the alignment's k < 16 pattern bytes lie in
 * front), so that AddressSanitizer and UBSan see any 16-byte access of a group or byte of the leftovers outside [0, n): a group
 * the plan hands out past the last whole one, a plane access that leaves the ragged unit, a shift or an index that overflows.
 * Element sizes 2, 4 and 8; units of 4 KiB and 64 KiB; every n in [0, 2 x 4096 + 40] for the small unit with the alignments walking
 * through 0 .. 15, all 256 pairs of alignments at the sizes where a path begins or ends, a size of several wavefronts, and the edges
 * of the large unit.
 * Built by tests/test_shuffle_device_cpu.py with -fsanitize=address,undefined. Prints "SHUFFLE OK <runs>", exits 0. */
#define SHR_CANARY 0u
#include "../container/san_util.h"

#include "shuffle_replay.h"

static int n_checked = 0;

static void one(uint64_t n, uint32_t E, uint32_t unit, uint32_t sa, uint32_t da) {
    CHECK(shr_check(n, E, unit, sa, da, (uint32_t)n + E) == 0);
    n_checked++;
}

int main(void) {
    const uint32_t Es[] = {2u, 4u, 8u};
    for (int e = 0; e < 3; e++) {
        const uint32_t E = Es[e];
        for (uint64_t n = 0; n <= 2u * 4096u + 40u; n++) one(n, E, 4096u, (uint32_t)(n & 15u), (uint32_t)((n >> 4) + 5u * n + 3u) & 15u);
        const uint64_t edges[] = {0, 1, E - 1u, E, E + 1u, 16u * E - 1u, 16u * E, 16u * E + 1u, 4095, 4096, 4097, 4096u + 16u * E + E - 1u,
                                  2u * 4096u + 3u * E + 1u};
        for (unsigned i = 0; i < sizeof edges / sizeof edges[0]; i++)
            for (uint32_t a = 0; a < 256u; a++) one(edges[i], E, 4096u, a >> 4, a & 15u);
        for (uint32_t a = 0; a < 16u; a++) one(9u * 4096u + 1000u, E, 4096u, a, (a * 7u + 3u) & 15u); /* several wavefronts */
        const uint64_t big[] = {65535, 65536, 65537, 65536u + 17u * E + 3u, 2u * 65536u + 8191u};
        for (unsigned i = 0; i < sizeof big / sizeof big[0]; i++)
            for (uint32_t a = 0; a < 16u; a += 3u) one(big[i], E, 65536u, a, (a * 7u + 3u) & 15u);
    }
    /* the chunk of the archive calls */
    CHECK(zsh_piece(0, 0, 4096u) == 4096u && zsh_piece(1, 0, 4096u) == 4096u && zsh_piece(9u * 4096u + 1000u, 8192u, 4096u) == 8192u);
    CHECK(zsh_piece(9u * 4096u + 1000u, 0, 4096u) == 10u * 4096u && zsh_piece(1ull << 40, 0, 1u << 19) == ZSH_DEFAULT_PIECE);
    CHECK(zsh_piece(1ull << 40, (1u << 20) + 5u, 1u << 19) == 1u << 20 && zsh_piece(~0ull, 0, 4096u) == ZSH_DEFAULT_PIECE);
    printf("SHUFFLE OK %d\n", n_checked);
    return 0;
}
