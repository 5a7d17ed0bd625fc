/* Test-only: the rules of zxc_amd/csrc/zxc_shuffle.h behind C-ABI names, for tests/test_shuffle_device_cpu.py (loaded with ctypes,
 * built with the host C compiler and no sanitizer). */
#include "shuffle_replay.h"

uint64_t shs_index(uint64_t p, uint64_t n, uint32_t E, uint32_t unit) { return zsh_index(p, n, E, unit); }
void shs_by_index(const uint8_t* src, uint8_t* dst, uint64_t n, uint32_t E, uint32_t unit, int inverse) { shr_by_index(src, dst, n, E, unit, inverse); }
void shs_replay(const uint8_t* src, uint8_t* dst, uint8_t* hits, uint64_t n, uint32_t E, uint32_t unit, int inverse) {
    shr_replay(src, dst, hits, n, E, unit, inverse);
}
uint64_t shs_waves(uint64_t n, uint32_t E, uint32_t unit) { return zsh_plan(n, E, unit).waves; }
uint32_t shs_ragged(uint64_t n, uint32_t E, uint32_t unit) { return zsh_plan(n, E, unit).ragged; }
uint64_t shs_piece(uint64_t total, uint64_t max_piece, uint32_t block_size) { return zsh_piece(total, max_piece, block_size); }
int shs_check(uint64_t n, uint32_t E, uint32_t unit, uint32_t src_align, uint32_t dst_align) { return shr_check(n, E, unit, src_align, dst_align, (uint32_t)n); }

/* every n in [n_lo, n_hi]: the alignments walk through 0 .. 15 with n (all = 0), or all 256 pairs (all = 1).
 * -> 0, or 1000 x (n - n_lo + 1) + 10 x the failed check + ... of the first failure; *checked counts the runs */
int64_t shs_sweep(uint32_t E, uint32_t unit, uint64_t n_lo, uint64_t n_hi, int all, uint64_t* checked) {
    for (uint64_t n = n_lo; n <= n_hi; n++)
        for (uint32_t a = 0; a < (all ? 256u : 1u); a++) {
            const uint32_t sa = all ? a >> 4 : (uint32_t)(n & 15u), da = all ? a & 15u : (uint32_t)((n >> 4) + 5u * n + 3u) & 15u;
            const int rc = shr_check(n, E, unit, sa, da, (uint32_t)n);
            if (rc) return (int64_t)(1000u * (n - n_lo + 1u) + (uint64_t)rc);
            ++*checked;
        }
    return 0;
}
