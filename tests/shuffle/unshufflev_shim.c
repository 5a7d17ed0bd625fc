/* Test-only: the rules of zxc_amd/csrc/zxc_unshufflev.h behind C-ABI names, for tests/test_decompress_shufflev_device_cpu.py (loaded
 * with ctypes, built with the host C compiler and no sanitizer). */
#include "unshufflev_replay.h"

uint64_t uvs_scratch_size(uint32_t n_iov) { return zsv_scratch_size(n_iov); }
uint64_t uvs_work_size(uint64_t shuffle_ws, uint32_t n_iov) { return zuv_work_size(shuffle_ws, n_iov); }
int64_t uvs_result(int status, int64_t word, uint64_t total) { return zuv_result(status, word, total); }

/* one table at the 16 alignments of its first entry (the later entries walk on from it)
 * -> 0, or 100 x (alignment + 1) + the failed check; out: the entries' bytes of the last run, concatenated */
int uvs_check(const uint8_t* y, const uint64_t* lens, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece, uint8_t* out) {
    for (uint32_t a = 0; a < 16u; a++) {
        const int rc = uvr_check(y, lens, n_iov, total, E, unit, piece, a, out);
        if (rc) return (int)(100u * (a + 1u)) + rc;
    }
    return 0;
}

int uvs_check_bad(const uint8_t* y, const uint64_t* lens, uint32_t n_iov, uint64_t promised, uint32_t null_at, uint32_t E, uint32_t unit,
                  uint64_t piece) {
    return uvr_check_bad(y, lens, n_iov, promised, null_at, E, unit, piece, 0);
}
