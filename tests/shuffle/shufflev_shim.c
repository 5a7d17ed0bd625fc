/* Test-only: the rules of zxc_amd/csrc/zxc_shufflev.h behind C-ABI names, for tests/test_compress_shufflev_device_cpu.py (loaded
 * with ctypes, built with the host C compiler and no sanitizer). */
#include "shufflev_replay.h"

uint64_t svs_scratch_size(uint32_t n_iov) { return zsv_scratch_size(n_iov); }
uint64_t svs_scratch_bound(uint32_t n_iov) { return zsv_scratch_bound(n_iov); }
uint64_t svs_work_size(uint64_t shuffle_ws, uint32_t n_iov) { return zsv_work_size(shuffle_ws, n_iov); }
int64_t svs_result(int status, int64_t word) { return zsv_result(status, word); }

/* one table at the 16 alignments of its first entry (the later entries walk on from it), the destination's walking along
 * -> 0, or 100 x (alignment + 1) + the failed check; out: the result of the last run */
int svs_check(const uint8_t* x, const uint64_t* lens, uint32_t n_iov, uint64_t total, uint32_t E, uint32_t unit, uint64_t piece, uint8_t* out) {
    for (uint32_t a = 0; a < 16u; a++) {
        const int rc = svr_check(x, lens, n_iov, total, E, unit, piece, a, (a * 7u + 3u) & 15u, out);
        if (rc) return (int)(100u * (a + 1u)) + rc;
    }
    return 0;
}

int svs_check_bad(const uint8_t* x, const uint64_t* lens, uint32_t n_iov, uint64_t promised, uint32_t null_at, uint32_t E, uint32_t unit,
                  uint64_t piece) {
    return svr_check_bad(x, lens, n_iov, promised, null_at, E, unit, piece, 0);
}
