/* Test-only view of zxc_amd/csrc/zxc_append.h for tests/test_compress_append_device_cpu.py: the session's shape and stated bound,
 * a whole session replayed on the host (append_replay.h: the plan of every piece, its copies and jobs, the advance, the finish and
 * a byte gather, exactly the functions the entry points and kernels of zxc_append_device.hip call), and the promises of one plan. */
#include <stddef.h>

#include "append_replay.h"

size_t t_shape_size(void) { return sizeof(zap_shape_t); }
size_t t_ctl_size(void) { return sizeof(zap_ctl_t); }
size_t t_piece_size(void) { return sizeof(zap_piece_t); }
int t_shape(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable, zap_shape_t* s) {
    return zap_shape(max_total, max_piece, block_size, slot_stride, seekable, s);
}
uint64_t t_work_bound(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable) {
    return zap_work_bound(max_total, max_piece, block_size, slot_stride, seekable);
}
uint64_t t_piece_len(uint32_t carry, uint64_t left, uint64_t max_piece, uint32_t block_size) {
    return zap_piece_len(carry, left, max_piece, block_size);
}
int64_t t_session(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                  uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, uint32_t n_lens, uint64_t max_piece,
                  uint8_t* dst, uint64_t cap) {
    return rp_session(src, total, blocks, blk_at, blk_size, n_blocks, bs, checksum, seekable, lens, n_lens, max_piece, dst, cap);
}
int t_plan_check(uint32_t carry, uint64_t n, uint32_t bs) { return rp_plan_check(carry, n, bs); }
/* every carry in [0, bs) with every n in [n_lo, n_hi): -> 0, or carry << 40 | n << 8 | the promise broken, of the first plan that fails */
uint64_t t_plan_check_range(uint32_t bs, uint64_t n_lo, uint64_t n_hi) {
    for (uint32_t carry = 0; carry < bs; carry++)
        for (uint64_t n = n_lo; n < n_hi; n++) {
            const int rc = rp_plan_check(carry, n, bs);
            if (rc) return (uint64_t)carry << 40 | n << 8 | (uint64_t)rc;
        }
    return 0;
}
/* the hash carried over pieces against the serial fold: trailers t[0 .. n), cut into pieces of `piece` blocks */
uint32_t t_hash_in_pieces(const uint32_t* t, uint32_t n, uint32_t piece) {
    uint32_t h = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += piece) {
        const uint32_t nb = n - b0 < piece ? n - b0 : piece;
        uint32_t ph = 0;
        for (uint32_t b = 0; b < nb; b++) ph ^= zc_rotl(t[b0 + b], (nb - 1u - b) & 31u);
        h = zc_rotl(h, nb & 31u) ^ ph;
    }
    return h;
}
uint32_t t_hash_serial(const uint32_t* t, uint32_t n) {
    uint32_t h = 0;
    for (uint32_t b = 0; b < n; b++) h = zc_hash_fold(h, t[b]);
    return h;
}
