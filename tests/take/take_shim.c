/* Test-only view of zxc_amd/csrc/zxc_take.h for tests/test_decompress_take_device_cpu.py: the session's shape and stated bound,
 * a whole session replayed on the host (take_replay.h: the real container stages, the plan of every chunk, a stand-in decoder that
 * scribbles behind every block, the copies, the events and the verdict, exactly the functions the entry points and kernels of
 * zxc_take_device.hip call), and the promises of one plan. */
#include <stddef.h>

#include "take_replay.h"

size_t t_shape_size(void) { return sizeof(zt_shape_t); }
size_t t_chunk_size(void) { return sizeof(zt_chunk_t); }
int t_shape(uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size, zt_shape_t* s) { return zt_shape(dst_capacity, max_piece, block_size, s); }
uint64_t t_work_bound(uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size) { return zt_work_bound(dst_capacity, max_piece, block_size); }
uint64_t t_chunk_len(uint64_t pos, uint64_t left, uint64_t max_piece, uint32_t block_size) { return zt_chunk_len(pos, left, max_piece, block_size); }
int64_t t_session(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, int want_verify, int use_table,
                  int have_dict, uint32_t dict_id, const uint8_t* blk_bytes, const uint64_t* blk_at, const int32_t* blk_status,
                  uint32_t n_blocks, const uint64_t* lens, uint32_t n_lens, uint32_t align, uint8_t* out) {
    return tr_session(src, src_size, cap, max_piece, bs, want_verify, use_table, have_dict, dict_id, blk_bytes, blk_at, blk_status, n_blocks,
                      lens, n_lens, align, out);
}
/* what the head stage decides for these bytes: -> file_ck | verify << 1 | final << 2 */
uint32_t t_head(const uint8_t* src, uint64_t src_size, uint64_t cap, uint32_t bs, int want_verify) {
    zc_ctl_t c;
    zc_head(src, src_size, cap, bs, want_verify, 1u, &c);
    return c.file_ck | c.verify << 1 | c.final << 2;
}
int t_plan_check(uint64_t pos, uint64_t n, uint64_t room, uint32_t align, uint32_t bs, uint64_t max_piece) {
    return tr_plan_check(pos, n, room, align, bs, max_piece);
}
/* every pos in [0, bs) with every n in [n_lo, n_hi), room n and n + 1000, at this alignment: -> 0, or pos << 40 | n << 8 | the
 * promise broken, of the first plan that fails */
uint64_t t_plan_check_range(uint32_t bs, uint64_t n_lo, uint64_t n_hi, uint32_t align) {
    for (uint32_t pos = 0; pos < bs; pos++)
        for (uint64_t n = n_lo; n < n_hi; n++)
            for (uint64_t extra = 0; extra <= 1000u; extra += 1000u) {
                const int rc = tr_plan_check(7ull * bs + pos, n, n + extra, align, bs, n > bs ? n : bs);
                if (rc) return (uint64_t)pos << 40 | n << 8 | (uint64_t)rc;
            }
    return 0;
}
