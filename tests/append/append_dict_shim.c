/* Test-only view of the dictionary session's rules in zxc_amd/csrc/zxc_append.h for tests/test_compress_append_dict_device_cpu.py:
 * the shape with its image area and the stated bound, the images-mode plan and its promises, and whole sessions replayed on the
 * host (append_dict_replay.h) over archives whose header carries a dictionary id. */
#include <stddef.h>

#include "append_dict_replay.h"

size_t t_shape_images_size(void) { return sizeof(zap_shape_images_t); }
int t_shape_images(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable, uint32_t dict_size,
                   zap_shape_images_t* s) {
    return zap_shape_images(max_total, max_piece, block_size, slot_stride, seekable, dict_size, s);
}
uint64_t t_work_bound_images(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable,
                             uint32_t dict_size) {
    return zap_work_bound_images(max_total, max_piece, block_size, slot_stride, seekable, dict_size);
}
uint64_t t_image_chunk(uint32_t block_size, uint32_t dict_size) { return zc_image_chunk(block_size, dict_size); }
int t_plan_check_images(uint32_t carry, uint64_t n, uint32_t bs) { return rpd_plan_check(carry, n, bs); }
/* the plan's numbers for the test to look at: nb, n_direct, n_staged, tail, swap, the lengths of job 0's two segments */
void t_plan_images(uint32_t carry, uint64_t n, uint32_t bs, uint32_t out[7]) {
    zap_piece_t p;
    zap_plan_piece_images(carry, n, bs, &p);
    out[0] = p.nb; out[1] = p.n_direct; out[2] = p.n_staged; out[3] = p.tail; out[4] = p.swap; out[5] = out[6] = 0;
    if (p.nb) {
        const zap_src2_t s = zap_job_images(&p, 0);
        out[5] = s.seg[0].len; out[6] = s.seg[1].len;
    }
}
/* the finished header of an empty dictionary session: 16 bytes */
void t_finish_header(uint32_t block_size, int checksum, uint32_t dict_id, uint8_t* dst, uint64_t cap) {
    zap_ctl_t c;
    zap_begin(&c);
    zap_finish_dict(&c, dst, cap, 0u, block_size, checksum, 0, 1, dict_id);
}
int64_t t_check_archive(const uint8_t* comp, uint64_t comp_size, const uint8_t* data, uint64_t total, const uint8_t* dict,
                        uint32_t dict_size, uint32_t seed, int dense) {
    return rpd_check_archive(comp, comp_size, data, total, dict, dict_size, seed, dense);
}
int64_t t_selftest(void) { return rpd_selftest(); }
