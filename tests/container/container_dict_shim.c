/* Test-only view of the dictionary rule of zxc_amd/csrc/zxc_container.h for tests/test_dict_device_cpu.py: the head stage as
 * zxc_mi355x_decompress_dict_device runs it, and beside it the head stage of the call that takes no dictionary. */
#include "../../zxc_amd/csrc/zxc_container.h"

size_t t_ctl_size(void) { return sizeof(zc_ctl_t); }
void t_head_dict(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint32_t n_jobs,
                 zc_ctl_t* c, int have_dict, uint32_t have_id) {
    zc_head_dict(src, src_size, dst_capacity, block_size, want_verify, n_jobs, c, have_dict, have_id);
}
void t_head(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint32_t n_jobs,
            zc_ctl_t* c) {
    zc_head(src, src_size, dst_capacity, block_size, want_verify, n_jobs, c);
}
/* the 16-bit header check as the finish pass of zxc_mi355x_compress_dict_device computes it: over the two little-endian words */
uint16_t t_hdr_hash16(uint64_t lo, uint64_t hi) { return zc_hdr_hash16(lo, hi); }
