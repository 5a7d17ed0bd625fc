/* Test-only view of the dictionary rules of zxc_amd/csrc/zxc_ranges.h for tests/test_dict_device_cpu.py: open in series, then the
 * job and the verdict of a range as zxc_mi355x_decompress_ranges_dict_device runs them, beside those of the call that takes no
 * dictionary. */
#include "../../zxc_amd/csrc/zxc_ranges.h"

uint64_t t_index_size(uint32_t max_blocks) { return zr_index_size(max_blocks); }
void t_open(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* index) {
    zr_open_serial(src, src_size, block_size, max_blocks, index);
}
void t_job_dict(const void* index, const zxc_dev_range_t* r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel, int have_dict, uint32_t have_id,
                zxc_dev_job_t* job, zr_copy_t* cp) {
    zr_job_dict(index, *r, j, job_index, src_size, max_len, dst_capacity, block_size, dst_rel, stage_rel, have_dict, have_id, job, cp);
}
void t_job(const void* index, const zxc_dev_range_t* r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
           uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel, zxc_dev_job_t* job, zr_copy_t* cp) {
    zr_job(index, *r, j, job_index, src_size, max_len, dst_capacity, block_size, dst_rel, stage_rel, job, cp);
}
int64_t t_verdict_dict(const void* index, const zxc_dev_range_t* r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                       uint64_t dst_capacity, uint32_t block_size, int have_dict, uint32_t have_id) {
    return zr_verdict_dict(index, *r, J, status, src_size, max_len, dst_capacity, block_size, have_dict, have_id);
}
int64_t t_verdict(const void* index, const zxc_dev_range_t* r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                  uint64_t dst_capacity, uint32_t block_size) {
    return zr_verdict(index, *r, J, status, src_size, max_len, dst_capacity, block_size);
}
