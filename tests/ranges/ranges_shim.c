/* Test-only view of zxc_amd/csrc/zxc_ranges.h for tests/test_decompress_ranges_device_cpu.py: the open passes in series, the
 * job and copy descriptor of (r, j), the direct / staged decision, the per-range verdict and the call's shape, exactly the
 * functions the kernels of zxc_ranges_device.hip call. */
#include <stddef.h>

#include "../../zxc_amd/csrc/zxc_ranges.h"

size_t t_index_hdr_size(void) { return sizeof(zr_index_t); }
size_t t_copy_size(void) { return sizeof(zr_copy_t); }
size_t t_shape_size(void) { return sizeof(zr_shape_t); }
size_t t_range_size(void) { return sizeof(zxc_dev_range_t); }
uint64_t t_index_size(uint32_t max_blocks) { return zr_index_size(max_blocks); }
void t_open(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* index) {
    zr_open_serial(src, src_size, block_size, max_blocks, index);
}
int t_shape(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, zr_shape_t* s) { return zr_shape(n_ranges, max_len, block_size, s); }
void t_job(const void* index, const zxc_dev_range_t* r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
           uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel, zxc_dev_job_t* job, zr_copy_t* cp) {
    zr_job(index, *r, j, job_index, src_size, max_len, dst_capacity, block_size, dst_rel, stage_rel, job, cp);
}
int t_direct(const zxc_dev_range_t* r, uint64_t b, uint32_t block_size) { return zr_direct(*r, b, block_size); }
int64_t t_verdict(const void* index, const zxc_dev_range_t* r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                  uint64_t dst_capacity, uint32_t block_size) {
    return zr_verdict(index, *r, J, status, src_size, max_len, dst_capacity, block_size);
}
