/* Test-only view of zxc_amd/csrc/zxc_batch.h for tests/test_decompress_batch_device_cpu.py: the call's shape, an item's effective
 * capacity, the plan of one item, the direct / staged decision, the bytes a copy-out moves and the per-item verdict, exactly the
 * functions the kernels of zxc_batch_device.hip call. */
#include <stddef.h>

#include "../../zxc_amd/csrc/zxc_batch.h"

size_t t_rec_size(void) { return sizeof(zb_rec_t); }
size_t t_item_size(void) { return sizeof(zxc_dev_item_t); }
size_t t_shape_size(void) { return sizeof(zb_shape_t); }
size_t t_job_size(void) { return sizeof(zxc_dev_job_t); }
int t_shape(uint32_t n_items, uint64_t max_capacity, uint32_t block_size, zb_shape_t* s) { return zb_shape(n_items, max_capacity, block_size, s); }
uint64_t t_cap(const zxc_dev_item_t* it, uint64_t max_capacity, uint64_t dst_capacity) { return zb_cap(*it, max_capacity, dst_capacity); }
int t_src_ok(const zxc_dev_item_t* it, uint64_t src_capacity) { return zb_src_ok(*it, src_capacity); }
void t_plan_item(const uint8_t* src, uint64_t src_capacity, const zxc_dev_item_t* it, uint32_t r, uint32_t J, uint32_t n_jobs,
                 uint64_t max_capacity, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint64_t dst_rel, uint64_t stage_rel,
                 int have_dict, uint32_t have_id, zb_rec_t* rec, zxc_dev_job_t* jobs) {
    zb_plan_item(src, src_capacity, *it, r, J, n_jobs, max_capacity, dst_capacity, block_size, want_verify, dst_rel, stage_rel, have_dict,
                 have_id, rec, jobs);
}
int t_direct(uint64_t dst_off, uint32_t i, uint32_t block_size, uint64_t cap) { return zb_direct(dst_off, i, block_size, cap); }
uint32_t t_copy_bytes(const zb_rec_t* rec, uint32_t i, int32_t status, uint32_t block_size) { return zb_copy_bytes(rec, i, status, block_size); }
int64_t t_verdict_item(const zb_rec_t* rec, const int32_t* status, uint32_t block_size) { return zb_verdict_item(rec, status, block_size); }
