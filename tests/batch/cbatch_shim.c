/* Test-only view of zxc_amd/csrc/zxc_cbatch.h for tests/test_compress_batch_device_cpu.py: the call's shape, an item's effective
 * capacity and source bounds, the plan of one item, the chunk arithmetic of the dictionary call, the finish of one item and the
 * gather's predicate, exactly the functions the kernels of zxc_cbatch_device.hip call. */
#include <stddef.h>

#include "../../zxc_amd/csrc/zxc_cbatch.h"

size_t t_rec_size(void) { return sizeof(zcb_rec_t); }
size_t t_item_size(void) { return sizeof(zxc_dev_item_t); }
size_t t_shape_size(void) { return sizeof(zcb_shape_t); }
size_t t_job_size(void) { return sizeof(zxc_enc_job_t); }
int t_shape(uint32_t n_items, uint64_t max_size, uint32_t block_size, uint32_t slot_stride, uint32_t dict_size, zcb_shape_t* s) {
    return zcb_shape(n_items, max_size, block_size, slot_stride, dict_size, s);
}
uint64_t t_cap(const zxc_dev_item_t* it, uint64_t dst_capacity) { return zcb_cap(*it, dst_capacity); }
int t_src_ok(const zxc_dev_item_t* it, uint64_t src_capacity) { return zcb_src_ok(*it, src_capacity); }
uint64_t t_known_size(uint64_t nb, int checksum, int seekable) { return zc_known_size(nb, checksum, seekable); }
uint64_t t_image_chunk(uint32_t block_size, uint32_t dict_size) { return zc_image_chunk(block_size, dict_size); }
uint32_t t_chunk_len(const zcb_shape_t* s, uint32_t c0) { return zcb_chunk_len(s, c0); }
void t_plan_item(const zxc_dev_item_t* it, uint32_t r, uint32_t J, uint64_t src_capacity, uint64_t max_size, uint64_t dst_capacity,
                 uint32_t block_size, int checksum, int seekable, zcb_rec_t* rec, zxc_enc_job_t* jobs) {
    zcb_plan_item(*it, r, J, src_capacity, max_size, dst_capacity, block_size, checksum, seekable, rec, jobs);
}
void t_finish_item(zcb_rec_t* rec, const uint32_t* sizes, uint64_t* offsets, const uint8_t* slots, uint32_t slot_stride, uint8_t* dst,
                   uint32_t block_size, int checksum, int seekable, int has_dict, uint32_t dict_id) {
    zcb_finish_item(rec, sizes, offsets, slots, slot_stride, dst, block_size, checksum, seekable, has_dict, dict_id);
}
int t_gathers(const zcb_rec_t* rec, uint32_t b) { return zcb_gathers(rec, b); }
