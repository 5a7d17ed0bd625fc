/* Test-only view of the dictionary rules of zxc_amd/csrc/zxc_appendv.h for tests/test_compress_appendv_dict_device_cpu.py: the
 * scratch's shape without images and its stated bound, and whole dictionary sessions that mix append and appendv_dict replayed on
 * the host (appendv_dict_replay.h: exactly the functions the entry point and the kernels of zxc_append_device.hip call). */
#include <stddef.h>

#include "appendv_dict_replay.h"

size_t t_vshape_size(void) { return sizeof(zav_shape_t); }
size_t t_stats_size(void) { return sizeof(rpvd_stats_t); }
int t_vshape_dict(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, uint32_t dict_size, zav_shape_t* s) {
    return zav_shape_dict(n_iov, max_piece, block_size, dict_size, s);
}
uint64_t t_vbound_dict(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, uint32_t dict_size) {
    return zav_scratch_bound_dict(n_iov, max_piece, block_size, dict_size);
}
int64_t t_check_archive(const uint8_t* comp, uint64_t comp_size, const uint8_t* data, uint64_t total, const uint8_t* dict, uint32_t dict_size,
                        uint32_t seed, uint32_t chunk, rpvd_stats_t* all) {
    return rpvd_check_archive(comp, comp_size, data, total, dict, dict_size, seed, chunk, all);
}
int64_t t_selftest(uint32_t chunk, rpvd_stats_t* all) { return rpvd_selftest(chunk, all); }
int64_t t_bad_table(uint32_t bs, uint32_t dict_size, uint64_t before, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t promised,
                    uint64_t after, int checksum, int seekable, uint64_t max_piece, uint32_t chunk, int small_cap, int* table_status) {
    return rpvd_session_bad_table(bs, dict_size, before, iov, n_iov, promised, after, checksum, seekable, max_piece, chunk, small_cap,
                                  table_status);
}
