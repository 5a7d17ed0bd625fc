/* Test-only view of zxc_amd/csrc/zxc_container.h for tests/test_decompress_device_cpu.py: the head stage, the seek-table path or
 * the walk, and the verdict, driven in series exactly as the kernels of zxc_unframe_device.hip drive them in launches. */
#include <string.h>

#include "../../zxc_amd/csrc/zxc_container.h"

size_t t_ctl_size(void) { return sizeof(zc_ctl_t); }
size_t t_shape_size(void) { return sizeof(zc_shape_t); }
int t_shape(uint64_t dst_capacity, uint32_t block_size, zc_shape_t* s) { return zc_shape(dst_capacity, block_size, s); }

/* clear, head, then the table (use_table) with the walk behind it, or the walk alone. -> 1 when the table's chain was used */
int t_plan(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, int want_verify, int use_table,
           uint32_t n_jobs, uint32_t k_direct, zc_ctl_t* c, zxc_dev_job_t* jobs) {
    memset(jobs, 0, (size_t)n_jobs * sizeof *jobs);
    zc_head(src, src_size, dst_capacity, block_size, want_verify, n_jobs, c);
    if (c->final) return 0;
    if (use_table && zc_seek_plan(src, block_size, k_direct, c, jobs)) return 1;
    memset(jobs, 0, (size_t)n_jobs * sizeof *jobs);
    zc_walk(src, src_size, block_size, k_direct, n_jobs, c, jobs);
    return 0;
}

/* the events pass and the result */
int64_t t_verdict(zc_ctl_t* c, const int32_t* status, uint32_t block_size, uint64_t dst_capacity) {
    if (!c->final)
        for (uint32_t i = 0; i < c->found; i++) {
            const int32_t ev = zc_block_event(i, status[i], c->found, c->done, block_size, dst_capacity);
            if (ev != 0 && zc_event_key(i, ev) < c->event) c->event = zc_event_key(i, ev);
        }
    return zc_verdict(c, (!c->final && c->found) ? status[c->found - 1u] : 0, block_size);
}
uint32_t t_tail_bytes(uint32_t i, int32_t status, uint32_t block_size, uint64_t dst_capacity) {
    return zc_tail_bytes(i, status, block_size, dst_capacity);
}

/* ---- the writers, for tests/test_container_writers_cpu.py */
int t_file_header(const uint8_t* h, uint32_t* lg, uint32_t* file_ck, uint32_t* dict_id) { return zc_file_header(h, lg, file_ck, dict_id); }
void t_put_file_header(uint8_t* p, uint32_t lg, int file_ck, int has_dict, uint32_t dict_id) { zc_put_file_header(p, lg, file_ck, has_dict, dict_id); }
void t_put_blk_hdr(uint8_t* p, uint32_t type, uint32_t csz) { zc_st_le(p, zc_blk_hdr(type, csz), ZC_BLK_HDR); }
void t_put_footer(uint8_t* p, uint64_t total, uint32_t hash) { zc_put_footer(p, total, hash); }
uint32_t t_block_size_lg(uint64_t bs) { return zc_block_size_lg(bs); }
uint32_t t_hash_fold(uint32_t h, uint32_t trailer) { return zc_hash_fold(h, trailer); }
/* -> 1 and the EOF header's offset when the archive ends in a seek table of nb entries */
int t_seek_tail(const uint8_t* src, uint64_t src_size, uint64_t nb, uint64_t* eof_at) {
    uint64_t eof = 0;
    return zc_seek_tail(src, src_size, nb, eof_at, &eof);
}
/* the chain from offset 16 to its end: -> the offset of the EOF block it ends at without an error, else -1 */
int64_t t_chain_eof(const uint8_t* src, uint64_t src_size, uint32_t file_ck) {
    zc_chain_t c = {ZC_FILE_HDR, 0, 0, 0, 0};
    while (!c.done) (void)zc_chain_next(src, src_size, file_ck, 0, &c);
    return c.saw_eof && c.tail_err == 0 ? (int64_t)c.ip : -1;
}
