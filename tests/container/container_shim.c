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
