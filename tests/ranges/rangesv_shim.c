/* Test-only view of zxc_amd/csrc/zxc_rangesv.h for tests/test_decompress_rangesv_device_cpu.py: the early verdict, job (r, j) and
 * the direct rule over a column of ranges as the kernels of zxc_ranges_device.hip call them, and whole calls replayed on the host
 * (rangesv_replay.h) with every destination a heap buffer of its own between canaries. */
#include <stddef.h>

#include "rangesv_replay.h"

#define RV_CANARY 64u
#define RV_FILL 0xC3

size_t rv_rangev_size(void) { return sizeof(zxc_dev_rangev_t); }
uint64_t rv_index_size(uint32_t max_blocks) { return zr_index_size(max_blocks); }
void rv_open(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* index) {
    zr_open_serial(src, src_size, block_size, max_blocks, index);
}
int rv_shape(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, zr_shape_t* s) { return zr_shape(n_ranges, max_len, block_size, s); }
/* -> 1 and *result when the range is answered before its blocks, else 0 */
int rv_final(const void* index, const zxc_dev_rangev_t* r, uint64_t src_size, uint64_t max_len, uint32_t block_size, int have_dict,
             uint32_t have_id, int64_t* result) {
    return zrv_range_final((const zr_index_t*)index, *r, src_size, max_len, block_size, have_dict, have_id, result);
}
/* zrv_job and zrv_direct for the ranges (offset, lens[i], base), i < n_lens, and every j < J (job index j): row i J + j of the six
 * output columns out_off, comp_size, dst_at, from, n, direct */
void rv_jobs(const void* index, uint64_t offset, const uint64_t* lens, uint32_t n_lens, uint64_t base, uint32_t J, uint64_t src_size,
             uint64_t max_len, uint32_t block_size, uint64_t out_base, uint64_t stage_rel, uint64_t* cols) {
    const uint64_t rows = (uint64_t)n_lens * J;
    for (uint32_t i = 0; i < n_lens; i++)
        for (uint32_t j = 0; j < J; j++) {
            const zxc_dev_rangev_t r = {offset, lens[i], base};
            const uint64_t row = (uint64_t)i * J + j;
            zxc_dev_job_t job;
            zr_copy_t cp;
            zrv_job(index, r, j, j, src_size, max_len, block_size, out_base, stage_rel, 0, 0u, &job, &cp);
            cols[row] = job.out_off; cols[rows + row] = job.comp_size; cols[2u * rows + row] = cp.dst_at;
            cols[3u * rows + row] = cp.from; cols[4u * rows + row] = cp.n;
            cols[5u * rows + row] = (uint64_t)zrv_direct(r, offset / block_size + j, block_size);
        }
}

/* One call over n ranges (offsets[r], lens[r]). Range r's destination is a heap buffer of 64 + 16 + len + 64 bytes filled with
 * 0xC3, its base at 64 + k inside it: k = offset mod 16 for even r (the direct path), every other residue in turn for odd r
 * (`shift` moves the turn). kinds[r]: 0 that base; 1 a zero base; 2 a base whose end wraps. The table entries of kinds 1 and 2
 * are never dereferenced; their buffers are judged like the others.
 * -> rvr_call's rc; results[r]; out: the ranges' bytes back to back; flags[r]: bit 0 a byte outside [base, base + len) of the
 * buffer changed, bit 1 a byte inside it changed. */
int rv_call(uint64_t src_size, const void* index, const uint64_t* offsets, const uint64_t* lens, const uint32_t* kinds, uint32_t n,
            uint64_t max_len, uint32_t bs, int have_dict, uint32_t have_id, const uint8_t* blk_bytes, const uint64_t* blk_at,
            const int32_t* blk_status, uint32_t n_blocks, uint32_t shift, int64_t* results, uint8_t* out, uint32_t* flags) {
    const rvr_blocks_t blk = {blk_bytes, blk_at, blk_status, n_blocks};
    zxc_dev_rangev_t* tab = malloc(((size_t)n + 1u) * sizeof *tab);
    uint8_t** buf = malloc(((size_t)n + 1u) * sizeof *buf);
    uint32_t* ks = malloc(((size_t)n + 1u) * sizeof *ks);
    for (uint32_t r = 0; r < n; r++) {
        const size_t size = RV_CANARY + 16u + lens[r] + RV_CANARY;
        ks[r] = (uint32_t)((offsets[r] + ((r & 1u) ? 1u + ((r >> 1) + shift) % 15u : 0u)) & 15u);
        buf[r] = malloc(size);
        memset(buf[r], RV_FILL, size);
        tab[r].offset = offsets[r]; tab[r].len = lens[r];
        tab[r].base = (uint64_t)(uintptr_t)(buf[r] + RV_CANARY + ks[r]);
        if (kinds[r] == 1u) tab[r].base = 0;
        if (kinds[r] == 2u) tab[r].base = ~(uint64_t)0 - lens[r] / 2u;
    }
    const int rc = rvr_call(src_size, index, tab, n, max_len, bs, have_dict, have_id, &blk, results);
    uint64_t at = 0;
    for (uint32_t r = 0; r < n; r++) {
        const size_t lo = RV_CANARY + ks[r], hi = lo + lens[r], size = RV_CANARY + 16u + lens[r] + RV_CANARY;
        flags[r] = 0;
        for (size_t b = 0; b < size; b++)
            if (buf[r][b] != RV_FILL) flags[r] |= (b < lo || b >= hi) ? 1u : 2u;
        memcpy(out + at, buf[r] + lo, lens[r]);
        at += lens[r];
        free(buf[r]);
    }
    free(ks); free(buf); free(tab);
    return rc;
}
