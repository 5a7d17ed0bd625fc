/* Test-only view of zxc_amd/csrc/zxc_cpack.h for tests/test_compress_pack_device_cpu.py, and the stages of
 * zxc_mi355x_compress_pack_device run the way the kernels of zxc_cbatch_device.hip group them: a tile of 1024 items per
 * "workgroup", 256 "threads" of four consecutive items each, the tiles' words scanned by one workgroup whose thread t owns
 * ceil(n_tiles / 256) consecutive tiles. Every rule is the header's; only the loops that stand for the launches are here.
 * tests/batch/cpack_san_main.c includes this file. */
#include <stddef.h>

#include "../../zxc_amd/csrc/zxc_cpack.h"

#define T_THREADS 256u
#define T_PER (ZC_TILE_BLOCKS / T_THREADS)

size_t t_pshape_size(void) { return sizeof(zcp_shape_t); }
int t_pshape(uint32_t n_items, uint64_t max_size, uint32_t block_size, uint32_t slot_stride, uint32_t dict_size, zcp_shape_t* s) {
    return zcp_shape(n_items, max_size, block_size, slot_stride, dict_size, s);
}
int t_align_ok(uint32_t align) { return zcp_align_ok(align); }
uint64_t t_extent(const zcb_rec_t* rec, uint32_t align) { return zcp_extent(rec, align); }

/* plan: one thread per item */
void t_pack_plan(const zxc_dev_item_t* items, uint32_t n, uint32_t J, uint64_t src_capacity, uint64_t max_size, uint32_t block_size,
                 int checksum, int seekable, zcb_rec_t* recs, zxc_enc_job_t* jobs) {
    for (uint32_t r = 0; r < n; r++) zcp_plan_item(items[r], r, J, src_capacity, max_size, block_size, checksum, seekable, recs + r, jobs);
}

/* size + reduce, scan, place: tiles has ceil(n / 1024) words; *end is the end word (cleared by the scan, raised by the place) */
void t_pack_layout(zcb_rec_t* recs, uint32_t n, uint32_t J, const uint32_t* sizes, uint32_t block_size, int checksum, int seekable,
                   uint32_t align, uint64_t dst_capacity, uint64_t* tiles, uint64_t* end) {
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS);
    for (uint32_t tile = 0; tile < n_tiles; tile++) { /* zxc_cpack_size_kernel */
        uint64_t all = 0;
        for (uint32_t t = 0; t < T_THREADS; t++) {
            const uint64_t r0 = (uint64_t)tile * ZC_TILE_BLOCKS + t * T_PER;
            uint64_t sum = 0;
            for (uint32_t j = 0; j < T_PER && r0 + j < n; j++) {
                zcp_size_item(recs + r0 + j, sizes + (r0 + j) * J, block_size, checksum, seekable);
                sum += zcp_extent(recs + r0 + j, align);
            }
            all += sum;
        }
        tiles[tile] = all;
    }
    { /* zxc_cpack_scan_kernel */
        const uint32_t per = (n_tiles + 255u) / 256u;
        uint64_t lower = 0; /* the sums of all lower threads */
        for (uint32_t t = 0; t < 256u; t++) {
            const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
            uint64_t run = lower;
            for (uint32_t i = lo; i < hi; i++) {
                const uint64_t s = tiles[i];
                tiles[i] = run;
                run += s;
            }
            lower = run;
        }
        *end = 0;
    }
    for (uint32_t tile = 0; tile < n_tiles; tile++) { /* zxc_cpack_place_kernel */
        uint64_t lower = 0;
        for (uint32_t t = 0; t < T_THREADS; t++) {
            const uint64_t r0 = (uint64_t)tile * ZC_TILE_BLOCKS + t * T_PER;
            uint64_t run = tiles[tile] + lower;
            for (uint32_t j = 0; j < T_PER && r0 + j < n; j++) {
                const uint64_t ext = zcp_extent(recs + r0 + j, align);
                const uint64_t e = zcp_place_item(recs + r0 + j, run, dst_capacity);
                if (e > *end) *end = e; /* the atomic max */
                run += ext;
                lower += ext;
            }
        }
    }
}

/* finish (one thread per item), then the gather (one job at a time) */
void t_pack_finish(zcb_rec_t* recs, uint32_t n, uint32_t J, const uint32_t* sizes, uint64_t* offsets, const uint8_t* slots,
                   uint32_t slot_stride, uint8_t* dst, uint32_t block_size, int checksum, int seekable, int has_dict, uint32_t dict_id) {
    for (uint32_t r = 0; r < n; r++) {
        const uint64_t first = (uint64_t)r * J;
        zcb_finish_item(recs + r, sizes + first, offsets + first, slots + first * slot_stride, slot_stride, dst, block_size, checksum,
                        seekable, has_dict, dict_id);
    }
    for (uint64_t i = 0; i < (uint64_t)n * J; i++) {
        const zcb_rec_t* rec = recs + i / J;
        if (!zcb_gathers(rec, (uint32_t)(i % J))) continue;
        for (uint32_t k = 0; k < sizes[i]; k++) dst[rec->dst_off + offsets[i] + k] = slots[i * slot_stride + k];
    }
}

/* results: packed may be the item table itself */
void t_pack_results(const zcb_rec_t* recs, uint32_t n, const uint64_t* end, zxc_dev_item_t* packed, int64_t* results, uint64_t* total) {
    for (uint32_t r = 0; r < n; r++) {
        results[r] = recs[r].result;
        packed[r] = zcp_packed_item(recs + r);
    }
    if (n) *total = *end;
}
