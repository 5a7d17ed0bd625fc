/* Test-only view of zxc_amd/csrc/zxc_rangesv_shuffle.h for tests/test_decompress_rangesv_shuffle_device_cpu.py: the shape, job
 * (r, j), the gather plan held against its definition and zsh_index, archives of stored blocks, and whole calls replayed on the host
 * (rangesv_shuffle_replay.h) with the destinations heap buffers between canaries below and above the work area, every store into
 * them counted. */
#include <stddef.h>
#include <stdint.h>

static uint8_t *rs_arena, *rs_hits;
static uint64_t rs_arena_size;
static uint32_t rs_outside; /* stores that left the arena */
static void rs_hit(uint64_t addr, uint32_t n) {
    const uint64_t lo = (uint64_t)(uintptr_t)rs_arena;
    for (uint32_t b = 0; b < n; b++) {
        if (addr + b < lo || addr + b >= lo + rs_arena_size) { rs_outside++; continue; }
        if (rs_hits[addr + b - lo] < 255u) rs_hits[addr + b - lo]++;
    }
}
#define RSR_HIT(addr, n) rs_hit((addr), (n))

#include "../container/stored_archive.h"
#include "rangesv_shuffle_replay.h"

#define RS_CANARY 64u
#define RS_FILL 0xC3

size_t rs_gather_size(void) { return sizeof(zrs_gather_t); }
uint64_t rs_index_size(uint32_t max_blocks) { return zr_index_size(max_blocks); }
void rs_open(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* index) {
    zr_open_serial(src, src_size, block_size, max_blocks, index);
}
int rs_shape(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, zrs_shape_t* s) { return zrs_shape(n_ranges, max_len, block_size, s); }
uint64_t rs_zsh_index(uint64_t p, uint64_t n, uint32_t E, uint32_t unit) { return zsh_index(p, n, E, unit); }

/* the seekable archive of stored blocks of src[0, total) -> its size (0: out is too small) */
uint64_t rs_stored_archive(const uint8_t* src, uint64_t total, uint32_t bs, int checksum, uint8_t* out, uint64_t cap) {
    rp_archive_t a;
    uint64_t size = 0;
    if (rp_stored_archive(src, total, bs, checksum, 1, 0, 0u, &a) && a.size <= cap) {
        memcpy(out, a.comp, a.size);
        size = a.size;
    }
    rp_archive_free(&a);
    return size;
}

/* zrs_job for the range (offset, len, base) and every j < J (job index j): row j of the seven columns out_off, comp_off, comp_size,
 * dst_at, from, n, m */
void rs_jobs(const void* index, uint64_t offset, uint64_t len, uint64_t base, uint32_t J, uint64_t src_size, uint64_t max_len,
             uint32_t block_size, uint64_t out_base, uint64_t stage_rel, uint64_t* cols) {
    for (uint32_t j = 0; j < J; j++) {
        const zxc_dev_rangev_t r = {offset, len, base};
        zxc_dev_job_t job;
        zrs_gather_t ga;
        zrs_job(index, r, j, j, src_size, max_len, block_size, out_base, stage_rel, 0, 0u, &job, &ga);
        cols[j] = job.out_off; cols[J + j] = job.comp_off; cols[2u * J + j] = job.comp_size; cols[3u * J + j] = ga.dst_at;
        cols[4u * J + j] = ga.from; cols[5u * J + j] = ga.n; cols[6u * J + j] = ga.m;
    }
}
int64_t rs_verdict(const void* index, uint64_t offset, uint64_t len, uint64_t base, uint32_t J, const int32_t* status, uint64_t src_size,
                   uint64_t max_len, uint32_t block_size) {
    const zxc_dev_rangev_t r = {offset, len, base};
    return zrs_verdict(index, r, J, status, src_size, max_len, block_size, 0, 0u);
}

/* the sibling's verdict for the same range and statuses */
int64_t rs_zrv_verdict(const void* index, uint64_t offset, uint64_t len, uint64_t base, uint32_t J, const int32_t* status, uint64_t src_size,
                       uint64_t max_len, uint32_t block_size, int have_dict, uint32_t have_id) {
    const zxc_dev_rangev_t r = {offset, len, base};
    return zrv_verdict(index, r, J, status, src_size, max_len, block_size, have_dict, have_id);
}

/* The gather plan of (from[i], n[i]) in a block of m bytes (unit: the block size), i < count, pairs with from + n > m skipped.
 * For every item (chunk c < chunks of the unit): a byte of a whole group is wanted, is a vector byte by the definition restated
 * here, and its place in the planes is zsh_index's; a single byte is wanted, is no vector byte, and zrs_src is zsh_index's; there
 * are at most 2 (16 E - 1) + 127 single bytes per job; every wanted byte has exactly one owner.
 * -> 0 and *checked pairs, else the failed check x 1000000 + the pair's index + 1 */
static int rs_def_vector(uint32_t p, uint32_t from, uint32_t n, uint32_t m, uint32_t E) {
    const uint32_t w = 16u * E, Gq = m / E / 16u, g0 = p / w * w;
    return p < w * Gq && g0 >= from && g0 + w <= from + n;
}
int64_t rs_plan_pairs(uint32_t E, uint32_t m, uint32_t unit, const uint32_t* from, const uint32_t* n, uint32_t count, uint64_t* checked) {
    uint8_t* own = malloc(m ? m : 1u);
    const uint32_t chunks = (unit + ZRS_CHUNK - 1u) / ZRS_CHUNK, q = m / E, w = 16u * E;
    int64_t bad = 0;
    *checked = 0;
    for (uint32_t i = 0; i < count && !bad; i++) {
        const uint32_t f = from[i], len = n[i];
        uint32_t singles = 0;
        if (len == 0 || (uint64_t)f + len > m) continue;
        memset(own + f, 0, len);
#define RS_FAIL(code) { bad = (int64_t)(code) * 1000000 + i + 1; break; }
        for (uint32_t c = 0; c < chunks && !bad; c++) {
            zrs_item_t it;
            if (!zrs_item(f, len, m, E, c, &it)) continue;
            for (uint32_t g = it.g_lo; g < it.g_hi && !bad; g++)
                for (uint32_t j = 0; j < 16u && !bad; j++)
                    for (uint32_t k = 0; k < E; k++) {
                        const uint32_t p = g * w + j * E + k;
                        if (p < f || p >= f + len || p / ZRS_CHUNK != c) RS_FAIL(1)
                        if (!rs_def_vector(p, f, len, m, E) || !zrs_vector_byte(p, f, len, m, E)) RS_FAIL(2)
                        if ((uint64_t)k * q + 16u * g + j != zsh_index(p, m, E, unit)) RS_FAIL(3)
                        own[p]++;
                    }
            for (uint32_t k = 0; k < it.head_n + it.tail_n && !bad; k++) {
                const uint32_t p = zrs_single(&it, k);
                if (p < f || p >= f + len || p / ZRS_CHUNK != c) RS_FAIL(4)
                if (rs_def_vector(p, f, len, m, E) || zrs_vector_byte(p, f, len, m, E)) RS_FAIL(5)
                if (zrs_src(p, m, E) != zsh_index(p, m, E, unit)) RS_FAIL(6)
                own[p]++;
                singles++;
            }
        }
        if (!bad && singles > 2u * (w - 1u) + 127u) RS_FAIL(7)
        for (uint32_t p = f; p < f + len && !bad; p++) if (own[p] != 1u) RS_FAIL(8)
#undef RS_FAIL
        (*checked)++;
    }
    free(own);
    return bad;
}

/* One call over n ranges (offsets[r], lens[r]). Range r's destination is a buffer of 64 + 16 + len + 64 bytes filled with 0xC3 in
 * one arena with the work area: the buffers of even r below the work area, those of odd r above it, the work area itself at an odd
 * address. base mod 16 = (r + shift) mod 16. kinds[r]: 0 that base; 1 a zero base; 2 a base whose end wraps (neither is ever
 * dereferenced; the buffers are judged like the others).
 * -> rsr_call's rc; results[r]; out: the ranges' bytes back to back, out_hits: how often each was stored; flags[r]: bit 0 a byte
 * of the buffer outside [base, base + len) changed or was stored to, bit 1 a byte inside it changed; *stray: stores that left the
 * arena or went into the work area. */
int rs_call(uint64_t src_size, const void* index, const uint64_t* offsets, const uint64_t* lens, const uint32_t* kinds, uint32_t n,
            uint64_t max_len, uint32_t E, uint32_t bs, int have_dict, uint32_t have_id, const uint8_t* blk_bytes, const uint64_t* blk_at,
            const int32_t* blk_status, uint32_t n_blocks, uint32_t shift, int64_t* results, uint8_t* out, uint8_t* out_hits, uint32_t* flags,
            uint32_t* stray) {
    const rvr_blocks_t blk = {blk_bytes, blk_at, blk_status, n_blocks};
    zrs_shape_t s;
    zxc_dev_rangev_t* tab = malloc(((size_t)n + 1u) * sizeof *tab);
    uint64_t* at = malloc(((size_t)n + 1u) * sizeof *at); /* where range r's bytes start in the arena */
    uint64_t* buf_at = malloc(((size_t)n + 1u) * sizeof *buf_at);
    const uint64_t work_bytes = zrs_shape(n, max_len, bs, &s) == 0 ? s.bytes : 0u;
    uint64_t size = 0, work_at = 0;
    for (uint32_t half = 0; half < 2u; half++) {
        for (uint32_t r = half; r < n; r += 2u) { buf_at[r] = size; size += RS_CANARY + 16u + lens[r] + RS_CANARY; }
        if (half == 0) { size += 16u; work_at = size + 3u; size += 3u + work_bytes + 16u; }
    }
    rs_arena = malloc(size); rs_hits = calloc(size, 1); rs_arena_size = size; rs_outside = 0;
    memset(rs_arena, RS_FILL, size);
    for (uint32_t r = 0; r < n; r++) {
        const uint64_t lo = (uint64_t)(uintptr_t)rs_arena + buf_at[r] + RS_CANARY;
        at[r] = buf_at[r] + RS_CANARY + (((r + shift) - lo) & 15u);
        tab[r].offset = offsets[r]; tab[r].len = lens[r];
        tab[r].base = (uint64_t)(uintptr_t)rs_arena + at[r];
        if (kinds[r] == 1u) tab[r].base = 0;
        if (kinds[r] == 2u) tab[r].base = ~(uint64_t)0 - lens[r] / 2u;
    }
    const int rc = rsr_call(src_size, index, tab, n, max_len, E, bs, have_dict, have_id, &blk, rs_arena + work_at, work_bytes, results);
    uint64_t o = 0;
    for (uint32_t r = 0; r < n; r++) {
        const uint64_t lo = at[r], hi = lo + lens[r], end = buf_at[r] + RS_CANARY + 16u + lens[r] + RS_CANARY;
        flags[r] = 0;
        for (uint64_t b = buf_at[r]; b < end; b++) {
            const int inside = b >= lo && b < hi;
            if (rs_arena[b] != RS_FILL) flags[r] |= inside ? 2u : 1u;
            if (!inside && rs_hits[b]) flags[r] |= 1u;
        }
        memcpy(out + o, rs_arena + lo, lens[r]);
        memcpy(out_hits + o, rs_hits + lo, lens[r]);
        o += lens[r];
    }
    *stray = rs_outside;
    for (uint64_t b = work_at - 19u; b < work_at + work_bytes + 16u; b++) *stray += rs_hits[b] != 0; /* the gather stores into no work area */
    free(rs_hits); free(rs_arena); free(buf_at); free(at); free(tab);
    rs_arena = rs_hits = NULL;
    return rc;
}
