/* Test-only view of zxc_amd/csrc/zxc_appendv.h for tests/test_compress_appendv_device_cpu.py: the scratch's shape and stated
 * bound, the table check, the placement rule against a walk over the entries, and whole sessions that mix append and appendv
 * replayed on the host (appendv_replay.h: exactly the functions the entry point and the kernels of zxc_append_device.hip call). */
#include <stddef.h>

#include "appendv_replay.h"

size_t t_vshape_size(void) { return sizeof(zav_shape_t); }
size_t t_vctl_size(void) { return sizeof(zav_ctl_t); }
size_t t_iov_size(void) { return sizeof(zxc_dev_iov_t); }
int t_vshape(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, zav_shape_t* s) { return zav_shape(n_iov, max_piece, block_size, s); }
uint64_t t_vbound(uint32_t n_iov, uint64_t max_piece, uint32_t block_size) { return zav_scratch_bound(n_iov, max_piece, block_size); }

/* the table's verdict; starts may be NULL */
int t_table_check(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint64_t* starts) {
    uint64_t* mine = starts ? starts : malloc(((size_t)n_iov + 1u) * 8u);
    const int rc = zav_scan_serial(iov, n_iov, total, mine);
    if (!starts) free(mine);
    return rc;
}
/* the same verdict from tiles of `tile` entries added up on their own and then together, as the kernels group them */
int t_table_check_tiled(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint32_t tile) {
    uint64_t sum = 0;
    uint32_t flags = 0;
    for (uint32_t r0 = 0; r0 < n_iov; r0 += tile) {
        uint64_t ts = 0;
        for (uint32_t r = r0; r < n_iov && r < r0 + tile; r++) {
            ts = zav_sat_add(ts, iov[r].len);
            flags |= zav_entry_flags(iov[r].base, iov[r].len, total);
        }
        sum = zav_sat_add(sum, ts);
    }
    return zav_table_status(flags, sum, total);
}
/* the session's status behind a table's verdict */
int64_t t_fold(int64_t before, int status) {
    zap_ctl_t c;
    zap_begin(&c);
    c.status = before;
    zav_fold_status(&c, status);
    return c.status;
}

/* Placement: for every offset v at which a whole block of the concatenation can start, the rule (zav_find + zav_in_place, as
 * zav_prep applies them) against a walk over the entries: in place exactly when the entry that holds byte v also holds bytes
 * [v, v + bs + 32). -> 0, or v + 1 of the first offset at which they differ; *n_in_place counts the offsets in place. */
uint64_t t_placement(const uint64_t* lens, uint32_t n_iov, uint32_t bs, uint64_t* n_in_place) {
    uint64_t* starts = malloc(((size_t)n_iov + 1u) * 8u);
    uint64_t total = 0, bad = 0;
    for (uint32_t r = 0; r < n_iov; r++) { starts[r] = total; total += lens[r]; }
    starts[n_iov] = total;
    *n_in_place = 0;
    uint32_t walk = 0;
    for (uint64_t v = 0; v + bs <= total && !bad; v++) {
        while (v >= starts[walk] + lens[walk]) walk++; /* the entry that holds byte v: the walk skips empty ones */
        const int want = v + bs + ZAP_OVERREAD <= starts[walk] + lens[walk];
        const uint32_t r = zav_find(starts, 0u, n_iov - 1u, v);
        const int got = zav_in_place(v - starts[r], starts[r + 1u] - starts[r], bs);
        if (r != walk || got != want) bad = v + 1u;
        /* never when an entry boundary or fewer than 32 bytes of its entry lie behind it */
        if (got && (starts[r + 1u] < v + bs + ZAP_OVERREAD || lens[r] == 0)) bad = v + 1u;
        *n_in_place += (uint64_t)got;
    }
    free(starts);
    return bad;
}

int64_t t_vsession(const uint8_t* src, uint64_t total, const uint8_t* blocks, const uint64_t* blk_at, const uint32_t* blk_size,
                   uint32_t n_blocks, uint32_t bs, int checksum, int seekable, const uint64_t* lens, const uint32_t* counts, uint32_t n_calls,
                   uint64_t max_piece, uint8_t* dst, uint64_t cap, rpv_stats_t* st) {
    return rpv_session(src, total, blocks, blk_at, blk_size, n_blocks, bs, checksum, seekable, lens, counts, n_calls, max_piece, dst, cap, st);
}
int64_t t_bad_table(const uint8_t* src, uint64_t before, const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t promised, uint32_t bs,
                    int checksum, int seekable, uint64_t max_piece, uint8_t* dst, uint64_t cap, int* table_status) {
    return rpv_session_bad_table(src, before, iov, n_iov, promised, bs, checksum, seekable, max_piece, dst, cap, table_status);
}
