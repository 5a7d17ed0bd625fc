/* Stand-alone program (its own main, not loaded into anything) that replays zxc_mi355x_decompress_rangesv_device the way the entry
 * point and kernels of zxc_ranges_device.hip run it (rangesv_replay.h), where every range's destination is a heap buffer of exactly
 * its length (plus k bytes in front for a base k mod 16) and the work area one of exactly its size, so that AddressSanitizer and
 * UBSan see any read or write outside either: the decoders' spill behind a block decoded in its destination, a 16-byte store of the
 * copy-out that passes a range's end, a job that leaves the index. The archives are tests/container/stored_archive.h's (every block
 * a stored block, seek table, with a trailer when checksums are on), opened by the real open passes; the decoder is the replay's
 * stand-in, which scribbles 32 bytes behind every block. Block sizes 4 KiB and 64 KiB, with and without checksums; sizes of 1, a
 * block - 1, a block, a block + 1, several blocks + 5 and 40 blocks; a seeded table per archive: the fixed edge ranges (whole
 * archive, first and last byte, seams, a block, a block + 31 / + 32 / + 33, two and three blocks), random ranges, and the refused
 * ones (empty, past the end, longer than max_len, a zero base, a wrapping base), at every alignment of base against offset.
 * Built by tests/test_decompress_rangesv_device_cpu.py with -fsanitize=address,undefined. Prints "RANGESV OK <ranges>", exits 0. */
#include "../container/san_util.h"
#include "../container/stored_archive.h"

#include "rangesv_replay.h"

static int n_checked = 0;

static void run(uint32_t bs, uint64_t total, int checksum) {
    uint8_t* data = malloc(total);
    for (uint64_t i = 0; i < total; i++) data[i] = (uint8_t)(rnd() >> 5);
    rp_archive_t a;
    CHECK(rp_stored_archive(data, total, bs, checksum, 1, 0, 0u, &a));
    uint64_t* blk_at;
    int32_t* blk_status;
    rp_stored_decoded(&a, bs, checksum, &blk_at, &blk_status);
    const rvr_blocks_t blk = {data, blk_at, blk_status, a.nb};
    void* index = malloc(zr_index_size(a.nb));
    zr_open_serial(a.comp, a.size, bs, a.nb, index);
    CHECK(((const zr_index_t*)index)->status == ZXC_OK && ((const zr_index_t*)index)->nb == a.nb);

    enum { MAXR = 96 };
    uint64_t off[MAXR], len[MAXR];
    const uint64_t fixed[][2] = {{0, total}, {0, 1}, {total - 1, 1}, {0, 0}, {total, 0}, {total + 5, 0}, {total, 1}, {total - 1, 2},
                                 {bs - 3, 6}, {bs, bs}, {bs - 1, bs + 2}, {0, bs}, {0, bs + 31}, {0, bs + 32}, {0, bs + 33}, {16, bs + 48},
                                 {bs + 16, 2ull * bs + 100}, {5, 3ull * bs}, {2ull * bs, bs + 40}, {bs - 16, 2ull * bs + 64}, {0, 3ull * bs + 32}};
    uint64_t max_len;
    const uint32_t n = rvr_san_table(fixed, sizeof fixed / sizeof fixed[0], MAXR, total, bs, rnd, off, len, &max_len);

    for (uint32_t shift = 0; shift < 3u; shift++) {
        zxc_dev_rangev_t tab[MAXR];
        uint8_t* raw[MAXR];
        uint32_t k[MAXR];
        int64_t results[MAXR];
        for (uint32_t r = 0; r < n; r++) k[r] = (uint32_t)((off[r] + ((r & 1u) ? 1u + ((r >> 1) + 5u * shift) % 15u : 0u)) & 15u);
        rvr_san_pass(off, len, k, n, max_len, total, shift != 0, tab, raw);
        CHECK(rvr_call(a.size, index, tab, n, max_len, bs, 0, 0u, &blk, results) == ZXC_OK);
        for (uint32_t r = 0; r < n; r++) {
            const int64_t want = rvr_san_want(off, len, n, r, max_len, total);
            CHECK(results[r] == want);
            CHECK((raw[r] != NULL) == (want > 0));
            if (raw[r]) CHECK(memcmp(raw[r] + k[r], data + off[r], len[r]) == 0);
            free(raw[r]);
            n_checked++;
        }
    }
    free(index); free(blk_status); free(blk_at); rp_archive_free(&a); free(data);
}

int main(void) {
    rnd_state = 24680u;
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++) {
            const uint32_t bs = bss[b];
            const uint64_t totals[] = {1, bs - 1u, bs, bs + 1u, 3ull * bs + 5u, bs == 4096u ? 40ull * bs : 5ull * bs - 1u};
            for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(bs, totals[i], checksum);
        }
    /* a call of no ranges, and the shapes the entry point refuses */
    CHECK(rvr_call(1000u, NULL, NULL, 0u, 100u, 4096u, 0, 0u, NULL, NULL) == ZXC_OK);
    CHECK(rvr_call(1000u, NULL, NULL, 4u, 100u, 5000u, 0, 0u, NULL, NULL) == ZXC_ERROR_BAD_BLOCK_SIZE);
    CHECK(rvr_call(1000u, NULL, NULL, 1u << 20, 1ull << 30, 4096u, 0, 0u, NULL, NULL) == ZXC_ERROR_MEMORY);
    printf("RANGESV OK %d\n", n_checked);
    return 0;
}
