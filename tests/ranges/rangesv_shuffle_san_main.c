/* Stand-alone program (its own main, not loaded into anything) that replays zxc_mi355x_decompress_rangesv_shuffle_device the way
 * the entry point and kernels of zxc_rangesv_shuffle_device.hip run it (rangesv_shuffle_replay.h), where every range's destination
 * is a heap buffer of exactly its length (plus k bytes in front for a base k mod 16) and the work area one of exactly its size, so
 * that AddressSanitizer and UBSan see any read or write outside either: a 16-byte plane load that passes a slot's bytes, a 16-byte
 * store of a group that passes a range's end, a single byte read behind a ragged block, a job that leaves the index. The archives
 * are tests/container/stored_archive.h's over the shuffle (by zsh_index, the definition) of seeded bytes, opened by the real open
 * passes; the decoder is the replay's stand-in, which scribbles 32 bytes behind every block. Element sizes 2, 4 and 8; block sizes
 * 4 KiB and 16 KiB, with and without checksums; sizes of 1, a block - 1, a block, a block + 1, and the two of the tests (nine
 * blocks + 1003; three blocks + 8589, whose ragged block spans a gather chunk's seam); a seeded table per archive: the fixed edge
 * ranges, random ranges, and the refused ones (empty, past the end, longer than max_len, a zero base, a wrapping base), at three
 * alignments each. One more pass per archive gives a middle block a status one below the block size and the last block one above
 * its length: the ranges that touch either get ZXC_ERROR_CORRUPT_DATA, the others stay exact.
 * Built by tests/test_decompress_rangesv_shuffle_device_cpu.py with -fsanitize=address,undefined.
 * Prints "RANGESV SHUFFLE OK <ranges>", exits 0. */
#include "../container/san_util.h"
#include "../container/stored_archive.h"

#include "rangesv_shuffle_replay.h"

static int n_checked = 0;

static void run(uint32_t E, uint32_t bs, uint64_t total, int checksum) {
    uint8_t *plain = malloc(total), *shuffled = malloc(total + 1u);
    for (uint64_t i = 0; i < total; i++) plain[i] = (uint8_t)(rnd() >> 5);
    for (uint64_t p = 0; p < total; p++) shuffled[zsh_index(p, total, E, bs)] = plain[p];
    shuffled[total] = 0;
    rp_archive_t a;
    CHECK(rp_stored_archive(shuffled, total, bs, checksum, 1, 0, 0u, &a));
    uint64_t* blk_at;
    int32_t* blk_status;
    rp_stored_decoded(&a, bs, checksum, &blk_at, &blk_status);
    const rvr_blocks_t blk = {shuffled, blk_at, blk_status, a.nb};
    void* index = malloc(zr_index_size(a.nb));
    zr_open_serial(a.comp, a.size, bs, a.nb, index);
    CHECK(((const zr_index_t*)index)->status == ZXC_OK && ((const zr_index_t*)index)->nb == a.nb);

    enum { MAXR = 64 };
    uint64_t off[MAXR], len[MAXR];
    const uint64_t fixed[][2] = {{0, total}, {0, 1}, {total - 1, 1}, {0, 0}, {total, 0}, {total + 5, 0}, {total, 1}, {total - 1, 2},
                                 {bs - 3, 6}, {bs, bs}, {bs - 1, bs + 2}, {0, bs}, {0, bs + 31}, {16, bs + 48}, {bs + 16, 2ull * bs + 100},
                                 {5, 3ull * bs}, {2ull * bs, bs + 40}, {bs - 16, 2ull * bs + 64}, {0, 3ull * bs + 32}, {8192 - 7, 14}};
    uint64_t max_len;
    const uint32_t n = rvr_san_table(fixed, sizeof fixed / sizeof fixed[0], MAXR, total, bs, rnd, off, len, &max_len);

    zr_shape_t s;
    CHECK(zrs_shape(n, max_len, bs, &s) == 0);
    const uint32_t mid = a.nb / 2u, last = a.nb - 1u;
    for (uint32_t pass = 0; pass < 4u; pass++) { /* three alignments, then the departure */
        const int broken = pass == 3u && a.nb >= 3u;
        if (pass == 3u && !broken) break;
        if (broken) { blk_status[mid] = (int32_t)bs - 1; blk_status[last] += 1; }
        zxc_dev_rangev_t tab[MAXR];
        uint8_t* raw[MAXR];
        uint32_t k[MAXR];
        int64_t results[MAXR];
        for (uint32_t r = 0; r < n; r++) k[r] = (r * 7u + 5u * pass) & 15u;
        rvr_san_pass(off, len, k, n, max_len, total, pass != 0, tab, raw);
        uint8_t* work = malloc(s.bytes);
        CHECK(rsr_call(a.size, index, tab, n, max_len, E, bs, 0, 0u, &blk, work, s.bytes, results) == ZXC_OK);
        free(work);
        for (uint32_t r = 0; r < n; r++) {
            int64_t want = rvr_san_want(off, len, n, r, max_len, total);
            CHECK((raw[r] != NULL) == (want > 0));
            if (broken && want > 0) {
                const uint64_t b0 = off[r] / bs, b1 = (off[r] + len[r] - 1u) / bs;
                if ((b0 <= mid && mid <= b1) || b1 == last) want = ZXC_ERROR_CORRUPT_DATA;
            }
            CHECK(results[r] == want);
            if (want > 0) CHECK(memcmp(raw[r] + k[r], plain + off[r], len[r]) == 0);
            free(raw[r]);
            n_checked++;
        }
    }
    free(index); free(blk_status); free(blk_at); rp_archive_free(&a); free(shuffled); free(plain);
}

int main(void) {
    rnd_state = 13579u;
    const uint32_t bss[] = {4096u, 16384u};
    for (uint32_t E = 2; E <= 8u; E *= 2u)
        for (int b = 0; b < 2; b++)
            for (int checksum = 0; checksum < 2; checksum++) {
                const uint32_t bs = bss[b];
                const uint64_t totals[] = {1, bs - 1u, bs, bs + 1u, bs == 4096u ? 9ull * bs + 1003u : 3ull * bs + 8589u};
                for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(E, bs, totals[i], checksum);
            }
    /* a call of no ranges, and the shapes and element sizes the entry point refuses */
    CHECK(rsr_call(1000u, NULL, NULL, 0u, 100u, 4u, 4096u, 0, 0u, NULL, NULL, 1u << 20, NULL) == ZXC_OK);
    CHECK(rsr_call(1000u, NULL, NULL, 4u, 100u, 3u, 5000u, 0, 0u, NULL, NULL, 1u << 20, NULL) == ZXC_ERROR_GPU_UNSUPPORTED);
    CHECK(rsr_call(1000u, NULL, NULL, 4u, 100u, 4u, 5000u, 0, 0u, NULL, NULL, 1u << 20, NULL) == ZXC_ERROR_BAD_BLOCK_SIZE);
    CHECK(rsr_call(1000u, NULL, NULL, 1u << 20, 1ull << 30, 4u, 4096u, 0, 0u, NULL, NULL, ~0ull, NULL) == ZXC_ERROR_MEMORY);
    CHECK(rsr_call(1000u, NULL, NULL, 4u, 100u, 4u, 4096u, 0, 0u, NULL, NULL, 100u, NULL) == ZXC_ERROR_MEMORY);
    printf("RANGESV SHUFFLE OK %d\n", n_checked);
    return 0;
}
