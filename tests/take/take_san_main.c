/* Stand-alone program (its own main, not loaded into anything) that replays sessions of zxc_amd/csrc/zxc_take.h the way the entry
 * points and kernels of zxc_take_device.hip run them (take_replay.h), over heap buffers of exactly the sizes a session is promised,
 * so that AddressSanitizer and UBSan see any read or write outside them. The archives are tests/container/stored_archive.h's (every
 * block a stored block, with a trailer when checksums are on) and parsed by the real container stages; the decoder is the replay's
 * stand-in, which scribbles 32 bytes behind every block. Every combination of block size, checksum, seek table and verification;
 * sizes of 0, 1, a block - 1, a block, a block + 1, several blocks + 5 and 70 blocks; takes at block boundaries, inside blocks,
 * zero-length takes, many takes inside one block, random cuts, chunks shorter than the takes; pieces at aligned and odd addresses;
 * a capacity of exactly the size, one byte less and a block and 3 bytes more.
 * Built by tests/test_decompress_take_device_cpu.py with -fsanitize=address,undefined. Prints "TAKE OK <sessions>" and exits 0. */
#include "../container/san_util.h"
#include "../container/stored_archive.h"

#include "take_replay.h"

static int sessions = 0;

/* one session over pieces that are heap buffers of exactly n bytes (malloc aligns them to 16) or, odd, of 1 + n bytes */
static int64_t session_exact(const uint8_t* arc, uint64_t size, uint64_t cap, uint64_t max_piece, uint32_t bs, int verify, int use_table,
                             const uint8_t* data, const uint64_t* blk_at, const int32_t* blk_status, uint32_t nb, const uint64_t* lens,
                             uint32_t n_lens, int odd, uint8_t* out) {
    tr_session_t s;
    memset(&s, 0, sizeof s);
    s.blk_bytes = data; s.blk_at = blk_at; s.blk_status = blk_status; s.n_blocks = nb;
    CHECK(tr_begin(&s, arc, size, cap, max_piece, bs, verify, use_table, 0, 0u) == 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_lens; i++) {
        uint8_t* raw = malloc(lens[i] + (odd ? 1u : 0u) + (lens[i] + (odd ? 1u : 0u) == 0 ? 1u : 0u));
        uint8_t* d = raw + (odd ? 1 : 0);
        CHECK(tr_take(&s, d, lens[i]) == ZXC_OK);
        memcpy(out + at, d, lens[i]);
        at += lens[i];
        free(raw);
    }
    CHECK(at == cap && tr_take(&s, out, 1) == ZXC_ERROR_OVERFLOW);
    const int64_t r = tr_end(&s);
    tr_free(&s);
    sessions++;
    return r;
}

static void run(uint32_t bs, uint64_t total, int checksum, int seekable) {
    uint8_t* data = malloc(total ? total : 1);
    for (uint64_t i = 0; i < total; i++) data[i] = (uint8_t)(rnd() >> 5);
    rp_archive_t a;
    CHECK(rp_stored_archive(data, total, bs, checksum, seekable, 0, 0u, &a));
    const uint8_t* arc = a.comp;
    const uint64_t size = a.size;
    const uint32_t nb = a.nb;
    uint64_t* blk_at;
    int32_t* blk_status;
    rp_stored_decoded(&a, bs, checksum, &blk_at, &blk_status);

    const uint64_t caps[3] = {total, total ? total - 1u : 0u, total + bs + 3u};
    uint64_t* lens = malloc(((total + bs + 3u) / 111u + 64u) * 8u);
    uint8_t* out = malloc(total + bs + 4u);
    for (int ci = 0; ci < 3; ci++) {
        const uint64_t cap = caps[ci];
        const int64_t want = cap >= total ? (int64_t)total : (int64_t)ZXC_ERROR_DST_TOO_SMALL;
        for (int pattern = 0; pattern < 7; pattern++) {
            uint32_t n_lens = 0;
            uint64_t left = cap, max_piece = cap > bs ? cap : bs;
            if (pattern == 0) lens[n_lens++] = cap;
            else if (pattern == 1) { while (left) { const uint64_t n = left < bs ? left : bs; lens[n_lens++] = n; left -= n; } }
            else if (pattern == 2) { while (left) { const uint64_t n = left < 111u ? left : 111u; lens[n_lens++] = n; left -= n; } }
            else if (pattern == 3) { /* one byte in front of a boundary, one behind, zero-length takes between */
                if (left >= bs - 1u) { lens[n_lens++] = bs - 1u; left -= bs - 1u; }
                lens[n_lens++] = 0;
                if (left >= 2u) { lens[n_lens++] = 2u; left -= 2u; }
                lens[n_lens++] = 0;
                lens[n_lens++] = left;
                lens[n_lens++] = 0;
            } else if (pattern == 4) { lens[n_lens++] = cap; max_piece = bs; }                 /* the chunk loop, block by block */
            else if (pattern == 5) { lens[n_lens++] = cap < 5u ? cap : 5u; lens[n_lens++] = cap - lens[0]; max_piece = 3ull * bs; }
            else { while (left) { uint64_t n = rnd() % (2u * bs + 7u); if (n > left) n = left; lens[n_lens++] = n; left -= n; } max_piece = 2ull * bs; }
            for (int odd = 0; odd < 2; odd++) {
                const int verify = (pattern + odd) & 1, use_table = (pattern >> 1) & 1;
                const int64_t rc = session_exact(arc, size, cap, max_piece, bs, verify, use_table, data, blk_at, blk_status, nb, lens, n_lens,
                                                 odd, out);
                CHECK(rc == want);
                if (rc >= 0) CHECK(memcmp(out, data, total) == 0);
            }
            if (pattern == 2 || pattern == 6) { /* ... and pieces with canaries around them, 8 and 15 bytes off an aligned address */
                const int64_t rc = tr_session(arc, size, cap, max_piece, bs, 1, 1, 0, 0u, data, blk_at, blk_status, nb, lens, n_lens,
                                              pattern == 2 ? 8u : 15u, out);
                CHECK(rc == want && (rc < 0 || memcmp(out, data, total) == 0));
                sessions++;
            }
        }
    }
    free(out); free(lens); free(blk_status); free(blk_at); rp_archive_free(&a); free(data);
}

int main(void) {
    rnd_state = 4321u;
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++) {
                const uint32_t bs = bss[b];
                const uint64_t totals[] = {0, 1, bs - 1u, bs, bs + 1u, 3ull * bs + 5u, bs == 4096u ? 70ull * bs : 5ull * bs - 1u};
                for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(bs, totals[i], checksum, seekable);
            }
    /* the promises of every plan near the block boundaries */
    for (uint32_t pos = 0; pos < 4096u; pos += 1u + pos / 64u)
        for (uint64_t n = 1; n < 3u * 4096u + 70u; n += (n % 4096u < 70u || n % 4096u > 4026u) ? 1u : 97u)
            for (uint32_t align = 0; align < 16u; align += 5u) CHECK(tr_plan_check(pos, n, n + (n & 63u), align, 4096u, n > 4096u ? n : 4096u) == 0);
    printf("TAKE OK %d\n", sessions);
    return 0;
}
