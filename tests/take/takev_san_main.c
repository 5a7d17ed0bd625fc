/* Stand-alone program (its own main, not loaded into anything) that replays sessions mixing zxc_mi355x_decompress_take_device and
 * zxc_mi355x_decompress_takev_device the way the entry points and kernels of zxc_take_device.hip run them (takev_replay.h), where
 * every entry of a table is a heap buffer of exactly its length (an empty entry has base 0), so that AddressSanitizer and UBSan
 * see any read or write outside an entry: the decoders' spill behind a block decoded in its entry, a 16-byte store of the scatter
 * that passes an entry's end, a search that leaves the table. The archives are tests/container/stored_archive.h's (every block a
 * stored block, with a trailer when checksums are on) and parsed by the real container stages; the decoder is the replay's
 * stand-in, which scribbles 32 bytes behind every block. Every combination of block size, checksum, seek table and verification;
 * sizes of 0, 1, a block - 1, a block, a block + 1, several blocks + 5 and 40 blocks; tables of one entry, of entries around a
 * block and its spill, of tiny entries, of random entries with empty ones between; chunks shorter than the calls; entries at
 * aligned and odd addresses; a capacity of exactly the size, one byte less and a block and 3 bytes more.
 * Built by tests/test_decompress_takev_device_cpu.py with -fsanitize=address,undefined. Prints "TAKEV OK <sessions>", exits 0. */
#include "../container/san_util.h"
#include "../container/stored_archive.h"

#include "takev_replay.h"

static int sessions = 0;

/* one session: the entries lens[0 .. n_lens) in calls of per_call entries, every third call a take of its entries' sum */
static int64_t session_exact(const uint8_t* arc, uint64_t size, uint64_t cap, uint64_t max_piece, uint32_t bs, int verify, int use_table,
                             const uint8_t* data, const uint64_t* blk_at, const int32_t* blk_status, uint32_t nb, const uint64_t* lens,
                             uint32_t n_lens, uint32_t per_call, int odd, uint8_t* out) {
    tr_session_t s;
    memset(&s, 0, sizeof s);
    s.blk_bytes = data; s.blk_at = blk_at; s.blk_status = blk_status; s.n_blocks = nb;
    CHECK(tr_begin(&s, arc, size, cap, max_piece, bs, verify, use_table, 0, 0u) == 0);
    uint64_t at = 0;
    for (uint32_t e = 0, call = 0; e < n_lens; e += per_call, call++) {
        const uint32_t cnt = n_lens - e < per_call ? n_lens - e : per_call;
        uint64_t total = 0;
        for (uint32_t r = 0; r < cnt; r++) total += lens[e + r];
        if (call % 3u == 2u) {
            uint8_t* raw = malloc(total + (odd ? 1u : 0u) + (total + (odd ? 1u : 0u) == 0 ? 1u : 0u));
            CHECK(tr_take(&s, raw + (odd ? 1 : 0), total) == ZXC_OK);
            memcpy(out + at, raw + (odd ? 1 : 0), total);
            at += total;
            free(raw);
            continue;
        }
        zxc_dev_iov_t* iov = malloc(((size_t)cnt + 1u) * sizeof *iov);
        uint8_t** raw = malloc(((size_t)cnt + 1u) * sizeof *raw);
        for (uint32_t r = 0; r < cnt; r++) {
            const uint64_t n = lens[e + r];
            const int shift = odd && ((e + r) & 1u);
            raw[r] = n ? malloc(n + (shift ? 1u : 0u)) : NULL;
            iov[r].base = n ? (uint64_t)(uintptr_t)(raw[r] + (shift ? 1 : 0)) : 0u;
            iov[r].len = n;
        }
        CHECK(tvr_takev(&s, iov, cnt, total) == ZXC_OK);
        for (uint32_t r = 0; r < cnt; r++) {
            if (iov[r].len) memcpy(out + at, (const uint8_t*)(uintptr_t)iov[r].base, iov[r].len);
            at += iov[r].len;
            free(raw[r]);
        }
        free(raw); free(iov);
    }
    zxc_dev_iov_t one = {(uint64_t)(uintptr_t)out, 1u};
    CHECK(at == cap && tvr_takev(&s, &one, 1u, 1u) == ZXC_ERROR_OVERFLOW && tvr_takev(&s, NULL, 0u, 1u) == ZXC_ERROR_DST_TOO_SMALL);
    CHECK(tvr_takev(&s, NULL, 0u, 0u) == ZXC_OK);
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
    uint64_t* lens = malloc(((total + bs + 3u) / 3u + 64u) * 8u);
    uint8_t* out = malloc(total + bs + 4u);
    for (int ci = 0; ci < 3; ci++) {
        const uint64_t cap = caps[ci];
        const int64_t want = cap >= total ? (int64_t)total : (int64_t)ZXC_ERROR_DST_TOO_SMALL;
        for (int pattern = 0; pattern < 6; pattern++) {
            uint32_t n_lens = 0, per_call = 1u << 30;
            uint64_t left = cap, max_piece = cap > bs ? cap : bs;
            if (pattern == 0) lens[n_lens++] = cap; /* one entry: what a take does */
            else if (pattern == 1) { /* entries around a block and its spill, which move the cuts through every alignment */
                const uint64_t around[] = {bs, bs + 31u, bs + 32u, bs + 33u, 0u, 2ull * bs + 32u, 15u, bs + 48u, 1u};
                for (uint32_t i = 0; left; i++) { uint64_t n = around[i % 9u]; if (n > left) n = left; lens[n_lens++] = n; left -= n; }
                max_piece = 3ull * bs;
            } else if (pattern == 2) { /* tiny entries: every block through the scatter */
                if (cap > 40000u) { lens[n_lens++] = cap - 40000u; left = 40000u; }
                while (left) { uint64_t n = 1u + rnd() % 7u; if (n > left) n = left; lens[n_lens++] = n; left -= n; }
                per_call = 1500u;
            } else if (pattern == 3) { /* random entries with empty ones between, several calls, the chunk loop */
                while (left) { uint64_t n = (rnd() & 3u) ? rnd() % (2u * bs + 70u) : 0u; if (n > left) n = left; lens[n_lens++] = n; left -= n; }
                lens[n_lens++] = 0;
                per_call = 5u; max_piece = 2ull * bs;
            } else if (pattern == 4) { /* calls that lie wholly inside one block, and entries of 16 and 17 bytes */
                while (left) { uint64_t n = 16u + (n_lens & 1u); if (n_lens > 300u || n > left) n = left; lens[n_lens++] = n; left -= n; }
                per_call = 7u; max_piece = bs;
            } else { /* only empty entries in front of everything, then one */
                lens[n_lens++] = 0; lens[n_lens++] = 0; lens[n_lens++] = cap;
                per_call = 2u; max_piece = bs + 1u;
            }
            for (int odd = 0; odd < 2; odd++) {
                const int verify = (pattern + odd) & 1, use_table = (pattern >> 1) & 1;
                const int64_t rc = session_exact(arc, size, cap, max_piece, bs, verify, use_table, data, blk_at, blk_status, nb, lens, n_lens,
                                                 per_call, odd, out);
                CHECK(rc == want);
                if (rc >= 0) CHECK(memcmp(out, data, total) == 0);
            }
        }
    }
    free(out); free(lens); free(blk_status); free(blk_at); rp_archive_free(&a); free(data);
}

int main(void) {
    rnd_state = 8765u;
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++) {
                const uint32_t bs = bss[b];
                const uint64_t totals[] = {0, 1, bs - 1u, bs, bs + 1u, 3ull * bs + 5u, bs == 4096u ? 40ull * bs : 5ull * bs - 1u};
                for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(bs, totals[i], checksum, seekable);
            }
    /* the in-place rule against the plain walk, entries of every length around a block and its spill at bases 0 and 1 mod 16 */
    for (uint32_t k = 0; k < 64u; k++) {
        zxc_dev_iov_t iov[8];
        for (uint32_t r = 0; r < 8u; r++) {
            iov[r].len = 4096u + (rnd() % 3u) * 4096u + 29u + rnd() % 6u;
            iov[r].base = 0x100000ull * (r + 1u) + ((k + r) & 1u);
        }
        CHECK(tvr_rule_check(iov, 8u, rnd() % 4096u, 3u * 4096u, 4096u) == 0);
    }
    /* (take_replay.h's own check and session, kept referenced: the header's functions are static) */
    CHECK(tr_plan_check(5u, 100u, 100u, 0u, 4096u, 4096u) == 0);
    {
        uint8_t arc[ZC_FILE_HDR + ZC_BLK_HDR + ZC_FOOTER], out[1];
        const uint64_t blk_at[1] = {0}, none[1] = {0};
        const int32_t blk_status[1] = {0};
        zc_put_file_header(arc, zc_block_size_lg(4096u), 0, 0, 0u);
        zc_st_le(arc + ZC_FILE_HDR, zc_blk_hdr(ZC_BLK_EOF, 0u), 8);
        zc_put_footer(arc + ZC_FILE_HDR + ZC_BLK_HDR, 0u, 0u);
        CHECK(tr_session(arc, sizeof arc, 0u, 4096u, 4096u, 0, 0, 0, 0u, out, blk_at, blk_status, 0u, none, 0u, 0u, out) == 0);
        const uint32_t calls[1] = {1u};
        CHECK(tvr_session(arc, sizeof arc, 0u, 4096u, 4096u, 0, 0, 0, 0u, out, blk_at, blk_status, 0u, none, calls, 1u, 0u, out) == 0);
    }
    printf("TAKEV OK %d\n", sessions);
    return 0;
}
