/* Stand-alone program (its own main, not loaded into anything) that replays sessions of zxc_amd/csrc/zxc_append.h the way the entry
 * points and kernels of zxc_append_device.hip run them (append_replay.h), over heap buffers of exactly the sizes a session is
 * promised, so that AddressSanitizer and UBSan see any read or write outside them. The encoder is a stand-in (every block a stored
 * block of the source's bytes, with a trailer when checksums are on); the archive it must give is built serially here with
 * zxc_container.h. Every combination of block size, checksum and seekable; sources of 0, 1, a block - 1, a block, a block + 1,
 * several blocks + 5 and 70 blocks (the hash rotation wraps); cuts at block boundaries, inside blocks, zero-length appends, many
 * sub-block appends in a row, random cuts, pieces shorter than the appends; a capacity of exactly the archive and one byte less.
 * Built by tests/test_compress_append_device_cpu.py with -fsanitize=address,undefined. Prints "APPEND OK <sessions>" and exits 0. */
#include <stdio.h>

#include "append_replay.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)
#define CANARY 0xC3u

static uint32_t rnd_state = 4321u;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static int sessions = 0;

/* one source: its stored blocks, the archive they make, and sessions over a set of cuts */
static void run(uint32_t bs, uint64_t total, int checksum, int seekable) {
    const uint32_t nb = (uint32_t)((total + bs - 1) / bs);
    uint8_t* src = malloc(total ? total : 1);
    for (uint64_t i = 0; i < total; i++) src[i] = (uint8_t)(rnd() >> 5);
    uint8_t* blocks = malloc((size_t)nb * (bs + 12u) + 1u);
    uint64_t* blk_at = malloc((nb + 1u) * 8u);
    uint32_t* blk_size = malloc((nb + 1u) * 4u);
    uint64_t at = 0;
    uint32_t hash = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t n = total - (uint64_t)b * bs < bs ? (uint32_t)(total - (uint64_t)b * bs) : bs;
        blk_at[b] = at;
        zc_st_le(blocks + at, zc_blk_hdr(0u, n), 8);
        memcpy(blocks + at + 8, src + (uint64_t)b * bs, n);
        if (checksum) {
            const uint32_t t = 0x9E3779B9u * (b + 1u) ^ src[(uint64_t)b * bs];
            zc_st_le(blocks + at + 8 + n, t, 4);
            hash = zc_hash_fold(hash, t);
        }
        blk_size[b] = 8u + n + (checksum ? 4u : 0u);
        at += blk_size[b];
    }
    /* the archive, serially */
    const uint64_t size = zc_known_size(nb, checksum, seekable) + total;
    uint8_t* want = malloc(size);
    zc_put_file_header(want, zc_block_size_lg(bs), checksum, 0, 0u);
    memcpy(want + ZC_FILE_HDR, blocks, at);
    uint64_t o = ZC_FILE_HDR + at;
    zc_st_le(want + o, zc_blk_hdr(ZC_BLK_EOF, 0u), 8); o += 8;
    if (seekable && nb) {
        zc_st_le(want + o, zc_blk_hdr(ZC_BLK_SEK, nb * 4u), 8); o += 8;
        for (uint32_t b = 0; b < nb; b++) { zc_st_le(want + o, blk_size[b], 4); o += 4; }
    }
    zc_put_footer(want + o, total, checksum ? hash : 0u);
    CHECK(o + ZC_FOOTER == size);

    uint64_t* lens = malloc((total / 111u + 64u) * 8u);
    for (int pattern = 0; pattern < 7; pattern++) {
        uint32_t n_lens = 0;
        uint64_t left = total, max_piece = total > bs ? total : bs;
        if (pattern == 0) lens[n_lens++] = total;
        else if (pattern == 1) { while (left) { const uint64_t n = left < bs ? left : bs; lens[n_lens++] = n; left -= n; } }
        else if (pattern == 2) { while (left) { const uint64_t n = left < 111u ? left : 111u; lens[n_lens++] = n; left -= n; } }
        else if (pattern == 3) { /* one byte in front of a boundary, one behind, zero-length appends between */
            if (left >= bs - 1u) { lens[n_lens++] = bs - 1u; left -= bs - 1u; }
            lens[n_lens++] = 0;
            if (left >= 2u) { lens[n_lens++] = 2u; left -= 2u; }
            lens[n_lens++] = 0;
            lens[n_lens++] = left;
            lens[n_lens++] = 0;
        } else if (pattern == 4) { lens[n_lens++] = total; max_piece = bs; }                 /* the piece loop, block by block */
        else if (pattern == 5) { lens[n_lens++] = total < 5u ? total : 5u; lens[n_lens++] = total - lens[0]; max_piece = 3ull * bs; }
        else { while (left) { uint64_t n = rnd() % (2u * bs + 7u); if (n > left) n = left; lens[n_lens++] = n; left -= n; } max_piece = 2ull * bs; }
        for (int short_by = 0; short_by < 2; short_by++) {
            const uint64_t cap = size - (uint64_t)short_by;
            uint8_t* dst = malloc(cap); /* exactly the capacity */
            memset(dst, CANARY, cap);
            const int64_t rc = rp_session(src, total, blocks, blk_at, blk_size, nb, bs, checksum, seekable, lens, n_lens, max_piece, dst, cap);
            if (short_by == 0) CHECK(rc == (int64_t)size && memcmp(dst, want, size) == 0);
            else CHECK(rc == ZXC_ERROR_DST_TOO_SMALL);
            free(dst);
            sessions++;
        }
    }
    free(lens); free(want); free(blk_size); free(blk_at); free(blocks); free(src);
}

int main(void) {
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++) {
                const uint32_t bs = bss[b];
                const uint64_t totals[] = {0, 1, bs - 1u, bs, bs + 1u, 3ull * bs + 5u, bs == 4096u ? 70ull * bs : 5ull * bs - 1u};
                for (unsigned i = 0; i < sizeof(totals) / sizeof(totals[0]); i++) run(bs, totals[i], checksum, seekable);
            }
    /* the promises of every plan near the block boundaries */
    for (uint32_t carry = 0; carry < 4096u; carry += 1u + carry / 64u)
        for (uint64_t n = 1; n < 3u * 4096u + 70u; n += (n % 4096u < 70u || n % 4096u > 4026u) ? 1u : 97u) CHECK(rp_plan_check(carry, n, 4096u) == 0);
    printf("APPEND OK %d\n", sessions);
    return 0;
}
