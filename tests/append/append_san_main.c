/* Stand-alone program (its own main, not loaded into anything) that replays sessions of zxc_amd/csrc/zxc_append.h the way the entry
 * points and kernels of zxc_append_device.hip run them (append_replay.h), over heap buffers of exactly the sizes a session is
 * promised, so that AddressSanitizer and UBSan see any read or write outside them. The encoder is a stand-in (every block a stored
 * block of the source's bytes, with a trailer when checksums are on); the archive it must give is rp_stored_archive's. Every
 * combination of block size, checksum and seekable; sources of 0, 1, a block - 1, a block, a block + 1,
 * several blocks + 5 and 70 blocks (the hash rotation wraps); cuts at block boundaries, inside blocks, zero-length appends, many
 * sub-block appends in a row, random cuts, pieces shorter than the appends; a capacity of exactly the archive and one byte less.
 * Built by tests/test_compress_append_device_cpu.py with -fsanitize=address,undefined. Prints "APPEND OK <sessions>" and exits 0. */
#include "../container/san_util.h"

#include "append_replay.h"

#define CANARY 0xC3u

static int sessions = 0;

/* one source: its stored blocks and the archive they make (rp_stored_archive), and sessions over a set of cuts */
static void run(uint32_t bs, uint64_t total, int checksum, int seekable) {
    uint8_t* src = malloc(total ? total : 1);
    for (uint64_t i = 0; i < total; i++) src[i] = (uint8_t)(rnd() >> 5);
    rp_archive_t a;
    CHECK(rp_stored_archive(src, total, bs, checksum, seekable, 0, 0u, &a));
    const uint64_t size = a.size;

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
            const int64_t rc = rp_session(src, total, a.blocks, a.blk_at, a.blk_size, a.nb, bs, checksum, seekable, lens, n_lens, max_piece, dst, cap);
            if (short_by == 0) CHECK(rc == (int64_t)size && memcmp(dst, a.comp, size) == 0);
            else CHECK(rc == ZXC_ERROR_DST_TOO_SMALL);
            free(dst);
            sessions++;
        }
    }
    free(lens); rp_archive_free(&a); free(src);
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
    for (uint32_t carry = 0; carry < 4096u; carry += 1u + carry / 64u)
        for (uint64_t n = 1; n < 3u * 4096u + 70u; n += (n % 4096u < 70u || n % 4096u > 4026u) ? 1u : 97u) CHECK(rp_plan_check(carry, n, 4096u) == 0);
    printf("APPEND OK %d\n", sessions);
    return 0;
}
