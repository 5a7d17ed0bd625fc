/* Stand-alone program (its own main, not loaded into anything) that runs the rules of zxc_amd/csrc/zxc_cbatch.h the way the kernels
 * of zxc_cbatch_device.hip do, over heap buffers of exactly the sizes the call is promised, so that AddressSanitizer and UBSan
 * see any read or write outside them: shape, plan, a stand-in for the encoder (every block a stored block of the source's
 * bytes, with a trailer when checksums are on), finish and gather, for every combination of block size, checksum, seekable and
 * dictionary flag, items of 0, 1, a block, a block + 1 and several blocks at odd offsets, and the refused items. Every archive is
 * walked back with zxc_container.h (file header, block chain, seek table, footer, global hash) and compared with its source.
 * Built by tests/test_compress_batch_device_cpu.py with -fsanitize=address,undefined. Prints "CBATCH OK <archives>" and exits 0. */
#include "../container/san_util.h"
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_cbatch.h"

#define CANARY 0xC3u

/* a stored block of n bytes in a slot: header, bytes, trailer (any word will do: the rules only fold it) -> its size */
static uint32_t fake_encode(uint8_t* slot, const uint8_t* in, uint32_t n, int checksum) {
    zc_st_le(slot, zc_blk_hdr(0u, n), 8);
    memcpy(slot + 8, in, n);
    if (checksum) zc_st_le(slot + 8 + n, 0x9E3779B9u * (n + 1u) ^ in[0], 4);
    return 8u + n + (checksum ? 4u : 0u);
}

static int run(uint32_t bs, int checksum, int seekable, int has_dict, uint32_t dict_id) {
    const uint64_t sizes_of[] = {0, 1, 31, bs - 1, bs, bs + 1, 2ull * bs, 3ull * bs + 5};
    const uint32_t n_good = sizeof(sizes_of) / sizeof(sizes_of[0]), n_items = n_good + 5u;
    const uint64_t max_size = 3ull * bs + 5;
    const uint32_t stride = 2u * bs + 512u;
    zcb_shape_t s;
    CHECK(zcb_shape(n_items, max_size, bs, stride, has_dict ? 1000u : 0u, &s) == 0);
    CHECK(s.J == 4 && s.n_jobs == 4 * n_items);
    if (has_dict) CHECK(s.chunk_jobs == s.n_jobs && zcb_chunk_len(&s, 0) == s.n_jobs);

    /* the source area: items at odd offsets, exactly src_capacity bytes on the heap */
    zxc_dev_item_t* items = calloc(n_items, sizeof(*items));
    uint64_t src_capacity = 0, dst_capacity = 0;
    for (uint32_t r = 0; r < n_good; r++) {
        src_capacity += 1u + rnd() % 7u;
        items[r].src_off = src_capacity;
        items[r].src_size = sizes_of[r];
        src_capacity += sizes_of[r];
        dst_capacity += 1u + rnd() % 30u;
        items[r].dst_off = dst_capacity;
        items[r].dst_capacity = zc_known_size((sizes_of[r] + bs - 1) / bs, checksum, seekable) + sizes_of[r]; /* stored blocks: exact */
        dst_capacity += items[r].dst_capacity;
    }
    const uint64_t big = zc_known_size(1, checksum, seekable) + 100u;
    /* refused: one byte short of what the blocks need; past the source; a wrapping offset; above max_size; behind the destination */
    items[n_good + 0] = (zxc_dev_item_t){items[3].src_off, items[3].src_size, dst_capacity + 3u, items[3].dst_capacity - 1u};
    dst_capacity += 3u + items[3].dst_capacity - 1u;
    items[n_good + 1] = (zxc_dev_item_t){src_capacity - 10u, 11u, dst_capacity, big};
    items[n_good + 2] = (zxc_dev_item_t){~0ull - 5u, 100u, dst_capacity, big};
    items[n_good + 3] = (zxc_dev_item_t){0u, max_size + 1u, dst_capacity, ~0ull};
    items[n_good + 4] = (zxc_dev_item_t){items[1].src_off, 1u, dst_capacity + 1u, big};
    uint8_t* src = malloc(src_capacity ? src_capacity : 1);
    for (uint64_t i = 0; i < src_capacity; i++) src[i] = (uint8_t)(rnd() >> 3);
    uint8_t* dst = malloc(dst_capacity ? dst_capacity : 1);
    memset(dst, CANARY, dst_capacity);

    zcb_rec_t* recs = malloc(n_items * sizeof(*recs));
    zxc_enc_job_t* jobs = calloc(s.n_jobs, sizeof(*jobs));
    uint32_t* sizes = calloc(s.n_jobs, 4);
    uint64_t* offsets = malloc(s.n_jobs * 8u);
    uint8_t* slots = malloc((size_t)s.n_jobs * stride);
    memset(recs, 0xEE, n_items * sizeof(*recs));
    memset(offsets, 0xEE, s.n_jobs * 8u);
    for (uint32_t r = 0; r < n_items; r++)
        zcb_plan_item(items[r], r, s.J, src_capacity, max_size, dst_capacity, bs, checksum, seekable, recs + r, jobs);
    for (uint32_t i = 0; i < s.n_jobs; i++) { /* the encode launch: one job each, unused ones skipped */
        if (jobs[i].len == 0) continue;
        CHECK(jobs[i].len <= bs && jobs[i].src_off <= src_capacity && jobs[i].len <= src_capacity - jobs[i].src_off);
        sizes[i] = fake_encode(slots + (size_t)i * stride, src + jobs[i].src_off, jobs[i].len, checksum);
    }
    for (uint32_t r = 0; r < n_items; r++)
        zcb_finish_item(recs + r, sizes + r * s.J, offsets + r * s.J, slots + (size_t)r * s.J * stride, stride, dst, bs, checksum, seekable,
                        has_dict, dict_id);
    for (uint32_t i = 0; i < s.n_jobs; i++) { /* the gather: one job each */
        const zcb_rec_t* rec = recs + i / s.J;
        if (zcb_gathers(rec, i % s.J)) memcpy(dst + rec->dst_off + offsets[i], slots + (size_t)i * stride, sizes[i]);
    }

    CHECK(recs[n_good + 0].result == ZXC_ERROR_DST_TOO_SMALL && recs[n_good + 1].result == ZXC_ERROR_SRC_TOO_SMALL);
    CHECK(recs[n_good + 2].result == ZXC_ERROR_SRC_TOO_SMALL && recs[n_good + 3].result == ZXC_ERROR_OVERFLOW);
    CHECK(recs[n_good + 4].result == ZXC_ERROR_DST_TOO_SMALL && recs[n_good + 4].cap == 0);
    uint8_t* mine = calloc(dst_capacity ? dst_capacity : 1, 1);
    for (uint32_t r = 0; r < n_good; r++) { /* walk every archive back */
        const uint64_t size = (uint64_t)recs[r].result;
        CHECK(recs[r].result > 0 && size == items[r].dst_capacity);
        const uint8_t* arc = dst + items[r].dst_off;
        memset(mine + items[r].dst_off, 1, size);
        uint32_t lg = 0, ck = 0, id = 0;
        CHECK(zc_file_header(arc, &lg, &ck, &id) == ZXC_OK && (1u << lg) == bs && ck == (uint32_t)checksum && id == (has_dict ? dict_id : 0u));
        zc_chain_t ch = {ZC_FILE_HDR, 0, 0, 0, 0};
        uint64_t total = 0, nb = 0;
        for (;;) {
            const uint64_t at = ch.ip;
            const uint32_t cs = zc_chain_next(arc, size, ck, ck, &ch);
            if (cs) {
                const uint32_t n = zc_blk_csz(zc_rd64(arc + at));
                CHECK(cs == 8u + n + 4u * ck && memcmp(arc + at + 8, src + items[r].src_off + total, n) == 0);
                total += n;
                nb++;
            }
            if (ch.done) break;
        }
        CHECK(ch.saw_eof && ch.tail_err == 0 && total == items[r].src_size && nb == (total + bs - 1) / bs);
        CHECK(zc_rd64(arc + size - ZC_FOOTER) == total && zc_rd32(arc + size - 4) == (ck ? ch.ghash : 0u));
        uint64_t eof_at = 0, eof = 0;
        if (seekable && nb) CHECK(zc_seek_tail(arc, size, nb, &eof_at, &eof) && eof_at == ch.ip);
        else CHECK(ch.ip + ZC_BLK_HDR + ZC_FOOTER == size);
    }
    for (uint64_t i = 0; i < dst_capacity; i++) CHECK(mine[i] || dst[i] == CANARY); /* nothing outside the archives */
    free(mine); free(slots); free(offsets); free(sizes); free(jobs); free(recs); free(dst); free(src); free(items);
    return (int)n_good;
}

int main(void) {
    rnd_state = 12345u;
    int archives = 0;
    const uint32_t bss[] = {4096u, 65536u};
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++)
                for (int has_dict = 0; has_dict < 2; has_dict++) archives += run(bss[b], checksum, seekable, has_dict, 0xA1B2C3D4u);
    /* a corrupt size and an archive one byte over its capacity write nothing */
    {
        const uint32_t bs = 4096, stride = 2u * bs + 512u;
        zxc_dev_item_t it = {0, 5000, 0, 6000};
        zcb_rec_t rec;
        zxc_enc_job_t jobs[2] = {{0, 0, 0}, {0, 0, 0}};
        uint32_t sizes[2] = {4096 + 8, 3};
        uint64_t offsets[2];
        uint8_t* slots = calloc(2, stride);
        uint8_t* dst = malloc(6000);
        memset(dst, CANARY, 6000);
        zcb_plan_item(it, 0, 2, 5000, 5000, 6000, bs, 0, 1, &rec, jobs);
        CHECK(rec.result == 0 && rec.nb == 2 && jobs[1].len == 904);
        zcb_finish_item(&rec, sizes, offsets, slots, stride, dst, bs, 0, 1, 0, 0);
        CHECK(rec.result == ZXC_ERROR_CORRUPT_DATA && !zcb_gathers(&rec, 0));
        rec.result = 0;
        sizes[1] = 6000 - (16 + 8 + 8 + 8 + 12) - (4096 + 8) + 1;
        zcb_finish_item(&rec, sizes, offsets, slots, stride, dst, bs, 0, 1, 0, 0);
        CHECK(rec.result == ZXC_ERROR_DST_TOO_SMALL);
        for (int i = 0; i < 6000; i++) CHECK(dst[i] == CANARY);
        rec.result = 0;
        sizes[1]--;
        zcb_finish_item(&rec, sizes, offsets, slots, stride, dst, bs, 0, 1, 0, 0);
        CHECK(rec.result == 6000);
        free(dst); free(slots);
    }
    printf("CBATCH OK %d\n", archives);
    return 0;
}
