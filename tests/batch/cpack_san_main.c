/* Stand-alone program (its own main, not loaded into anything) that runs the stages of zxc_mi355x_compress_pack_device the way
 * the kernels of zxc_cbatch_device.hip group them (the loops of cpack_shim.c over the rules of zxc_amd/csrc/zxc_cpack.h), over
 * heap buffers of exactly the sizes the call is promised, so that AddressSanitizer and UBSan see any read or write outside
 * them: the destination has exactly min(dst_capacity, total) bytes, the scan exactly one word per tile. The encoder's stand-in
 * makes every block a stored block of the source's bytes (with a trailer when checksums are on), so an archive's size is known
 * without it and the layout is modelled here by a loop of its own. Cases: every combination of block size, checksum, seekable,
 * dictionary flag and align in (1, 16, 256, 4096) over items of 0 bytes to several blocks; 0, 1, 1023, 1024, 1025 and 2049 items
 * with items without a size at the tile edges; the capacity cut one byte short of every archive's end, at it, at 0 and at the
 * total; the packed table written over the item table. Every written archive is walked back with zxc_container.h and compared
 * with its source. Built by tests/test_compress_pack_device_cpu.py with -fsanitize=address,undefined. Prints "CPACK OK <archives>". */
#include "../container/san_util.h"
#include <stdlib.h>
#include <string.h>

#include "cpack_shim.c"

#define CANARY 0xC3u
#define WHOLE (~0ull) /* capacity: exactly the total */

/* a stored block of n bytes in a slot: header, bytes, trailer (any word will do: the rules only fold it) -> its size */
static uint32_t fake_encode(uint8_t* slot, const uint8_t* in, uint32_t n, int checksum) {
    zc_st_le(slot, zc_blk_hdr(0u, n), 8);
    memcpy(slot + 8, in, n);
    if (checksum) zc_st_le(slot + 8 + n, 0x9E3779B9u * (n + 1u) ^ in[0], 4);
    return 8u + n + (checksum ? 4u : 0u);
}

static void walk_back(const uint8_t* arc, uint64_t size, const uint8_t* src, uint64_t src_size, uint32_t bs, int checksum, int seekable,
                      int has_dict, uint32_t dict_id) {
    uint32_t lg = 0, ck = 0, id = 0;
    CHECK(zc_file_header(arc, &lg, &ck, &id) == ZXC_OK && (1u << lg) == bs && ck == (uint32_t)checksum && id == (has_dict ? dict_id : 0u));
    zc_chain_t ch = {ZC_FILE_HDR, 0, 0, 0, 0};
    uint64_t total = 0, nb = 0;
    for (;;) {
        const uint64_t at = ch.ip;
        const uint32_t cs = zc_chain_next(arc, size, ck, ck, &ch);
        if (cs) {
            const uint32_t n = zc_blk_csz(zc_rd64(arc + at));
            CHECK(cs == 8u + n + 4u * ck && memcmp(arc + at + 8, src + total, n) == 0);
            total += n;
            nb++;
        }
        if (ch.done) break;
    }
    CHECK(ch.saw_eof && ch.tail_err == 0 && total == src_size && nb == (total + bs - 1) / bs);
    CHECK(zc_rd64(arc + size - ZC_FOOTER) == total && zc_rd32(arc + size - 4) == (ck ? ch.ghash : 0u));
    uint64_t eof_at = 0, eof = 0;
    if (seekable && nb) CHECK(zc_seek_tail(arc, size, nb, &eof_at, &eof) && eof_at == ch.ip);
    else CHECK(ch.ip + ZC_BLK_HDR + ZC_FOOTER == size);
}

/* kinds of an item without a size */
enum { GOOD = 0, OOB, WRAP, BIG, CORRUPT };

/* one call. small: items of at most one block (J = 1), else up to 3 blocks + 5. dst_capacity WHOLE: the total. -> the total;
 * *written counts the archives written and checked */
static uint64_t run(uint32_t n, int small, uint32_t bs, int checksum, int seekable, int has_dict, uint32_t align, uint64_t dst_capacity,
                    int with_bad, int in_place, int* written) {
    const uint32_t dict_id = 0xA1B2C3D4u, stride = 2u * bs + 512u;
    const uint64_t many[] = {0, 1, 31, bs - 1, bs, bs + 1, 2ull * bs, 3ull * bs + 5}, few[] = {0, 1, 33, bs - 1, bs};
    const uint64_t max_size = small ? bs : 3ull * bs + 5;
    zcp_shape_t p;
    CHECK(zcp_shape(n, max_size, bs, stride, has_dict ? 1000u : 0u, &p) == 0);
    const zcb_shape_t* s = &p.b;
    CHECK(s->J == (small ? 1u : 4u) && s->n_jobs == s->J * n && p.n_tiles == (n + 1023u) / 1024u);

    zxc_dev_item_t* items = calloc(n ? n : 1, sizeof(*items));
    zxc_dev_item_t* given = calloc(n ? n : 1, sizeof(*items));
    uint8_t* kind = calloc(n ? n : 1, 1);
    uint64_t src_capacity = 0;
    for (uint32_t r = 0; r < n; r++) {
        src_capacity += 1u + rnd() % 7u;
        items[r].src_off = src_capacity;
        items[r].src_size = small ? few[(r * 3u + r / 1024u) % 5u] : many[r % 8u];
        items[r].dst_off = ~0ull - r; /* not looked at */
        items[r].dst_capacity = r;
        src_capacity += items[r].src_size;
    }
    src_capacity += max_size + 1u; /* (room for the item above max_size: its source lies inside, so that rule is the one it breaks) */
    if (with_bad) {
        const uint32_t edges[] = {0, 3, 4, 255, 256, 1019, 1020, 1022, 1023, 1024, 1025, 1027, 1028, 2047, 2048};
        for (uint32_t k = 0; k < sizeof(edges) / sizeof(edges[0]); k++) {
            const uint32_t r = edges[k];
            if (r >= n) continue;
            kind[r] = (uint8_t)(1u + k % 4u);
            if (kind[r] == CORRUPT && items[r].src_size == 0) kind[r] = BIG; /* (no block: no size to corrupt) */
            if (kind[r] == OOB) items[r].src_off = src_capacity - items[r].src_size + 1u;
            if (kind[r] == WRAP) { items[r].src_off = ~0ull - 3u; items[r].src_size = 100u; }
            if (kind[r] == BIG) items[r].src_size = max_size + 1u;
        }
    }
    memcpy(given, items, (n ? n : 1) * sizeof(*items));
    uint8_t* src = malloc(src_capacity ? src_capacity : 1);
    for (uint64_t i = 0; i < src_capacity; i++) src[i] = (uint8_t)(rnd() >> 3);

    /* the model: stored blocks make the archive size known */
    uint64_t* at = calloc(n ? n : 1, 8);
    uint64_t* size = calloc(n ? n : 1, 8);
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; r++) {
        if (kind[r]) continue;
        size[r] = zc_known_size((given[r].src_size + bs - 1) / bs, checksum, seekable) + given[r].src_size;
        at[r] = (total + align - 1u) / align * align;
        total = at[r] + size[r];
    }
    if (dst_capacity == WHOLE) dst_capacity = total;
    const uint64_t dst_bytes = dst_capacity < total ? dst_capacity : total;
    uint8_t* dst = dst_bytes ? malloc(dst_bytes) : NULL;
    if (dst) memset(dst, CANARY, dst_bytes);

    zcb_rec_t* recs = malloc((n ? n : 1) * sizeof(*recs));
    zxc_enc_job_t* jobs = calloc(s->n_jobs ? s->n_jobs : 1, sizeof(*jobs));
    uint32_t* sizes = calloc(s->n_jobs ? s->n_jobs : 1, 4);
    uint64_t* offsets = malloc((s->n_jobs ? s->n_jobs : 1) * 8u);
    uint8_t* slots = malloc((size_t)(s->n_jobs ? s->n_jobs : 1) * stride);
    uint64_t* tiles = malloc((p.n_tiles ? p.n_tiles : 1) * 8u);
    int64_t* results = malloc((n ? n : 1) * 8u);
    zxc_dev_item_t* packed = in_place ? items : malloc((n ? n : 1) * sizeof(*items));
    uint64_t end = 0xEEEE, d_total = 0xEEEE;
    memset(recs, 0xEE, (n ? n : 1) * sizeof(*recs));
    memset(offsets, 0xEE, (s->n_jobs ? s->n_jobs : 1) * 8u);

    t_pack_plan(items, n, s->J, src_capacity, max_size, bs, checksum, seekable, recs, jobs);
    for (uint32_t i = 0; i < s->n_jobs; i++) { /* the encode launch: one job each, unused ones skipped */
        if (jobs[i].len == 0) continue;
        CHECK(jobs[i].len <= bs && jobs[i].src_off <= src_capacity && jobs[i].len <= src_capacity - jobs[i].src_off);
        sizes[i] = fake_encode(slots + (size_t)i * stride, src + jobs[i].src_off, jobs[i].len, checksum);
    }
    for (uint32_t r = 0; r < n; r++)
        if (kind[r] == CORRUPT) sizes[(uint64_t)r * s->J + recs[r].nb - 1u] = bs + 65u;
    t_pack_layout(recs, n, s->J, sizes, bs, checksum, seekable, align, dst_capacity, tiles, &end);
    t_pack_finish(recs, n, s->J, sizes, offsets, slots, stride, dst, bs, checksum, seekable, has_dict, dict_id);
    t_pack_results(recs, n, &end, packed, results, &d_total);

    CHECK(d_total == (n ? total : 0xEEEE));
    uint8_t* mine = calloc(dst_bytes ? dst_bytes : 1, 1);
    int seen_short = 0;
    for (uint32_t r = 0; r < n; r++) {
        CHECK(packed[r].dst_off == given[r].src_off && packed[r].dst_capacity == given[r].src_size);
        if (kind[r]) {
            const int64_t want = kind[r] == BIG ? ZXC_ERROR_OVERFLOW : kind[r] == CORRUPT ? ZXC_ERROR_CORRUPT_DATA : ZXC_ERROR_SRC_TOO_SMALL;
            CHECK(results[r] == want && packed[r].src_off == 0 && packed[r].src_size == 0);
        } else if (at[r] + size[r] > dst_capacity) {
            seen_short = 1;
            CHECK(results[r] == ZXC_ERROR_DST_TOO_SMALL && packed[r].src_off == 0 && packed[r].src_size == 0);
        } else {
            CHECK(!seen_short); /* the items that fit are a prefix of the sized ones */
            CHECK(results[r] == (int64_t)size[r] && packed[r].src_off == at[r] && packed[r].src_size == size[r] && at[r] % align == 0);
            walk_back(dst + at[r], size[r], src + given[r].src_off, given[r].src_size, bs, checksum, seekable, has_dict, dict_id);
            memset(mine + at[r], 1, size[r]);
            (*written)++;
        }
    }
    for (uint64_t i = 0; i < dst_bytes; i++) CHECK(mine[i] || dst[i] == CANARY); /* the gaps, and whatever was not written */
    if (!in_place) free(packed);
    free(mine); free(results); free(tiles); free(slots); free(offsets); free(sizes); free(jobs); free(recs); free(dst); free(size); free(at);
    free(src); free(kind); free(given); free(items);
    return total;
}

int main(void) {
    rnd_state = 4321u;
    int archives = 0;
    const uint32_t bss[] = {4096u, 65536u}, aligns[] = {1u, 16u, 256u, 4096u}, counts[] = {0u, 1u, 1023u, 1024u, 1025u, 2049u};
    /* the rules over every kind of archive */
    for (int b = 0; b < 2; b++)
        for (int checksum = 0; checksum < 2; checksum++)
            for (int seekable = 0; seekable < 2; seekable++)
                for (int has_dict = 0; has_dict < 2; has_dict++)
                    for (int a = 0; a < 4; a++) run(16, 0, bss[b], checksum, seekable, has_dict, aligns[a], WHOLE, 0, 0, &archives);
    /* the scan's grouping, with and without items that take no room */
    for (int c = 0; c < 6; c++)
        for (int with_bad = 0; with_bad < 2; with_bad++) {
            run(counts[c], 1, 4096u, 1, 1, 0, 1u, WHOLE, with_bad, 0, &archives);
            run(counts[c], 1, 4096u, 0, 1, 0, 256u, WHOLE, with_bad, with_bad, &archives);
        }
    /* capacity cuts: the total does not move */
    for (int a = 0; a < 4; a += 2) {
        const uint64_t total = run(16, 0, 4096u, 1, 1, 0, aligns[a], WHOLE, 0, 0, &archives);
        uint64_t cuts[40];
        uint32_t n_cuts = 0;
        cuts[n_cuts++] = 0;
        cuts[n_cuts++] = total;
        cuts[n_cuts++] = total + 5;
        { /* every archive's end: found by asking for one byte less than the smallest capacity that writes one more */
            const uint64_t many[] = {0, 1, 31, 4095, 4096, 4097, 8192, 3 * 4096 + 5};
            uint64_t end = 0;
            for (uint32_t r = 0; r < 16; r++) {
                const uint64_t at = (end + aligns[a] - 1u) / aligns[a] * aligns[a];
                end = at + zc_known_size((many[r % 8] + 4095u) / 4096u, 1, 1) + many[r % 8];
                cuts[n_cuts++] = end - 1u;
                cuts[n_cuts++] = end;
            }
            CHECK(end == total);
        }
        for (uint32_t k = 0; k < n_cuts; k++) {
            CHECK(run(16, 0, 4096u, 1, 1, 0, aligns[a], cuts[k], 0, 0, &archives) == total);
            CHECK(run(16, 0, 4096u, 1, 1, 0, aligns[a], cuts[k], 0, 1, &archives) == total); /* ... and in place */
        }
    }
    /* in place, with items of every kind */
    for (int a = 0; a < 4; a++) run(1025, 1, 4096u, 1, 0, 1, aligns[a], WHOLE, 1, 1, &archives);
    printf("CPACK OK %d\n", archives);
    return 0;
}
