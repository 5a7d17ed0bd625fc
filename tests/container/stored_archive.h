/* Test-only: the one builder of an archive of stored blocks: every block a stored block of the source's bytes, with a trailer when
 * checksums are on, and the container around them (zxc_amd/csrc/zxc_container.h), built serially. It is the archive the stand-in
 * encoder of the append replays must give (tests/append/append_replay.h) and the one the take replays take apart (tests/take). */
#ifndef STORED_ARCHIVE_H
#define STORED_ARCHIVE_H
#include <stdlib.h>
#include <string.h>

#include "../../zxc_amd/csrc/zxc_container.h"

typedef struct rp_archive {
    uint8_t *blocks, *comp; /* the blocks back to back; the finished archive, `size` bytes */
    uint64_t *blk_at, size; /* where block b starts in `blocks` */
    uint32_t *blk_size, nb;
} rp_archive_t;
/* -> 1 when the archive came out at the size zc_known_size promises */
static inline int rp_stored_archive(const uint8_t* src, uint64_t total, uint32_t bs, int checksum, int seekable, int has_dict,
                                    uint32_t dict_id, rp_archive_t* a) {
    const uint32_t nb = a->nb = (uint32_t)((total + bs - 1) / bs);
    a->size = zc_known_size(nb, checksum, seekable) + total;
    a->comp = malloc(a->size);
    a->blocks = malloc((size_t)nb * (bs + 12u) + 1u);
    a->blk_at = malloc((nb + 1u) * 8u);
    a->blk_size = malloc((nb + 1u) * 4u);
    uint64_t at = 0;
    uint32_t hash = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t n = total - (uint64_t)b * bs < bs ? (uint32_t)(total - (uint64_t)b * bs) : bs;
        a->blk_at[b] = at;
        zc_st_le(a->blocks + at, zc_blk_hdr(0u, n), 8);
        memcpy(a->blocks + at + 8, src + (uint64_t)b * bs, n);
        if (checksum) {
            const uint32_t t = 0x9E3779B9u * (b + 1u) ^ src[(uint64_t)b * bs];
            zc_st_le(a->blocks + at + 8 + n, t, 4);
            hash = zc_hash_fold(hash, t);
        }
        a->blk_size[b] = 8u + n + (checksum ? 4u : 0u);
        at += a->blk_size[b];
    }
    zc_put_file_header(a->comp, zc_block_size_lg(bs), checksum, has_dict, dict_id);
    memcpy(a->comp + ZC_FILE_HDR, a->blocks, at);
    uint64_t o = ZC_FILE_HDR + at;
    zc_st_le(a->comp + o, zc_blk_hdr(ZC_BLK_EOF, 0u), 8); o += 8;
    if (seekable && nb) {
        zc_st_le(a->comp + o, zc_blk_hdr(ZC_BLK_SEK, nb * 4u), 8); o += 8;
        for (uint32_t b = 0; b < nb; b++) { zc_st_le(a->comp + o, a->blk_size[b], 4); o += 4; }
    }
    zc_put_footer(a->comp + o, total, checksum ? hash : 0u);
    return o + ZC_FOOTER == a->size;
}
static inline void rp_archive_free(rp_archive_t* a) { free(a->comp); free(a->blocks); free(a->blk_at); free(a->blk_size); }
/* What a decoder answers for such an archive, as the take replays' stand-in wants it: block b decodes to the source's bytes from
 * b x bs on, blk_status[b] of them. Two arrays of nb + 1 entries, the caller's to free. */
static inline void rp_stored_decoded(const rp_archive_t* a, uint32_t bs, int checksum, uint64_t** blk_at, int32_t** blk_status) {
    *blk_at = malloc((a->nb + 1u) * 8u);
    *blk_status = malloc((a->nb + 1u) * 4u);
    for (uint32_t b = 0; b < a->nb; b++) {
        (*blk_at)[b] = (uint64_t)b * bs;
        (*blk_status)[b] = (int32_t)(a->blk_size[b] - 8u - (checksum ? 4u : 0u));
    }
}
#endif
