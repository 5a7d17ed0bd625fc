/* zxc_cpack.h — the rules of zxc_mi355x_compress_pack_device on top of zxc_cbatch.h: the batch call whose archives lie back to
 * back. The caller gives no destination per item; every item that can be given a size (a "sized" item: its source lies inside
 * d_src, src_size <= max_size, the encoder left legal block sizes) is laid out in table order, each at the end of the sized item
 * in front of it rounded up to `align`, the first at 0. So the place of an item is the exclusive prefix sum of the extents
 * round_up(size, align) of the items in front of it (a place is a multiple of align, so place + round_up(size, align) is the next
 * place), and an item that is not sized has extent 0. The layout does not depend on dst_capacity: the capacity only decides which
 * items are written (place + size <= dst_capacity; places only grow, so these are a prefix of the sized items), and the end of the
 * last sized item, *d_total, is the capacity with which all are. Plain inline C that hipcc and a host C compiler both take, so
 * that the kernels of zxc_cpack_device.hip and the CPU tests run the same lines.
 *
 * No sum here can pass 2^64, so the adds are plain: a call has at most 2^31 - 2 jobs (zcb_shape) of at most 2 MiB + 64 bytes each,
 * below 2^53 in all; around its blocks an item has 44 bytes of container and 4 per block of seek table, and less than 4096 of
 * padding, below 2^45 for 2^31 items and jobs. (The scan the kernels share with appendv saturates; here it never does.)
 *
 * Work area: zxc_cbatch.h's, and behind it one 64-bit sum per tile of ZC_TILE_BLOCKS = 1024 items and the word that collects the
 * end of the last sized item; everything else the passes hand on fits the record's reserved words (ZCP_SRC_OFF, ZCP_SIZE). In
 * closed form at most zxc_cbatch.h's bound + 8 x ceil(n_items / 1024) + 256                       (ZCP_TILE_BYTES, ZCP_WORK_FIXED) */
#ifndef ZXC_CPACK_H
#define ZXC_CPACK_H
#include "zxc_cbatch.h"

#define ZCP_TILE_BYTES 8u   /* work area per tile of 1024 items: the sum of its extents, then the place of its first item */
#define ZCP_WORK_FIXED 256u /* the end word and the alignment of the two */
#define ZCP_ALIGN_MAX 4096u
#define ZCP_SRC_OFF 0       /* rec->rsv[]: the item's src_off, for the packed table (which may overwrite the item table) */
#define ZCP_SIZE 1          /* rec->rsv[]: the archive size of a sized item */

/* ---- the call's shape: the sibling's, then the scan's words */
typedef struct zcp_shape {
    zcb_shape_t b;
    uint32_t n_tiles, rsv;
    uint64_t o_tiles, o_end, bytes; /* work-area offsets from its 256-byte aligned base */
} zcp_shape_t;
/* -> what zcb_shape answers for these arguments */
ZC_FN int zcp_shape(uint32_t n_items, uint64_t max_size, uint32_t block_size, uint32_t slot_stride, uint32_t dict_size, zcp_shape_t* s) {
    const int rc = zcb_shape(n_items, max_size, block_size, slot_stride, dict_size, &s->b);
    if (rc != 0) return rc;
    s->n_tiles = (uint32_t)(((uint64_t)n_items + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS);
    s->rsv = 0;
    s->o_tiles = s->b.bytes - 256u; /* (behind the sibling's last part, which ends on a multiple of 256) */
    s->o_end = s->o_tiles + (uint64_t)ZCP_TILE_BYTES * s->n_tiles;
    s->bytes = zc_round_up(s->o_end + 8u, 256u) + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}
ZC_FN int zcp_align_ok(uint32_t align) { return align >= 1u && align <= ZCP_ALIGN_MAX && (align & (align - 1u)) == 0; }

/* ---- plan: the sibling's (source bounds, max_size, the item's jobs) without a destination: the check of the known size passes
 * against a capacity of 2^64 - 1, and place and capacity come from the layout later. The record keeps src_off besides src_size. */
ZC_FN void zcp_plan_item(zxc_dev_item_t it, uint32_t r, uint32_t J, uint64_t src_capacity, uint64_t max_size, uint32_t block_size,
                         int checksum, int seekable, zcb_rec_t* rec, zxc_enc_job_t* jobs) {
    const uint64_t src_off = it.src_off;
    it.dst_off = 0;
    it.dst_capacity = ~0ull;
    zcb_plan_item(it, r, J, src_capacity, max_size, ~0ull, block_size, checksum, seekable, rec, jobs);
    rec->cap = 0;
    rec->rsv[ZCP_SRC_OFF] = src_off;
}

/* ---- size: behind the encoder. An item the plan refused stays as it is; illegal block sizes make it ZXC_ERROR_CORRUPT_DATA;
 * else it is sized and the record keeps its archive size. Nothing is written but the record. */
ZC_FN void zcp_size_item(zcb_rec_t* rec, const uint32_t* sizes, uint32_t block_size, int checksum, int seekable) {
    if (rec->result < 0) return;
    uint64_t eof_at = 0, seek_bytes = 0;
    const uint64_t size = zcb_archive_size(rec->nb, sizes, block_size, checksum, seekable, &eof_at, &seek_bytes);
    if (size == 0) { rec->result = ZXC_ERROR_CORRUPT_DATA; return; }
    rec->rsv[ZCP_SIZE] = size;
}
ZC_FN int zcp_sized(const zcb_rec_t* rec) { return rec->result >= 0; }
/* the room an item takes in the layout: its size rounded up to align (a power of two), or none */
ZC_FN uint64_t zcp_extent(const zcb_rec_t* rec, uint32_t align) {
    return zcp_sized(rec) ? zc_round_up(rec->rsv[ZCP_SIZE], align) : 0u;
}

/* ---- place: `at` = the extents of all items in front of this one added up. The record gets the place and what d_dst holds
 * behind it, which is what zcb_finish_item checks the archive against and writes at. -> the end of a sized item (0: not sized),
 * of which the largest, the last sized item's, is *d_total. */
ZC_FN uint64_t zcp_place_item(zcb_rec_t* rec, uint64_t at, uint64_t dst_capacity) {
    if (!zcp_sized(rec)) return 0;
    rec->dst_off = at;
    rec->cap = at <= dst_capacity ? dst_capacity - at : 0u;
    return at + rec->rsv[ZCP_SIZE];
}

/* ---- the packed table, behind the finish: the item of zxc_mi355x_decompress_batch_device that restores buffer r. An item that
 * was not written has src_size 0, which that call answers with ZXC_ERROR_SRC_TOO_SMALL without reading anything. */
ZC_FN zxc_dev_item_t zcp_packed_item(const zcb_rec_t* rec) {
    zxc_dev_item_t p;
    p.src_off = rec->result >= 0 ? rec->dst_off : 0u;
    p.src_size = rec->result >= 0 ? (uint64_t)rec->result : 0u;
    p.dst_off = rec->rsv[ZCP_SRC_OFF];
    p.dst_capacity = rec->src_size;
    return p;
}
#endif
