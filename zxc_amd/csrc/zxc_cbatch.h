/* zxc_cbatch.h — the rules of zxc_mi355x_compress_batch_device on top of zxc_container.h: the call's shape, an item's effective
 * capacity and source bounds, the plan of one item (its jobs for the job-table encode entries), and the finish of one item (size
 * check, archive size, block offsets, file header, EOF block, seek table, footer with the global hash). Plain inline C that hipcc
 * and a host C compiler both take, so that the kernels of zxc_cbatch_device.hip and the CPU tests run the same lines. An item's
 * archive is the one zxc_compress (zxc_host.c) and zxc_mi355x_compress_device write for the same bytes and options.
 *
 * Work area, from its 256-byte aligned base: a record per item, then per job a zxc_enc_job_t, a size, an archive offset and a
 * slot of zxc_mi355x_encode_slot_stride(block_size) bytes; with a dictionary the image area of one chunk behind them. In closed
 * form, with n_jobs = n_items x J and S = the slot stride, the size is at most
 *     n_jobs x (S + 28) + 64 x n_items + 1536                                     (ZCB_JOB_BYTES, ZCB_REC_BYTES, ZCB_WORK_FIXED)
 * and with a dictionary of D bytes at most that + min(n_jobs, C) x (block_size + D) + 320, C = zc_image_chunk(block_size, D).
 *
 * The finish of an item loops over its blocks serially (one thread per item): this call is for many items of few blocks each; one
 * source of many blocks belongs in zxc_mi355x_compress_device, whose passes are tiled. */
#ifndef ZXC_CBATCH_H
#define ZXC_CBATCH_H
#include "zxc_container.h"
#include "zxc_dev.h" /* zxc_enc_job_t */

#define ZCB_REC_BYTES 64u    /* work area per item: zcb_rec_t */
#define ZCB_JOB_BYTES 28u    /* work area per job besides its slot: zxc_enc_job_t, size, archive offset */
#define ZCB_WORK_FIXED 1536u /* work area besides items and jobs: alignment of the five parts and of the caller's pointer */
#define ZCB_IMAGE_FIXED 320u /* ... and of the image area, with its ZC_IMAGE_PAD */

/* Per-item state between the passes. */
typedef struct zcb_rec {
    int64_t result;   /* plan: 0, or the error that refuses the item; finish: the archive size, or the error */
    uint64_t dst_off;
    uint64_t cap;     /* the item's effective capacity */
    uint64_t src_size;
    uint32_t nb;      /* its blocks = the jobs it fills (0 for a refused item) */
    uint32_t rsv0;
    uint64_t rsv[3];
} zcb_rec_t;

/* ---- the call's shape, known to the host before any byte of the item table */
typedef struct zcb_shape {
    uint32_t J, n_jobs, slot_stride, chunk_jobs; /* jobs per item; n_items J; bytes per slot; jobs per image chunk (0: no dictionary) */
    uint64_t o_rec, o_jobs, o_sizes, o_offsets, o_slots, o_images, bytes; /* work-area offsets from its 256-byte aligned base */
} zcb_shape_t;
/* -> 0, ZXC_ERROR_BAD_BLOCK_SIZE, or ZXC_ERROR_MEMORY (more jobs than a launch counts). J = max(1, ceil(max_size / bs)): an item
 * of src_size <= max_size has at most that many blocks (an empty item has none and leaves its one job unused). slot_stride is
 * zxc_mi355x_encode_slot_stride(block_size); dict_size 0: the call without a dictionary. */
ZC_FN int zcb_shape(uint32_t n_items, uint64_t max_size, uint32_t block_size, uint32_t slot_stride, uint32_t dict_size, zcb_shape_t* s) {
    if (!zc_block_size_ok(block_size)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    uint64_t J = max_size / block_size + (max_size % block_size != 0);
    if (J == 0) J = 1;
    if (n_items && (J > 0x7FFFFFFEull || J * n_items > 0x7FFFFFFEull)) return ZXC_ERROR_MEMORY;
    if (J > 0x7FFFFFFEull) J = 0x7FFFFFFEull; /* (no item: nothing is sized by it) */
    s->J = (uint32_t)J;
    s->n_jobs = (uint32_t)(J * n_items);
    s->slot_stride = slot_stride;
    const uint64_t chunk = zc_image_chunk(block_size, dict_size);
    s->chunk_jobs = dict_size ? (uint32_t)(s->n_jobs < chunk ? s->n_jobs : chunk) : 0u;
    uint64_t o = 0;
    s->o_rec = o;     o = zc_round_up(o + (uint64_t)n_items * sizeof(zcb_rec_t), 256u);
    s->o_jobs = o;    o = zc_round_up(o + (uint64_t)s->n_jobs * sizeof(zxc_enc_job_t), 256u);
    s->o_sizes = o;   o = zc_round_up(o + 4ull * s->n_jobs, 256u);
    s->o_offsets = o; o = zc_round_up(o + 8ull * s->n_jobs, 256u);
    s->o_slots = o;   o = zc_round_up(o + (uint64_t)s->n_jobs * slot_stride, 256u);
    s->o_images = o;
    if (s->chunk_jobs) o = zc_round_up(o + (uint64_t)s->chunk_jobs * ((uint64_t)block_size + dict_size) + ZC_IMAGE_PAD, 256u);
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}

/* ---- an item. Its effective capacity: what the item allows and what d_dst holds behind dst_off. */
ZC_FN uint64_t zcb_cap(zxc_dev_item_t it, uint64_t dst_capacity) {
    if (it.dst_off > dst_capacity) return 0;
    const uint64_t room = dst_capacity - it.dst_off;
    return it.dst_capacity < room ? it.dst_capacity : room;
}
/* the item's bytes lie inside d_src[0, src_capacity), compared without overflow */
ZC_FN int zcb_src_ok(zxc_dev_item_t it, uint64_t src_capacity) {
    return it.src_off <= src_capacity && it.src_size <= src_capacity - it.src_off;
}

/* ---- plan: item r of the table. In this order: the effective capacity; the source bounds (ZXC_ERROR_SRC_TOO_SMALL); the promise
 * src_size <= max_size (ZXC_ERROR_OVERFLOW: the item has more blocks than its J jobs); the capacity against the part of the archive
 * known before encoding (ZXC_ERROR_DST_TOO_SMALL, as zxc_mi355x_compress_device answers synchronously); else job b of the item's
 * J (jobs[r J + b]) is block b: its offset in d_src and its byte count, of which only the last may be short. The entries behind
 * the item's blocks, and all J of a refused item, are left as they are (the caller zeroed them: len 0 is an unused job). */
ZC_FN void zcb_plan_item(zxc_dev_item_t it, uint32_t r, uint32_t J, uint64_t src_capacity, uint64_t max_size, uint64_t dst_capacity,
                         uint32_t block_size, int checksum, int seekable, zcb_rec_t* rec, zxc_enc_job_t* jobs) {
    rec->dst_off = it.dst_off; rec->cap = zcb_cap(it, dst_capacity); rec->src_size = it.src_size; rec->nb = 0; rec->rsv0 = 0;
    rec->rsv[0] = rec->rsv[1] = rec->rsv[2] = 0;
    if (!zcb_src_ok(it, src_capacity)) { rec->result = ZXC_ERROR_SRC_TOO_SMALL; return; }
    if (it.src_size > max_size) { rec->result = ZXC_ERROR_OVERFLOW; return; }
    const uint64_t nb = it.src_size / block_size + (it.src_size % block_size != 0); /* <= J */
    if (rec->cap < zc_known_size(nb, checksum, seekable)) { rec->result = ZXC_ERROR_DST_TOO_SMALL; return; }
    rec->result = 0;
    rec->nb = (uint32_t)nb;
    zxc_enc_job_t* tab = jobs + (uint64_t)r * J;
    for (uint32_t b = 0; b < rec->nb; b++) {
        const uint64_t at = (uint64_t)b * block_size, left = it.src_size - at;
        tab[b].src_off = it.src_off + at;
        tab[b].len = left < block_size ? (uint32_t)left : block_size;
        tab[b].pad = 0;
    }
}

/* ---- images (dictionary call): the jobs are encoded in chunks [c0, c0 + zcb_chunk_len), c0 a multiple of chunk_jobs; a chunk's
 * images are made in the one image area, which holds chunk_jobs of them, and consumed before the next chunk's, in stream order */
ZC_FN uint32_t zcb_chunk_len(const zcb_shape_t* s, uint32_t c0) { return s->n_jobs - c0 < s->chunk_jobs ? s->n_jobs - c0 : s->chunk_jobs; }

/* ---- finish: the item's archive around its blocks, from the nb sizes the encoder left (sizes, offsets, slots: the item's first
 * job's). A size outside [8 (+4), block_size + 64] is ZXC_ERROR_CORRUPT_DATA (the check of comp_sink, zxc_host.c; such a size is
 * never used as a length or to find a trailer); an archive larger than the capacity is ZXC_ERROR_DST_TOO_SMALL, and nothing of the
 * item is written. Else offsets[b] = block b's offset in the archive, and the file header (with a dictionary: its flag and id), the
 * EOF block, with `seekable` and nb > 0 the SEK header and entries, and the footer are written at dst + dst_off: the footer's
 * global hash is rotl(h, 1) ^ t_b folded from 0 over the trailers in order, which is what zxc_frame_tiles_kernel computes in
 * parallel as XOR_b rotl(t_b, (nb - 1 - b) mod 32). rec->result becomes the archive size; the blocks themselves are the gather's.
 * zcb_archive_size is its first half, the size check and the archive size, and writes nothing (zxc_cpack.h sizes every item with
 * it before it knows where one goes): -> the size of the archive around nb blocks of these sizes, or 0 when one of them is outside
 * the legal range; *eof_at = where its EOF block lies, *seek_bytes = its seek table's bytes (0: none). */
ZC_FN uint64_t zcb_archive_size(uint32_t nb, const uint32_t* sizes, uint32_t block_size, int checksum, int seekable, uint64_t* eof_at,
                                uint64_t* seek_bytes) {
    const uint32_t min_size = ZC_BLK_HDR + (checksum ? 4u : 0u), max_size = block_size + 64u;
    uint64_t sum = 0;
    for (uint32_t b = 0; b < nb; b++) {
        if (sizes[b] < min_size || sizes[b] > max_size) return 0;
        sum += sizes[b];
    }
    *eof_at = ZC_FILE_HDR + sum;
    *seek_bytes = (seekable && nb) ? ZC_BLK_HDR + 4ull * nb : 0ull;
    return *eof_at + ZC_BLK_HDR + *seek_bytes + ZC_FOOTER;
}
ZC_FN void zcb_finish_item(zcb_rec_t* rec, const uint32_t* sizes, uint64_t* offsets, const uint8_t* slots, uint32_t slot_stride,
                           uint8_t* dst, uint32_t block_size, int checksum, int seekable, int has_dict, uint32_t dict_id) {
    if (rec->result < 0) return;
    const uint32_t nb = rec->nb;
    uint64_t eof_at = 0, seek_bytes = 0;
    const uint64_t size = zcb_archive_size(nb, sizes, block_size, checksum, seekable, &eof_at, &seek_bytes);
    if (size == 0) { rec->result = ZXC_ERROR_CORRUPT_DATA; return; }
    if (size > rec->cap) { rec->result = ZXC_ERROR_DST_TOO_SMALL; return; }
    uint8_t* arc = dst + rec->dst_off;
    uint8_t* seek = arc + eof_at + 2u * ZC_BLK_HDR;
    uint64_t off = ZC_FILE_HDR;
    uint32_t hash = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t sz = sizes[b];
        offsets[b] = off;
        if (checksum) hash = zc_hash_fold(hash, zc_rd32(slots + (uint64_t)b * slot_stride + sz - 4u));
        if (seek_bytes) zc_st_le(seek + 4ull * b, sz, 4);
        off += sz;
    }
    zc_put_file_header(arc, zc_block_size_lg(block_size), checksum, has_dict, dict_id);
    zc_st_le(arc + eof_at, zc_blk_hdr(ZC_BLK_EOF, 0u), 8);
    if (seek_bytes) zc_st_le(arc + eof_at + ZC_BLK_HDR, zc_blk_hdr(ZC_BLK_SEK, nb * 4u), 8);
    zc_put_footer(arc + size - ZC_FOOTER, rec->src_size, checksum ? hash : 0u);
    rec->result = (int64_t)size;
}

/* block b of the item goes from its slot to dst + dst_off + offsets[b]: only for an item that succeeded */
ZC_FN int zcb_gathers(const zcb_rec_t* rec, uint32_t b) { return rec->result >= 0 && b < rec->nb; }
#endif
