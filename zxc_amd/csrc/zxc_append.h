/* zxc_append.h — the rules of the append session (zxc_mi355x_compress_begin_device / _append_device / _end_device) on top of
 * zxc_container.h: the work area's shape, the plan of one piece (what is copied where, which job reads which bytes), the session's
 * running state and how a piece advances it, and the finish (file header, EOF block, seek table, footer). Plain inline C that hipcc
 * and a host C compiler both take, so that the kernels of zxc_append_device.hip and the CPU tests run the same lines. The archive
 * is the one zxc_compress (zxc_host.c) and zxc_mi355x_compress_device write for the concatenation of the appended bytes.
 *
 * A piece is at most max_piece bytes of one append. With `carry` bytes of an unfinished block waiting in the carry area, a piece
 * of n bytes completes nb = (carry + n) / block_size blocks and leaves tail = (carry + n) mod block_size bytes waiting. The host
 * knows carry and n, so the whole plan is the host's; the device only learns what the encoder made of the blocks.
 *
 * Work area, from its 256-byte aligned base: the state, three words per tile of 1024 jobs, per job a zxc_enc_job_t, a size, an
 * archive offset and a slot of S = zxc_mi355x_encode_slot_stride(block_size) bytes, three areas of block_size + 64 bytes (two carry
 * areas that take turns, one stage area), and with a seek table 4 bytes per block of max_total. In closed form, with
 * J = max_piece / block_size + 2 jobs and NB = ceil(max_total / block_size), the size is at most
 *     J x (S + 28) + 16 x ceil(J / 1024) + 3 x (block_size + 64) + 4 x NB (seekable only) + 4096
 *                                                                          (ZAP_JOB_BYTES, ZAP_TILE_BYTES, ZAP_AREAS, ZAP_WORK_FIXED)
 *
 * A session with a dictionary of D bytes (zxc_mi355x_compress_begin_dict_device) encodes every block from a [dict | block] image,
 * as zxc_mi355x_compress_dict_device does: the rules with `images` in their names. An image is a copy with padding behind it, so
 * nothing is staged and the head of a piece is not copied into the carry area first: the carried block's image takes its bytes
 * from two places. The image area lies behind the layout above: min(J, C) images of block_size + D bytes, C =
 * zc_image_chunk(block_size, D), which the chunks of a piece reuse in stream order, and ZC_IMAGE_PAD; the size is at most the
 * closed form above + min(J, C) x (block_size + D) + 320                                                    (ZAP_IMAGE_FIXED) */
#ifndef ZXC_APPEND_H
#define ZXC_APPEND_H
#include "zxc_container.h"
#include "zxc_dev.h" /* zxc_enc_job_t */

#define ZAP_OVERREAD 32u    /* the encoder reads up to 32 bytes past a block (include/zxc_mi355x.h) */
#define ZAP_PAD 64u         /* zero bytes behind whatever a copy leaves in an area (covers the over-read) */
#define ZAP_JOB_BYTES 28u   /* work area per job besides its slot: zxc_enc_job_t, size, archive offset */
#define ZAP_TILE_BYTES 16u  /* work area per tile: sum, hash, bad flag */
#define ZAP_AREAS 3u        /* areas of block_size + ZAP_PAD bytes: two carry areas, one stage area */
#define ZAP_WORK_FIXED 4096u /* the state, the alignment of the twelve parts and of the caller's pointer */
#define ZAP_IMAGE_FIXED 320u /* the dictionary session's image area: its ZC_IMAGE_PAD and its alignment */

/* where bytes lie: in the piece's source, or in one of the three areas */
enum { ZAP_SRC = 0, ZAP_CARRY = 1, ZAP_NEXT = 2, ZAP_STAGE = 3 };

/* ---- the session's shape, known to the host from the arguments of begin */
typedef struct zap_shape {
    uint32_t J, n_tiles, slot_stride, area; /* jobs of a piece; ceil(J / 1024); bytes per slot; bytes per carry / stage area */
    uint64_t nb_max;                        /* ceil(max_total / block_size) */
    uint64_t o_tile_sum, o_tile_hash, o_tile_bad, o_jobs, o_sizes, o_offsets, o_carry[2], o_stage, o_seek, o_slots, bytes;
} zap_shape_t;
/* -> 0, or ZXC_ERROR_BAD_BLOCK_SIZE: the block size, max_piece < block_size, more than 2^31 - 1 blocks in max_total, more jobs in
 * a piece than a launch counts. A piece of n <= max_piece bytes behind a carry < block_size completes at most
 * max_piece / block_size + 1 blocks; J keeps one more. slot_stride is zxc_mi355x_encode_slot_stride(block_size). */
ZC_FN int zap_shape(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable, zap_shape_t* s) {
    if (!zc_block_size_ok(block_size) || max_piece < block_size) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->nb_max = max_total / block_size + (max_total % block_size != 0);
    const uint64_t J = max_piece / block_size + 2u;
    if (s->nb_max > 0x7FFFFFFFull || J > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->J = (uint32_t)J;
    s->n_tiles = (s->J + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS;
    s->slot_stride = slot_stride;
    s->area = (uint32_t)zc_round_up((uint64_t)block_size + ZAP_PAD, 256u);
    uint64_t o = 256u; /* zap_ctl_t */
    s->o_tile_sum = o;  o = zc_round_up(o + 8ull * s->n_tiles, 256u);
    s->o_tile_hash = o; o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_tile_bad = o;  o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_jobs = o;      o = zc_round_up(o + J * sizeof(zxc_enc_job_t), 256u);
    s->o_sizes = o;     o = zc_round_up(o + 4ull * J, 256u);
    s->o_offsets = o;   o = zc_round_up(o + 8ull * J, 256u);
    s->o_carry[0] = o;  o += s->area;
    s->o_carry[1] = o;  o += s->area;
    s->o_stage = o;     o += s->area;
    s->o_seek = o;      o = zc_round_up(o + (seekable ? 4ull * s->nb_max : 0ull), 256u);
    s->o_slots = o;     o = zc_round_up(o + J * slot_stride, 256u);
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}
/* the closed form the header states */
ZC_FN uint64_t zap_work_bound(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable) {
    const uint64_t J = max_piece / block_size + 2u, nb = max_total / block_size + (max_total % block_size != 0);
    return J * ((uint64_t)slot_stride + ZAP_JOB_BYTES) + ZAP_TILE_BYTES * ((J + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS) +
           ZAP_AREAS * ((uint64_t)block_size + ZAP_PAD) + (seekable ? 4u * nb : 0u) + ZAP_WORK_FIXED;
}
/* The dictionary session's shape: the sibling's layout, and behind it the image area of chunk_jobs = min(J, C) images of
 * image = block_size + dict_size bytes with ZC_IMAGE_PAD behind the last. dict_size == 0: no image area, bytes is the sibling's.
 * -> 0, or what zap_shape answers. */
typedef struct zap_shape_images {
    zap_shape_t s;
    uint32_t chunk_jobs, image; /* jobs per encode launch (0 without a dictionary); bytes per image */
    uint64_t o_images, bytes;
} zap_shape_images_t;
ZC_FN int zap_shape_images(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable,
                           uint32_t dict_size, zap_shape_images_t* s) {
    const int rc = zap_shape(max_total, max_piece, block_size, slot_stride, seekable, &s->s);
    if (rc != 0) return rc;
    s->chunk_jobs = 0; s->image = block_size + dict_size; s->o_images = s->s.bytes - 256u; s->bytes = s->s.bytes;
    if (dict_size) {
        const uint64_t chunk = zc_image_chunk(block_size, dict_size);
        s->chunk_jobs = s->s.J < chunk ? s->s.J : (uint32_t)chunk;
        s->bytes = zc_round_up(s->o_images + (uint64_t)s->chunk_jobs * s->image + ZC_IMAGE_PAD, 256u) + 256u;
    }
    return 0;
}
/* ... and its closed form */
ZC_FN uint64_t zap_work_bound_images(uint64_t max_total, uint64_t max_piece, uint32_t block_size, uint32_t slot_stride, int seekable,
                                     uint32_t dict_size) {
    const uint64_t J = max_piece / block_size + 2u, chunk = zc_image_chunk(block_size, dict_size);
    return zap_work_bound(max_total, max_piece, block_size, slot_stride, seekable) +
           (dict_size ? (J < chunk ? J : chunk) * ((uint64_t)block_size + dict_size) + ZAP_IMAGE_FIXED : 0u);
}

/* ---- the plan of one piece */
/* area[at, at + len) = src[from, from + len), and ZAP_PAD zero bytes behind it. area == ZAP_SRC: no copy. */
typedef struct zap_copy {
    uint32_t area, at, len, rsv;
    uint64_t from;
} zap_copy_t;
typedef struct zap_piece {
    uint64_t n;        /* source bytes of the piece */
    uint64_t first;    /* source offset of the first block that lies whole in the source */
    uint32_t carry;    /* bytes waiting in the carry area in front of the piece (< block_size) */
    uint32_t nb;       /* blocks the piece encodes */
    uint32_t n_direct; /* of those that lie whole in the source, the leading ones are encoded where they lie ... */
    uint32_t n_staged; /* ... and the rest (at most one) from a zero-padded copy in the stage area */
    uint32_t tail;     /* bytes waiting behind the piece */
    uint32_t last_len; /* bytes of the last job: block_size, or the carry when `end` encodes it as the short last block */
    uint32_t swap;     /* the tail went to the other carry area: the two change roles behind this piece */
    uint32_t block_size;
    zap_copy_t cp[3];  /* the head of the source into the carry area, the staged block, the tail into the next carry area */
} zap_piece_t;

/* A piece of n > 0 bytes behind `carry` waiting bytes. No block completed: the bytes join the carry. Else the carried block takes
 * the first block_size - carry bytes; the blocks behind it lie in the source at first + i block_size, and block i is encoded there
 * while its over-read stays inside the piece, first + (i + 1) block_size + 32 <= n (as frame_plan's k_direct); at most one whole
 * block fails that and is staged, because the source ends less than 32 bytes behind it or the tail does. The tail goes to the
 * other carry area, which no job of this piece reads. Every source byte is copied once or read by one direct job. */
ZC_FN void zap_plan_piece(uint32_t carry, uint64_t n, uint32_t block_size, zap_piece_t* p) {
    const zap_copy_t none = {ZAP_SRC, 0u, 0u, 0u, 0u};
    const uint64_t total = carry + n;
    p->n = n; p->first = 0; p->carry = carry; p->nb = (uint32_t)(total / block_size); p->n_direct = 0; p->n_staged = 0;
    p->tail = (uint32_t)(total % block_size); p->last_len = block_size; p->swap = 0; p->block_size = block_size;
    p->cp[0] = p->cp[1] = p->cp[2] = none;
    if (p->nb == 0) {
        p->cp[0].area = ZAP_CARRY; p->cp[0].at = carry; p->cp[0].len = (uint32_t)n;
        return;
    }
    const uint32_t head = carry ? block_size - carry : 0u, whole = p->nb - (carry ? 1u : 0u);
    if (carry) { p->cp[0].area = ZAP_CARRY; p->cp[0].at = carry; p->cp[0].len = head; }
    const uint64_t room = n - head; /* >= whole x block_size */
    uint64_t direct = room >= ZAP_OVERREAD ? (room - ZAP_OVERREAD) / block_size : 0u;
    if (direct > whole) direct = whole;
    p->first = head;
    p->n_direct = (uint32_t)direct;
    p->n_staged = whole - p->n_direct; /* 0 or 1 */
    if (p->n_staged) { p->cp[1].area = ZAP_STAGE; p->cp[1].len = p->n_staged * block_size; p->cp[1].from = head + direct * block_size; }
    p->cp[2].area = ZAP_NEXT; p->cp[2].len = p->tail; p->cp[2].from = n - p->tail;
    p->swap = 1;
}
/* An append of `left` bytes behind `carry` waiting bytes: the bytes of its next piece. At most max_piece (>= block_size), and all
 * of them when they fit; else as many as end on a block boundary of the archive, so that only an append's last piece leaves a tail. */
ZC_FN uint64_t zap_piece_len(uint32_t carry, uint64_t left, uint64_t max_piece, uint32_t block_size) {
    return left <= max_piece ? left : (carry + max_piece) / block_size * block_size - carry;
}
/* `end`: what waits in the carry area is the archive's short last block (nothing waits: no block) */
ZC_FN void zap_plan_end(uint32_t carry, uint32_t block_size, zap_piece_t* p) {
    const zap_copy_t none = {ZAP_SRC, 0u, 0u, 0u, 0u};
    p->n = 0; p->first = 0; p->carry = carry; p->nb = carry ? 1u : 0u; p->n_direct = 0; p->n_staged = 0; p->tail = 0;
    p->last_len = carry; p->swap = 0; p->block_size = block_size;
    p->cp[0] = p->cp[1] = p->cp[2] = none;
}
/* job j < nb of the piece: where its bytes lie and how many they are */
typedef struct zap_src {
    uint32_t area, len;
    uint64_t off;
} zap_src_t;
ZC_FN zap_src_t zap_job(const zap_piece_t* p, uint32_t j) {
    zap_src_t r = {ZAP_CARRY, j + 1u == p->nb ? p->last_len : p->block_size, 0u};
    if (p->carry && j == 0) return r;
    const uint32_t i = j - (p->carry ? 1u : 0u);
    if (i < p->n_direct) { r.area = ZAP_SRC; r.off = p->first + (uint64_t)i * p->block_size; }
    else { r.area = ZAP_STAGE; r.off = (uint64_t)(i - p->n_direct) * p->block_size; }
    return r;
}

/* The same piece when every job is encoded from an image (the dictionary session). An image is a copy already, with padding
 * behind it for the encoder's over-read: every whole block is direct whatever lies behind it, nothing is staged, and the head of
 * the piece is not copied into the carry area, it is delivered to job 0's image straight from the source (zap_job_images). What
 * is left to copy is the tail, into the other carry area; a piece that completes no block joins the carry as above. nb, tail,
 * first and swap are zap_plan_piece's. Every source byte is read by one job segment or by the tail copy. The plan of `end` is
 * zap_plan_end. */
ZC_FN void zap_plan_piece_images(uint32_t carry, uint64_t n, uint32_t block_size, zap_piece_t* p) {
    const zap_copy_t none = {ZAP_SRC, 0u, 0u, 0u, 0u};
    zap_plan_piece(carry, n, block_size, p);
    if (p->nb == 0) return;
    p->n_direct = p->nb - (carry ? 1u : 0u);
    p->n_staged = 0;
    p->cp[0] = p->cp[1] = none;
}
/* job j < nb of such a piece: the one or two places its bytes lie, in order (seg[1].len == 0: one). The carried block is the
 * `carry` bytes waiting in the current carry area and then the first block_size - carry bytes of the piece; at `end` it is the
 * carry alone. */
typedef struct zap_src2 {
    zap_src_t seg[2];
} zap_src2_t;
ZC_FN zap_src2_t zap_job_images(const zap_piece_t* p, uint32_t j) {
    const uint32_t len = j + 1u == p->nb ? p->last_len : p->block_size;
    zap_src2_t r = {{{ZAP_SRC, len, 0u}, {ZAP_SRC, 0u, 0u}}};
    if (p->carry && j == 0) {
        r.seg[0].area = ZAP_CARRY; r.seg[0].len = p->carry;
        r.seg[1].len = len - p->carry;
        return r;
    }
    r.seg[0].off = p->first + (uint64_t)(j - (p->carry ? 1u : 0u)) * p->block_size;
    return r;
}

/* ---- the session's state in device memory */
typedef struct zap_ctl {
    int64_t status;   /* 0 while the archive fits, or the sticky negative zxc_error_t; behind `end` the archive size */
    uint64_t off;     /* archive offset behind the blocks gathered so far */
    uint64_t nb;      /* blocks so far */
    uint64_t first;   /* the current piece: the index of its first block (= its first seek-table entry) */
    uint64_t seek_at; /* `end`: offset of the first seek-table entry in the archive */
    uint32_t hash;    /* the global hash over the blocks so far */
    uint32_t rsv;
} zap_ctl_t;
ZC_FN void zap_begin(zap_ctl_t* c) {
    c->status = 0; c->off = ZC_FILE_HDR; c->nb = 0; c->first = 0; c->seek_at = 0; c->hash = 0; c->rsv = 0;
}
/* the size of the archive if it ended behind nb blocks that reach to `off`: EOF block, seek table, footer */
ZC_FN uint64_t zap_size_if_ended(uint64_t off, uint64_t nb, int seekable) {
    return off + ZC_BLK_HDR + ((seekable && nb) ? ZC_BLK_HDR + 4u * nb : 0u) + ZC_FOOTER;
}
ZC_FN int zap_size_ok(uint32_t sz, uint32_t block_size, int checksum) {
    return sz >= ZC_BLK_HDR + (checksum ? 4u : 0u) && sz <= block_size + 64u;
}
/* A piece's totals from the sizes the encoder left: the sum of the sizes, whether one lies outside [8 (+4), block_size + 64]
 * (such a size is never used as a length or to find a trailer), and the piece's hash XOR_b rotl(t_b, (nb - 1 - b) mod 32) over
 * the trailers. In series here (tests); zxc_frame_tiles_kernel computes the same per tile in parallel. */
ZC_FN void zap_piece_totals(const uint32_t* sizes, const uint8_t* slots, uint32_t slot_stride, uint32_t nb, uint32_t block_size,
                            int checksum, uint64_t* sum, uint32_t* hash, uint32_t* bad) {
    *sum = 0; *hash = 0; *bad = 0;
    for (uint32_t b = 0; b < nb; b++) {
        if (!zap_size_ok(sizes[b], block_size, checksum)) { *bad = 1u; continue; }
        *sum += sizes[b];
        if (checksum) *hash ^= zc_rotl(zc_rd32(slots + (uint64_t)b * slot_stride + sizes[b] - 4u), (nb - 1u - b) & 31u);
    }
}
/* A piece of nb_piece blocks with these totals joins the archive. A bad size is ZXC_ERROR_CORRUPT_DATA, whatever the status was
 * (the precedence of zxc_mi355x_compress_device). Once the blocks so far plus the tail the archive would need if it ended here
 * pass the capacity, the status is ZXC_ERROR_DST_TOO_SMALL: that size grows with every block, so this is the condition
 * size > dst_capacity of the finished archive. An error stays. -> 1 when the piece's blocks are to be gathered, block b at the
 * old c->off + the sizes in front of it, with seek-table entries c->first + b; then the hash is carried on: folding nb_piece more
 * trailers into h one at a time (zc_hash_fold) gives rotl(h, nb_piece mod 32) ^ piece_hash. */
ZC_FN int zap_advance(zap_ctl_t* c, uint32_t nb_piece, uint64_t sum, uint32_t piece_hash, uint32_t bad, uint64_t dst_capacity,
                      int checksum, int seekable) {
    if (bad) { c->status = ZXC_ERROR_CORRUPT_DATA; return 0; }
    if (c->status < 0) return 0;
    if (zap_size_if_ended(c->off + sum, c->nb + nb_piece, seekable) > dst_capacity) { c->status = ZXC_ERROR_DST_TOO_SMALL; return 0; }
    c->first = c->nb;
    c->nb += nb_piece;
    c->off += sum;
    if (checksum) c->hash = zc_rotl(c->hash, nb_piece & 31u) ^ piece_hash;
    return 1;
}

/* ---- finish: the archive around its blocks. total = the bytes appended. Writes the file header (with has_dict it carries the
 * dictionary flag and dict_id: the dictionary session), the EOF block, with `seekable` and blocks the SEK header, and the footer
 * with total and the global hash; the seek-table entries are zap_put_seek_entry's. c->status becomes the archive size. Nothing is
 * written for a session whose status is an error. */
ZC_FN void zap_finish_dict(zap_ctl_t* c, uint8_t* dst, uint64_t dst_capacity, uint64_t total, uint32_t block_size, int checksum,
                           int seekable, int has_dict, uint32_t dict_id) {
    if (c->status < 0) return;
    const uint64_t eof_at = c->off, size = zap_size_if_ended(c->off, c->nb, seekable);
    if (size > dst_capacity) { c->status = ZXC_ERROR_DST_TOO_SMALL; return; } /* (begin and every piece saw to that) */
    zc_put_file_header(dst, zc_block_size_lg(block_size), checksum, has_dict, dict_id);
    zc_st_le(dst + eof_at, zc_blk_hdr(ZC_BLK_EOF, 0u), 8);
    if (seekable && c->nb) zc_st_le(dst + eof_at + ZC_BLK_HDR, zc_blk_hdr(ZC_BLK_SEK, (uint32_t)c->nb * 4u), 8);
    c->seek_at = eof_at + 2u * ZC_BLK_HDR;
    zc_put_footer(dst + size - ZC_FOOTER, total, checksum ? c->hash : 0u);
    c->status = (int64_t)size;
}
/* ... of the session without a dictionary */
ZC_FN void zap_finish(zap_ctl_t* c, uint8_t* dst, uint64_t dst_capacity, uint64_t total, uint32_t block_size, int checksum, int seekable) {
    zap_finish_dict(c, dst, dst_capacity, total, block_size, checksum, seekable, 0, 0u);
}
/* entry b of the seek table: block b's size, from the array in the work area to its unaligned place in the archive */
ZC_FN void zap_put_seek_entry(const zap_ctl_t* c, uint8_t* dst, const uint32_t* seek, uint64_t b) {
    if (c->status >= 0 && b < c->nb) zc_st_le(dst + c->seek_at + 4u * b, seek[b], 4);
}
#endif
