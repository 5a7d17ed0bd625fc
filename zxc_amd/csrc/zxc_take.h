/* zxc_take.h — the rules of the take session (zxc_mi355x_decompress_begin_device / _take_device / _end_device) on top of
 * zxc_container.h: the work area's shape and its stated bound, the plan of one chunk of a take (which blocks are copied from the
 * carry slot, decoded straight into the piece, decoded into a slot and copied, or decoded into the next carry slot, and which
 * bytes each copy moves), and how the session's position and carry advance. Plain inline C that hipcc and a host C compiler both
 * take, so that the entry points and kernels of zxc_take_device.hip and the CPU tests run the same lines. The container itself
 * (head, seek table, walk, events, verdict) is zxc_container.h's, unchanged: the session decodes the archive as
 * zxc_mi355x_decompress_device does, into a destination it is handed in pieces.
 *
 * The host knows block_size, the position pos (the bytes taken so far) and every n, so it knows which block lands where. With
 * pos inside block pos / block_size, that block was decoded by the take that ended inside it and waits in a carry slot; a chunk
 * of n bytes copies its next `head` bytes from there, decodes the `whole` blocks that lie wholly inside the chunk, and decodes
 * the block it ends inside (`tail` bytes wanted) into the other carry slot. Every block is decoded once.
 *
 * Work area, from its 256-byte aligned base: what zc_shape keeps per block of dst_capacity (the state, three words per tile of
 * 1024 jobs, two job tables and two status tables of n_jobs = ceil(dst_capacity / block_size) + 1), then per chunk job its entry
 * in the two chunk tables and a slot of block_size + 64 bytes, and two carry slots. In closed form, with
 * J = max_piece / block_size + 2, the size is at most
 *     56 x n_jobs + 16 x ceil(n_jobs / 1024) + J x (block_size + 64 + 48) + 2 x (block_size + 64) + 4096
 *                                                (ZT_BLOCK_BYTES, ZT_TILE_BYTES, ZT_SLOT_PAD, ZT_JOB_BYTES, ZT_CARRIES, ZT_WORK_FIXED) */
#ifndef ZXC_TAKE_H
#define ZXC_TAKE_H
#include "zxc_container.h"

#define ZT_SLOT_PAD 64u      /* behind every slot: the decoders store up to 32 bytes past out_len, and slots stay 16-aligned */
#define ZT_SPILL 32u         /* ... which a block decoded straight into a piece must keep inside the piece */
#define ZT_COPY_CHUNK 8192u  /* destination bytes one wavefront of the copy-out moves */
#define ZT_BLOCK_BYTES 56u   /* work area per job of the capacity: two zxc_dev_job_t, two statuses (as zc_shape) */
#define ZT_TILE_BYTES 16u    /* work area per tile: sum, hash, bad flag (as zc_shape) */
#define ZT_JOB_BYTES 48u     /* work area per chunk job besides its slot: its entry in the two chunk tables */
#define ZT_CARRIES 2u        /* carry slots of block_size + ZT_SLOT_PAD bytes, which take turns */
#define ZT_WORK_FIXED 4096u  /* the state, the alignment of the ten parts and of the caller's pointer */

/* ---- the session's shape, known to the host from the arguments of begin */
typedef struct zt_shape {
    uint32_t n_jobs, n_tiles, J, slot_stride, copy_chunks, rsv; /* zc_shape's; jobs and slots of a chunk; bytes per slot; copy-out chunks per copy */
    uint64_t o_tile_sum, o_tile_hash, o_tile_bad, o_jobs, o_status, o_cjobs, o_carry[2], o_slots, bytes;
} zt_shape_t;
/* -> 0, or ZXC_ERROR_BAD_BLOCK_SIZE: the block size, max_piece < block_size, more than 2^31 - 2 blocks in dst_capacity or jobs
 * in a chunk. A chunk of n <= max_piece bytes decodes the blocks that start inside it, at most max_piece / block_size + 1; J
 * keeps one more. Up to o_status the offsets are zc_shape's, so the container stages run on this work area as they are. */
ZC_FN int zt_shape(uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size, zt_shape_t* s) {
    zc_shape_t z;
    if (zc_shape(dst_capacity, block_size, &z) != 0 || max_piece < block_size) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t J = max_piece / block_size + 2u;
    if (J > 0x7FFFFFFEull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->n_jobs = z.n_jobs; s->n_tiles = z.n_tiles; s->J = (uint32_t)J; s->slot_stride = block_size + ZT_SLOT_PAD; s->rsv = 0;
    s->copy_chunks = (block_size + 15u + ZT_COPY_CHUNK - 1u) / ZT_COPY_CHUNK; /* a copy of n bytes spans < n + 16 from its aligned start */
    s->o_tile_sum = z.o_tile_sum; s->o_tile_hash = z.o_tile_hash; s->o_tile_bad = z.o_tile_bad; s->o_jobs = z.o_jobs; s->o_status = z.o_status;
    uint64_t o = z.o_stage; /* (behind the status tables; zc_shape's staged slots are not kept) */
    s->o_cjobs = o;    o = zc_round_up(o + 2ull * J * sizeof(zxc_dev_job_t), 256u);
    s->o_carry[0] = o; o = zc_round_up(o + s->slot_stride, 256u);
    s->o_carry[1] = o; o = zc_round_up(o + s->slot_stride, 256u);
    s->o_slots = o;    o = zc_round_up(o + J * s->slot_stride, 256u);
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}
/* the closed form the header states */
ZC_FN uint64_t zt_work_bound(uint64_t dst_capacity, uint64_t max_piece, uint32_t block_size) {
    const uint64_t n_jobs = dst_capacity / block_size + (dst_capacity % block_size != 0) + 1u, J = max_piece / block_size + 2u;
    return ZT_BLOCK_BYTES * n_jobs + ZT_TILE_BYTES * ((n_jobs + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS) +
           J * ((uint64_t)block_size + ZT_SLOT_PAD + ZT_JOB_BYTES) + ZT_CARRIES * ((uint64_t)block_size + ZT_SLOT_PAD) + ZT_WORK_FIXED;
}

/* ---- the plan of one chunk: n > 0 bytes at decoded position pos, delivered to d[0, n) */
enum { ZT_NONE = 0, ZT_DIRECT = 1, ZT_SLOT = 2, ZT_CARRY = 3 };

typedef struct zt_chunk {
    uint64_t pos;        /* decoded position of the chunk's first byte */
    uint64_t n;          /* bytes of the chunk */
    uint64_t first;      /* index of the first block the chunk decodes */
    uint32_t block_size;
    uint32_t head_at;    /* pos mod block_size: where in the waiting block the chunk starts */
    uint32_t head;       /* bytes copied out of the carry slot: the rest of that block, or all n (0 when pos is a block boundary) */
    uint32_t whole;      /* blocks that lie wholly inside the chunk */
    uint32_t n_direct;   /* of those, the leading ones are decoded where they belong ... */
    uint32_t tail;       /* bytes wanted of the block the chunk ends inside, which is decoded into the other carry slot */
    uint32_t nb;         /* blocks the chunk decodes: whole + (tail != 0) */
    uint32_t cur;        /* the carry slot that holds block pos / block_size */
    uint32_t swap;       /* the tail's block went to the other carry slot: the two change roles behind this chunk */
    uint32_t rsv;
} zt_chunk_t;

/* A take of `left` bytes at position pos: the bytes of its next chunk. At most max_piece (>= block_size), and all of them when
 * they fit; else as many as end on a block boundary of the archive, so that only a take's last chunk leaves a block waiting. */
ZC_FN uint64_t zt_chunk_len(uint64_t pos, uint64_t left, uint64_t max_piece, uint32_t block_size) {
    const uint64_t at = pos % block_size;
    return left <= max_piece ? left : (at + max_piece) / block_size * block_size - at;
}
/* room >= n: the bytes of the take from the chunk's first byte on (what a store behind a block may still hit and a later chunk
 * of the same take overwrites in stream order). dst_lo4: the low four bits of d. A whole block i lies at d + head + i bs; it is
 * decoded there when that place is 16-byte aligned and its slot plus the decoders' 32 bytes, head + (i + 1) bs + 32 <= room, end
 * inside the piece (zc_shape's k_direct): the leading n_direct of them, the others (at most one when the place is aligned) go
 * through slots 0 .. whole - n_direct - 1. Every byte of d[0, n) lies in one direct block or is written by one copy. */
ZC_FN void zt_plan_chunk(uint64_t pos, uint64_t n, uint64_t room, uint32_t dst_lo4, uint32_t block_size, uint32_t cur, zt_chunk_t* c) {
    c->pos = pos; c->n = n; c->block_size = block_size; c->cur = cur; c->rsv = 0;
    c->head_at = (uint32_t)(pos % block_size);
    const uint64_t in_block = block_size - c->head_at;
    c->head = c->head_at ? (uint32_t)(n < in_block ? n : in_block) : 0u;
    const uint64_t rest = n - c->head;
    c->first = (pos + c->head) / block_size; /* (rest > 0: pos + head is a block boundary) */
    c->whole = (uint32_t)(rest / block_size);
    c->tail = (uint32_t)(rest % block_size);
    const int aligned = ((dst_lo4 + c->head) & 15u) == 0;
    uint64_t direct = (aligned && room >= (uint64_t)c->head + ZT_SPILL) ? (room - c->head - ZT_SPILL) / block_size : 0u;
    if (direct > c->whole) direct = c->whole;
    c->n_direct = (uint32_t)direct;
    c->nb = c->whole + (c->tail ? 1u : 0u);
    c->swap = c->tail ? 1u : 0u;
}
/* `end`: block n_max = ceil(dst_capacity / block_size), the one job behind the capacity, into slot 0 (only its status counts) */
ZC_FN void zt_plan_extra(uint64_t n_max, uint32_t block_size, uint32_t cur, zt_chunk_t* c) {
    c->pos = n_max * block_size; c->n = 0; c->first = n_max; c->block_size = block_size; c->head_at = 0; c->head = 0; c->whole = 1;
    c->n_direct = 0; c->tail = 0; c->nb = 1; c->cur = cur; c->swap = 0; c->rsv = 0;
}
/* the session behind a chunk */
ZC_FN void zt_advance(const zt_chunk_t* c, uint64_t* pos, uint32_t* cur) {
    *pos += c->n;
    if (c->swap) *cur ^= 1u;
}

/* where job j < nb of the chunk (block first + j) is decoded: straight at d + at, into slot `slot`, or into carry slot `slot` */
typedef struct zt_place {
    uint32_t kind, slot;
    uint64_t at;
} zt_place_t;
ZC_FN zt_place_t zt_job_place(const zt_chunk_t* c, uint32_t j) {
    zt_place_t p = {ZT_CARRY, c->cur ^ 1u, 0u};
    if (j < c->n_direct) { p.kind = ZT_DIRECT; p.slot = 0; p.at = c->head + (uint64_t)j * c->block_size; }
    else if (j < c->whole) { p.kind = ZT_SLOT; p.slot = j - c->n_direct; }
    return p;
}
/* Copy k < nb + 1 of the chunk: d[to, to + len) = bytes [from, from + len) of block `block`, which lie in slot / carry slot
 * `slot`. k == 0 is the head out of the waiting block, k == 1 + j belongs to job j. kind == ZT_NONE: no copy. */
typedef struct zt_copy {
    uint32_t kind, slot, from, len;
    uint64_t to, block;
} zt_copy_t;
ZC_FN zt_copy_t zt_copy(const zt_chunk_t* c, uint32_t k) {
    zt_copy_t cp = {ZT_NONE, 0u, 0u, 0u, 0u, 0u};
    if (k == 0) {
        if (c->head) { cp.kind = ZT_CARRY; cp.slot = c->cur; cp.from = c->head_at; cp.len = c->head; cp.block = c->pos / c->block_size; }
        return cp;
    }
    const uint32_t j = k - 1u;
    if (j >= c->nb) return cp;
    const zt_place_t p = zt_job_place(c, j);
    if (p.kind == ZT_DIRECT) return cp;
    cp.kind = p.kind; cp.slot = p.slot; cp.len = p.kind == ZT_SLOT ? c->block_size : c->tail;
    cp.to = c->head + (uint64_t)j * c->block_size; cp.block = c->first + j;
    return cp;
}
/* ... and the bytes it moves once the block's status is known: min(decoded size, bytes wanted of it) */
ZC_FN uint32_t zt_copy_bytes(const zt_copy_t* cp, int32_t status, uint32_t block_size) {
    const uint32_t have = status <= 0 ? 0u : (uint32_t)status < block_size ? (uint32_t)status : block_size;
    if (cp->kind == ZT_NONE || cp->from >= have) return 0;
    return cp->len < have - cp->from ? cp->len : have - cp->from;
}
#endif
