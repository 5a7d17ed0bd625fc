/* zxc_takev.h — the rules of zxc_mi355x_decompress_takev_device on top of zxc_take.h and zxc_appendv.h: one call delivers the next
 * `total` decoded bytes into a table of (base, len) entries that lies in device memory. Plain inline C that hipcc and a host C
 * compiler both take, so that the kernels of zxc_take_device.hip and the CPU tests run the same lines: the scratch's shape and its
 * closed-form bound, the table's verdict and its fold into the session's control word, the plan of a chunk over a virtual
 * destination, the place of each job (in its entry, a slot or the next carry slot) and where byte k of a copy goes.
 *
 * The virtual destination of a call is the concatenation Y of its entries, total bytes; starts[r] is the offset of entry r in Y
 * (starts[n_iov] = total), the scan of zxc_appendv.h as it is. The host knows only n_iov and total: it cuts Y into chunks exactly as
 * a take cuts its piece (zt_chunk_len, zt_plan_chunk with nothing placed on the host), so grids, carry and position are the
 * host's. What the device decides is where a whole block is decoded: where it belongs when that place is 16-byte aligned and the
 * block and the decoders' 32-byte spill end inside ONE entry (the entry, not the chunk, bounds the spill: nothing is promised
 * writable behind an entry); every other whole block goes to the session's slot j and is copied out. The block a chunk ends inside
 * goes to the next carry slot, as in a take.
 *
 * Scratch, from its 256-byte aligned base: the call's control word, starts[0 .. n_iov], per tile of 1024 entries a sum and the
 * flags of the check, and per job of a chunk (J = max_piece / block_size + 2) its place record. In closed form the size is at most
 *     8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + 16 x J + 4096                             (ZTV_TILE_BYTES, ZTV_PLACE_BYTES, ZTV_FIXED) */
#ifndef ZXC_TAKEV_H
#define ZXC_TAKEV_H
#include "zxc_appendv.h"
#include "zxc_take.h"

#define ZTV_TILE_BYTES 16u   /* scratch per tile of 1024 entries: its sum, its flags */
#define ZTV_PLACE_BYTES 16u  /* scratch per job of a chunk: its place record */
#define ZTV_FIXED 4096u      /* the control word, the alignment of the four parts and of the caller's pointer */
#define ZTV_SINK 64u         /* in the control word's 256 bytes: the zap_ctl_t the scan of zxc_appendv.h folds into, which nobody reads */

/* ---- the scratch. Its control word is zav_ctl_t: status is the call's verdict (ztv_verdict of what the scan found). */
typedef struct ztv_place {
    uint32_t kind; /* ZT_DIRECT, ZT_SLOT, ZT_CARRY; ZT_NONE: an empty job (table error, or a session whose result is final) */
    uint32_t r;    /* the entry that holds the job's first byte */
    uint64_t rsv;
} ztv_place_t;
typedef struct ztv_shape {
    uint32_t J, n_tiles; /* place records; ceil(n_iov / 1024) */
    uint64_t o_starts, o_tile_sum, o_tile_flags, o_places, bytes;
} ztv_shape_t;
/* -> 0, or ZXC_ERROR_BAD_BLOCK_SIZE for what zt_shape refuses of these arguments */
ZC_FN int ztv_shape(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, ztv_shape_t* s) {
    if (!zc_block_size_ok(block_size) || max_piece < block_size) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t J = max_piece / block_size + 2u;
    if (J > 0x7FFFFFFEull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->J = (uint32_t)J;
    s->n_tiles = (uint32_t)(((uint64_t)n_iov + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS);
    uint64_t o = 256u; /* zav_ctl_t, and at ZTV_SINK the unread zap_ctl_t */
    s->o_starts = o;     o = zc_round_up(o + 8ull * ((uint64_t)n_iov + 1u), 256u);
    s->o_tile_sum = o;   o = zc_round_up(o + 8ull * s->n_tiles, 256u);
    s->o_tile_flags = o; o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_places = o;     o += J * ZTV_PLACE_BYTES;
    s->bytes = o + 256u; /* (the caller's d_scratch may have any alignment) */
    return 0;
}
/* the closed form the header states */
ZC_FN uint64_t ztv_scratch_bound(uint32_t n_iov, uint64_t max_piece, uint32_t block_size) {
    const uint64_t J = max_piece / block_size + 2u;
    return 8ull * ((uint64_t)n_iov + 1u) + ZTV_TILE_BYTES * (((uint64_t)n_iov + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS) + ZTV_PLACE_BYTES * J +
           ZTV_FIXED;
}

/* ---- the table's verdict. The check is zxc_appendv.h's (zav_entry_flags, zav_sat_add, zav_table_status: a zero base with a
 * length, then an entry longer than total or a sum above it, then a sum below it); a short table is fewer destination bytes than
 * promised, so ZXC_ERROR_SRC_TOO_SMALL reads ZXC_ERROR_DST_TOO_SMALL here. */
ZC_FN int ztv_verdict(int table_status) { return table_status == ZXC_ERROR_SRC_TOO_SMALL ? ZXC_ERROR_DST_TOO_SMALL : table_status; }
ZC_FN int ztv_table_status(uint32_t flags, uint64_t sum, uint64_t total) { return ztv_verdict(zav_table_status(flags, sum, total)); }
/* An error of the table becomes the session's result unless that is final already (a file-header error, a dictionary error, the
 * empty-frame probe, an earlier table): zc_verdict then reports it unchanged, and every copy of the session moves nothing. */
ZC_FN void ztv_fold(zc_ctl_t* c, int verdict) {
    if (verdict < 0 && !c->final) { c->final = 1u; c->head_result = verdict; }
}
/* The scan in series (tests; the kernels do the same per tile in parallel): starts[0 .. n_iov] -> the verdict. */
ZC_FN int ztv_scan_serial(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint64_t* starts) {
    return ztv_verdict(zav_scan_serial(iov, n_iov, total, starts));
}

/* ---- the plan of a chunk: m <= max_piece bytes of Y at virtual offset v, at decoded position pos. zt_plan_chunk with nothing
 * placed on the host (room 0: n_direct = 0, the host knows no addresses); head, whole blocks, tail, the carry swap, zt_copy,
 * zt_copy_bytes and zt_advance are zt_take.h's as they are. whole <= J - 1, so job j's slot is slot j. */
typedef struct ztv_chunk {
    zt_chunk_t c;
    uint64_t v;
} ztv_chunk_t;
ZC_FN void ztv_plan_chunk(uint64_t pos, uint64_t m, uint32_t block_size, uint32_t cur, uint64_t v, ztv_chunk_t* c) {
    zt_plan_chunk(pos, m, 0u, 0u, block_size, cur, &c->c);
    c->v = v;
}
/* A whole block that starts `off` bytes into an entry of len_r bytes at `base` is decoded where it belongs exactly when that
 * place is 16-byte aligned and the block and the decoders' spill end inside that entry (the mirror of zav_in_place). What the
 * spill hits are later virtual offsets of the same entry, hence of the same call: a copy of the same chunk or a later chunk fills
 * them afterwards in stream order. */
ZC_FN int ztv_in_place(uint64_t base, uint64_t off, uint64_t len_r, uint32_t block_size) {
    return ((base + off) & 15u) == 0 && off + block_size + ZT_SPILL <= len_r;
}
/* Job j < nb of the chunk: its place record, and in *addr where it is decoded (an address inside its entry, or of slot j, or of the
 * next carry slot). Reads the table: only behind a verdict of 0. */
ZC_FN ztv_place_t ztv_job_place(const ztv_chunk_t* c, uint32_t j, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov,
                                uint64_t carry0, uint64_t carry1, uint64_t slots, uint32_t slot_stride, uint64_t* addr) {
    const zt_place_t p = zt_job_place(&c->c, j); /* (n_direct = 0: a slot or the carry) */
    const uint64_t y = c->v + c->c.head + (uint64_t)j * c->c.block_size;
    ztv_place_t rec = {p.kind, zav_find(starts, 0u, n_iov - 1u, y), 0u};
    if (p.kind == ZT_CARRY) { *addr = p.slot ? carry1 : carry0; return rec; }
    const uint64_t off = y - starts[rec.r], base = iov[rec.r].base;
    if (ztv_in_place(base, off, starts[rec.r + 1u] - starts[rec.r], c->c.block_size)) { rec.kind = ZT_DIRECT; *addr = base + off; }
    else *addr = slots + (uint64_t)p.slot * slot_stride;
    return rec;
}

/* ---- the scatter, source-driven: the mirror of zav_fetch. cnt <= 16 bytes at s go to Y from virtual offset x on; [e_lo, e_hi] are
 * entries that hold the range (narrowed once per wavefront). One 16-byte load and one 16-byte store of any alignment when
 * cnt == 16 and the bytes lie inside one entry; else byte by byte into consecutive entries, past empty ones, whose base is not
 * looked at. Writes exactly the bytes it delivers. The cursor is the thread's, as in zav_fetch. */
ZC_FN void ztv_scatter(const uint8_t* s, uint32_t cnt, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo,
                       uint32_t e_hi, zav_cursor_t* cur) {
    if (x < cur->lo || x >= cur->hi) {
        cur->r = zav_find(starts, e_lo, e_hi, x);
        cur->lo = starts[cur->r]; cur->hi = starts[cur->r + 1u]; cur->base = iov[cur->r].base;
    }
    uint64_t off = x - cur->lo;
    if (cnt == 16u && x + 16u <= cur->hi) {
        zav_u128_t v;
        __builtin_memcpy(&v, s, 16);
        __builtin_memcpy((uint8_t*)(uintptr_t)cur->base + off, &v, 16);
        return;
    }
    for (uint32_t k = 0; k < cnt; k++) {
        if (cur->lo + off == cur->hi) {
            do { cur->r++; cur->lo = cur->hi; cur->hi = starts[cur->r + 1u]; } while (cur->hi == cur->lo);
            cur->base = iov[cur->r].base;
            off = 0;
        }
        ((uint8_t*)(uintptr_t)cur->base)[off++] = s[k];
    }
}
/* Unit u of the copy s[0, n) -> Y[y, y + n): source bytes [16 u, 16 u + 16) of the range, 16-byte aligned when s is (every copy
 * but a head out of the carry slot). ceil(n / 16) units cover the copy. */
ZC_FN uint64_t ztv_units(uint64_t n) { return (n + 15u) / 16u; }
ZC_FN void ztv_scatter_unit(const uint8_t* s, uint64_t n, uint64_t y, uint64_t u, const zxc_dev_iov_t* iov, const uint64_t* starts,
                            uint32_t e_lo, uint32_t e_hi, zav_cursor_t* cur) {
    const uint64_t lo = 16u * u, hi = lo + 16u < n ? lo + 16u : n;
    if (lo < hi) ztv_scatter(s + lo, (uint32_t)(hi - lo), y + lo, iov, starts, e_lo, e_hi, cur);
}
/* What lane `lane` of the wavefront that owns source bytes [8 KiB x ch, 8 KiB x (ch + 1)) of a scattered copy does: the search is
 * narrowed to the entries that meet those bytes (the same for every lane: once per wavefront), e_first being an entry at or in
 * front of the copy's first byte; the lane owns units lane, lane + 64, ... of them. */
ZC_FN void ztv_scatter_lane(const uint8_t* s, uint32_t n, uint64_t y, uint32_t ch, uint32_t lane, const zxc_dev_iov_t* iov,
                            const uint64_t* starts, uint32_t e_first, uint32_t n_iov) {
    const uint64_t lo = (uint64_t)ch * ZT_COPY_CHUNK, hi = lo + ZT_COPY_CHUNK < n ? lo + ZT_COPY_CHUNK : n;
    if (lo >= hi) return;
    const uint32_t e_lo = zav_find(starts, e_first, n_iov - 1u, y + lo), e_hi = zav_find(starts, e_lo, n_iov - 1u, y + hi - 1u);
    zav_cursor_t cur = {0u, 0u, 0u, 0u, 0u};
    for (uint64_t u = lo / 16u + lane; 16u * u < hi; u += 64u) ztv_scatter_unit(s, n, y, u, iov, starts, e_lo, e_hi, &cur);
}

/* ---- copy k of a chunk, as the copy kernel sees it: what zt_copy and the block's status say, the virtual range it fills, and
 * whether that range lies inside one entry (then `d` is its address there and the copy is zd_copy_chunk's; else it is the
 * scatter's, over entries [e_lo, e_hi]). rec: the job's place record (k > 0), NULL for the head, whose entry is searched here. */
typedef struct ztv_copy {
    uint32_t n, e_lo, one, rsv; /* bytes (0: nothing to do); the entry of the first byte; the range lies inside it */
    uint64_t y, d;
} ztv_copy_t;
ZC_FN ztv_copy_t ztv_copy_place(const ztv_chunk_t* c, const zt_copy_t* cp, uint32_t n, const ztv_place_t* rec, const zxc_dev_iov_t* iov,
                                const uint64_t* starts, uint32_t n_iov) {
    ztv_copy_t o = {n, 0u, 0u, 0u, c->v + cp->to, 0u};
    if (n == 0) return o;
    o.e_lo = rec ? rec->r : zav_find(starts, 0u, n_iov - 1u, o.y);
    if (o.y + n <= starts[o.e_lo + 1u]) { o.one = 1u; o.d = iov[o.e_lo].base + (o.y - starts[o.e_lo]); }
    return o;
}
#endif
