/* zxc_ranges.h — the rules of zxc_mi355x_seekable_open_device and zxc_mi355x_decompress_ranges_device on top of
 * zxc_container.h: the index a seek table becomes, when it is accepted, what a range may ask for, which block job (r, j) is,
 * whether that block is decoded straight into the destination or into a staged slot, what is copied out of a slot, the
 * per-range result, and the call's shape. The range rules are written once for the three front ends of the family, ranges, rangesv
 * (zxc_rangesv.h) and the shuffled ranges (zxc_rangesv_shuffle.h): a front end builds a zr_req_t of its table entry, says whether a
 * block may be decoded in place and how a block's status is held, and has a record of its own for the copy-out. Plain inline C that
 * hipcc and a host C compiler both take, so that the kernels of zxc_ranges_device.hip and zxc_rangesv_shuffle_device.hip and the CPU
 * tests run the same lines. Every function states what zxc_seekable_open / zxc_seekable_decompress_range (zxc_host.c) do for the
 * same bytes; where the device call departs from them, it says so. */
#ifndef ZXC_RANGES_H
#define ZXC_RANGES_H
#include "zxc_container.h"

#define ZR_OPEN_MIN (ZC_FILE_HDR + 2u * ZC_BLK_HDR + ZC_FOOTER) /* 44: file header, EOF block, SEK header, footer */
#define ZR_INDEX_HDR 64u   /* bytes of zr_index_t in front of comp_offsets[] */
#define ZR_SLOT_PAD 64u    /* behind every staged slot: the decoders store up to 32 bytes past out_len, and slots stay 16-aligned */
#define ZR_COPY_CHUNK 8192u /* destination bytes one wavefront of the copy-out moves */
#define ZR_JOB_BYTES 44u   /* work area per job besides its slot: zxc_dev_job_t + status + zr_copy_t */
#define ZR_WORK_FIXED 1536u /* work area besides the jobs: alignment of the four parts and of the caller's pointer */

/* The index: this header, then comp_offsets[0 .. nb] (uint64_t archive offsets of the block headers, [nb] = the EOF block). */
typedef struct zr_index {
    int32_t status;      /* ZXC_OK once the table is accepted, else the negative zxc_error_t every range of this index gets */
    uint32_t nb;         /* blocks */
    uint64_t total;      /* footer: decoded size */
    uint32_t file_ck;    /* blocks carry 4-byte checksum trailers */
    uint32_t dict_id;    /* file header: non-zero = written with a dictionary */
    uint32_t block_size;
    uint32_t seek;       /* open's progress: 1 the head stage passed, 2 the entries sum to the EOF block */
    uint64_t eof_at;     /* archive offset of the EOF block header */
    uint64_t rsv[3];
} zr_index_t;

/* A staged job's copy-out: slot[from, from + n) -> d_dst[dst_at, dst_at + n), when the block decoded to at least from + n bytes.
 * n == 0: nothing to copy (an empty job, or a block decoded straight into the destination). */
typedef struct zr_copy {
    uint64_t dst_at;
    uint32_t from, n;
} zr_copy_t;

ZC_FN uint64_t zr_index_size(uint32_t max_blocks) { return ZR_INDEX_HDR + 8ull * ((uint64_t)max_blocks + 1u); }
ZC_FN uint32_t zr_open_tiles(uint32_t max_blocks) { return max_blocks ? (max_blocks + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS : 1u; }
ZC_FN uint64_t* zr_offsets(void* index) { return (uint64_t*)((uint8_t*)index + ZR_INDEX_HDR); }
ZC_FN const uint64_t* zr_coffsets(const void* index) { return (const uint64_t*)((const uint8_t*)index + ZR_INDEX_HDR); }

/* ---- open. zxc_seekable_open over src[0, src_size), src_size >= 44: the file header, a non-zero footer size, a SEK header with
 * a valid check byte and length 4 nb where the footer says it is, a valid EOF header right in front of it. Two additions: the
 * header's block size is the argument's (the caller sized everything with it), and nb <= max_blocks (the index holds no more).
 * -> status stays negative; seek = 1 when the entries are worth summing. */
ZC_FN void zr_open_head(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, zr_index_t* ix) {
    uint32_t lg = 0, ck = 0, dict_id = 0;
    ix->status = ZXC_ERROR_CORRUPT_DATA; ix->nb = 0; ix->total = 0; ix->file_ck = 0; ix->dict_id = 0; ix->block_size = block_size;
    ix->seek = 0; ix->eof_at = 0; ix->rsv[0] = ix->rsv[1] = ix->rsv[2] = 0;
    int rc = zc_file_header(src, &lg, &ck, &dict_id);
    if (rc == ZXC_OK && (1u << lg) != block_size) rc = ZXC_ERROR_BAD_BLOCK_SIZE; /* departure, as zc_head */
    if (rc != ZXC_OK) { ix->status = rc; return; }
    const uint64_t total = zc_rd64(src + src_size - ZC_FOOTER);
    if (total == 0) return;
    const uint64_t nb = total / block_size + (total % block_size != 0);
    if (nb > 0xFFFFFFFFull) return;
    if (nb > max_blocks) { ix->status = ZXC_ERROR_MEMORY; return; }
    uint64_t eof_at = 0, eof = 0;
    if (!zc_seek_tail(src, src_size, nb, &eof_at, &eof)) return; /* (the EOF header's size field is not looked at, as on the host) */
    ix->nb = (uint32_t)nb; ix->total = total; ix->file_ck = ck; ix->dict_id = dict_id; ix->eof_at = eof_at;
    ix->seek = 1;
}
ZC_FN const uint8_t* zr_entries(const uint8_t* src, const zr_index_t* ix) { return src + ix->eof_at + 2u * ZC_BLK_HDR; }
/* seekable_build: an entry is at least a block header. Departure: none above ZC_SEEK_ENTRY_MAX (4 MiB; the tile sums are 32-bit;
 * no legal block, at most 2 MiB of payload, is that large). The host's "entry and running sum <= archive size" follow from the
 * sum landing on the EOF block. */
ZC_FN int zr_entry_ok(uint32_t e) { return zc_seek_entry_ok(e, 0u); }
/* the entries summed from offset 16 land on the EOF block -> the table is accepted */
ZC_FN void zr_open_judge(zr_index_t* ix, int any_bad, uint64_t sum) {
    if (!any_bad && ZC_FILE_HDR + sum == ix->eof_at) { ix->status = ZXC_OK; ix->seek = 2; }
}
/* The passes in series (tests; the kernels run the same element functions over tiles). index: zr_index_size(max_blocks) bytes. */
ZC_FN void zr_open_serial(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t max_blocks, void* index) {
    zr_index_t* ix = (zr_index_t*)index;
    uint64_t* offs = zr_offsets(index);
    zr_open_head(src, src_size, block_size, max_blocks, ix);
    if (ix->seek != 1u) return;
    const uint8_t* ent = zr_entries(src, ix);
    uint64_t sum = 0;
    int bad = 0;
    for (uint32_t i = 0; i < ix->nb; i++) {
        const uint32_t e = zc_rd32(ent + 4ull * i);
        if (zr_entry_ok(e)) sum += e;
        else bad = 1;
    }
    zr_open_judge(ix, bad, sum);
    if (ix->status != ZXC_OK) return;
    uint64_t run = ZC_FILE_HDR;
    for (uint32_t i = 0; i < ix->nb; i++) { offs[i] = run; run += zc_rd32(ent + 4ull * i); }
    offs[ix->nb] = run;
}

/* ---- a range. What a range asks for, whichever front end it came through: plain bytes [offset, offset + len) to `place`, the
 * destination of the range's first byte counted from the decode launch's d_out modulo 2^64 (a destination may lie above or below
 * d_out; the decode and copy kernels only ever add such an offset to a base in 64 bits, the convention of takev,
 * zxc_take_device.hip), and dst_err: 0, or the refusal the front end's own destination check gives. The request builder is all a
 * front end contributes to the rules: zr_req here, zrv_req (zxc_rangesv.h) for rangesv and the shuffled ranges. d_out is a multiple
 * of 16, so a place has its address's alignment. */
typedef struct zr_req {
    uint64_t offset, len, place;
    int32_t dst_err;
} zr_req_t;
/* ranges: offsets into one 16-aligned buffer d_dst = d_out + dst_rel. max_len is the capacity the launch was sized for */
ZC_FN zr_req_t zr_req(zxc_dev_range_t r, uint64_t max_len, uint64_t dst_capacity, uint64_t dst_rel) {
    zr_req_t q;
    q.offset = r.offset; q.len = r.len; q.place = dst_rel + r.dst_off;
    q.dst_err = (r.len > max_len || r.dst_off > dst_capacity || r.len > dst_capacity - r.dst_off) ? ZXC_ERROR_DST_TOO_SMALL : 0;
    return q;
}
/* What is decided before any block is looked at, in zxc_seekable_decompress_range's order (seek_range_check, then range_source's
 * bound): -> 1 and *result when the range is answered already, 0 when its blocks decide.
 * have_dict / have_id: the caller's dictionary and its zxc_dict_id. An archive written with a dictionary wants one
 * (seek_range_check) and that one (zxc_seekable_set_dict refuses another with DICT_MISMATCH; here the range is refused). */
ZC_FN int zr_req_final(const zr_index_t* ix, zr_req_t q, uint64_t src_size, uint32_t block_size, int have_dict, uint32_t have_id,
                         int64_t* result) {
    if (q.len == 0) { *result = 0; return 1; }
    if (ix->status < 0) { *result = ix->status; return 1; }
    if (ix->block_size != block_size) { *result = ZXC_ERROR_BAD_BLOCK_SIZE; return 1; } /* (an index opened with another size) */
    if (q.dst_err != 0) { *result = q.dst_err; return 1; }
    if (q.offset > ix->total || q.len > ix->total - q.offset) { *result = ZXC_ERROR_SRC_TOO_SMALL; return 1; }
    if (ix->dict_id != 0 && !have_dict) { *result = ZXC_ERROR_DICT_REQUIRED; return 1; }
    if (ix->dict_id != 0 && have_id != ix->dict_id) { *result = ZXC_ERROR_DICT_MISMATCH; return 1; }
    if (ix->eof_at + ZC_BLK_HDR > src_size) { *result = ZXC_ERROR_SRC_TOO_SMALL; return 1; } /* fewer bytes than were opened */
    return 0;
}
/* bytes [*from, *to) of block b (counted from the block's first byte) that a non-final range wants; from == to: not covered */
ZC_FN void zr_wanted(zr_req_t q, uint64_t b, uint32_t block_size, uint32_t* from, uint32_t* to) {
    const uint64_t lo = b * block_size, hi = lo + block_size, end = q.offset + q.len;
    const uint64_t f = q.offset > lo ? q.offset : lo, t = end < hi ? end : hi;
    *from = *to = 0;
    if (t > f) { *from = (uint32_t)(f - lo); *to = (uint32_t)(t - lo); }
}
/* the length the index gives block b < nb: min(block_size, total - b block_size) */
ZC_FN uint32_t zr_block_len(const zr_index_t* ix, uint64_t b, uint32_t block_size) {
    const uint64_t left = ix->total - b * block_size;
    return left < block_size ? (uint32_t)left : block_size;
}
/* Block b of a valid range decodes straight to its place d_out + place + b bs - offset: all of it is wanted, the place is 16-byte
 * aligned, and the block plus the 32 bytes the decoders may store behind it end inside the range's own destination:
 * place + bs + 32 <= the range's end is b bs + bs + 32 <= offset + len. Nothing is promised writable behind a range, so a range's
 * last whole block is staged unless 32 more bytes of the range follow it. */
ZC_FN int zr_req_direct(zr_req_t q, uint64_t b, uint32_t block_size) {
    const uint64_t lo = b * block_size;
    if (lo < q.offset || lo + block_size + 32u > q.offset + q.len) return 0;
    return ((q.place + (lo - q.offset)) & 15u) == 0;
}
/* What job (r, j) moves out of its staged slot once its block is decoded: plain bytes [from, from + n) of block b -> d_out + dst_at.
 * n == 0, everything 0: nothing (an empty job, or a block decoded straight to its place). */
typedef struct zr_part {
    uint64_t b, dst_at;
    uint32_t from, n;
} zr_part_t;
/* Job j of range r (job_index = r J + j): block offset / bs + j while the range reaches it, else an empty job (comp_size 0: the
 * decoder answers with an error status and touches nothing). out_len is a whole block, as range_source has it. Staged slot i is
 * d_out + stage_rel + i slot_stride. may_direct: the front end lets a block be decoded in place (zr_req_direct); the planes of a
 * shuffled block never are. A front end makes its record of *p: zr_copy_of here, zrs_job's own lines (zxc_rangesv_shuffle.h). */
ZC_FN void zr_req_job(const void* index, zr_req_t q, uint32_t j, uint64_t job_index, uint64_t src_size, uint32_t block_size, uint64_t stage_rel,
                  int may_direct, int have_dict, uint32_t have_id, zxc_dev_job_t* job, zr_part_t* p) {
    const zr_index_t* ix = (const zr_index_t*)index;
    const uint64_t* offs = zr_coffsets(index);
    int64_t res;
    uint32_t from, to;
    job->comp_off = 0; job->out_off = stage_rel + job_index * ((uint64_t)block_size + ZR_SLOT_PAD); job->comp_size = 0; job->out_len = block_size;
    p->b = 0; p->dst_at = 0; p->from = 0; p->n = 0;
    if (zr_req_final(ix, q, src_size, block_size, have_dict, have_id, &res)) return;
    const uint64_t b = q.offset / block_size + j;
    zr_wanted(q, b, block_size, &from, &to);
    if (to == from) return;
    job->comp_off = offs[b];
    job->comp_size = (uint32_t)(offs[b + 1u] - offs[b]);
    const uint64_t at = q.place + (b * block_size + from - q.offset);
    if (may_direct && zr_req_direct(q, b, block_size)) job->out_off = at;
    else { p->b = b; p->dst_at = at; p->from = from; p->n = to - from; }
}
/* the copy record of a part, its destination counted from the pointer the copy-out is launched with, d_out + copy_rel (a multiple
 * of 16, which keeps dst_at & 15 the address's alignment): d_dst for ranges, d_out itself for rangesv */
ZC_FN zr_copy_t zr_copy_of(zr_part_t p, uint64_t copy_rel) {
    zr_copy_t cp;
    cp.dst_at = p.n ? p.dst_at - copy_rel : 0; cp.from = p.from; cp.n = p.n;
    return cp;
}
/* A covered block's own error, or CORRUPT_DATA; 0 = fine. exact == 0 is range_sink: the block decoded short of the `need` bytes
 * the range needs of it. exact != 0, the shuffled ranges' departure: it did not decode to exactly `need`, the length its planes
 * were laid out by (which contains "short of what the range needs": that is at most the block's length). */
ZC_FN int32_t zr_block_rule(int32_t status, uint32_t need, int exact) {
    if (status < 0) return status;
    return (exact ? (uint32_t)status != need : (uint32_t)status < need) ? ZXC_ERROR_CORRUPT_DATA : 0;
}
/* The range's result from its J statuses: the early verdict, then the first failing covered block in block order, else len. */
ZC_FN int64_t zr_req_verdict(const void* index, zr_req_t q, uint32_t J, const int32_t* status, uint64_t src_size, uint32_t block_size,
                         int exact, int have_dict, uint32_t have_id) {
    const zr_index_t* ix = (const zr_index_t*)index;
    int64_t res;
    if (zr_req_final(ix, q, src_size, block_size, have_dict, have_id, &res)) return res;
    const uint64_t b0 = q.offset / block_size;
    for (uint32_t j = 0; j < J; j++) {
        uint32_t from, to;
        zr_wanted(q, b0 + j, block_size, &from, &to);
        if (to == from) break;
        const int32_t v = zr_block_rule(status[j], exact ? zr_block_len(ix, b0 + j, block_size) : to, exact);
        if (v != 0) return v;
    }
    return (int64_t)q.len;
}
/* ---- the ranges front end: its table entry through the rules above (direct decodes allowed, statuses "at least"), under the
 * names its kernels and the CPU tests call. The launch's d_out is one base for both areas: d_dst = d_out + dst_rel, staged slot i
 * = d_out + stage_rel + i slot_stride. The twins without a dictionary pass none. */
ZC_FN int zr_direct(zxc_dev_range_t r, uint64_t b, uint32_t block_size) { return zr_req_direct(zr_req(r, r.len, ~0ull, 0u), b, block_size); }
ZC_FN void zr_job_dict(const void* index, zxc_dev_range_t r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                       uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel, int have_dict, uint32_t have_id,
                       zxc_dev_job_t* job, zr_copy_t* cp) {
    zr_part_t p;
    zr_req_job(index, zr_req(r, max_len, dst_capacity, dst_rel), j, job_index, src_size, block_size, stage_rel, 1, have_dict, have_id, job, &p);
    *cp = zr_copy_of(p, dst_rel);
}
ZC_FN void zr_job(const void* index, zxc_dev_range_t r, uint32_t j, uint64_t job_index, uint64_t src_size, uint64_t max_len,
                  uint64_t dst_capacity, uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel, zxc_dev_job_t* job, zr_copy_t* cp) {
    zr_job_dict(index, r, j, job_index, src_size, max_len, dst_capacity, block_size, dst_rel, stage_rel, 0, 0u, job, cp);
}
ZC_FN int64_t zr_verdict_dict(const void* index, zxc_dev_range_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                              uint64_t dst_capacity, uint32_t block_size, int have_dict, uint32_t have_id) {
    return zr_req_verdict(index, zr_req(r, max_len, dst_capacity, 0u), J, status, src_size, block_size, 0, have_dict, have_id);
}
ZC_FN int64_t zr_verdict(const void* index, zxc_dev_range_t r, uint32_t J, const int32_t* status, uint64_t src_size, uint64_t max_len,
                         uint64_t dst_capacity, uint32_t block_size) {
    return zr_verdict_dict(index, r, J, status, src_size, max_len, dst_capacity, block_size, 0, 0u);
}

/* ---- the call's shape, known to the host before any byte of the archive or of the range table */
typedef struct zr_shape {
    uint32_t J, n_jobs, slot_stride; /* jobs per range; n_ranges J; bytes per slot */
    union { uint32_t copy_chunks, chunks; }; /* copy-out (gather) chunks per job */
    uint64_t o_jobs, o_status; /* work-area offsets from its 256-byte aligned base */
    union { uint64_t o_copy, o_gather; }; /* the front end's records: zr_copy_t, or the shuffled ranges' zrs_gather_t */
    uint64_t o_stage, bytes;
} zr_shape_t;
/* copy-out chunks of a job's zr_copy_t: a copy of n bytes spans < n + 16 from its aligned start */
ZC_FN uint32_t zr_copy_chunks(uint32_t block_size) { return (block_size + 15u + ZR_COPY_CHUNK - 1u) / ZR_COPY_CHUNK; }
/* -> 0, ZXC_ERROR_BAD_BLOCK_SIZE, or ZXC_ERROR_MEMORY (more jobs than a launch counts). A range of len <= max_len touches at
 * most (max_len - 1) / bs + 2 blocks. rec_bytes, chunks: the front end's record per job (at o_copy) and its copy-out chunks per
 * job: sizeof(zr_copy_t) and zr_copy_chunks, or the shuffled ranges' zrs_gather_t and chunks of ZRS_CHUNK (zrs_shape). */
ZC_FN int zr_shape_of(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, uint32_t rec_bytes, uint32_t chunks, zr_shape_t* s) {
    if (!zc_block_size_ok(block_size)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t J = max_len ? (max_len - 1u) / block_size + 2u : 1u;
    if (J > 0x7FFFFFFEull || J * n_ranges > 0x7FFFFFFEull) return ZXC_ERROR_MEMORY;
    s->J = (uint32_t)J;
    s->n_jobs = (uint32_t)(J * n_ranges);
    s->slot_stride = block_size + ZR_SLOT_PAD;
    s->copy_chunks = chunks;
    uint64_t o = 0;
    s->o_jobs = o;   o = zc_round_up(o + (uint64_t)s->n_jobs * sizeof(zxc_dev_job_t), 256u);
    s->o_status = o; o = zc_round_up(o + 4ull * s->n_jobs, 256u);
    s->o_copy = o;   o = zc_round_up(o + (uint64_t)s->n_jobs * rec_bytes, 256u);
    s->o_stage = o;  o += (uint64_t)s->n_jobs * s->slot_stride;
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}
/* the shape of ranges and rangesv */
ZC_FN int zr_shape(uint32_t n_ranges, uint64_t max_len, uint32_t block_size, zr_shape_t* s) {
    return zr_shape_of(n_ranges, max_len, block_size, sizeof(zr_copy_t), zr_copy_chunks(block_size), s);
}
#endif
