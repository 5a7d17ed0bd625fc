/* zxc_batch.h — the rules of zxc_mi355x_decompress_batch_device on top of zxc_container.h: the call's shape, an item's effective
 * capacity and source bounds, the plan of one item (head, header walk, jobs, global hash), whether a block is decoded straight
 * into the destination or into a staged slot, and the per-item result. Plain inline C that hipcc and a host C compiler both
 * take, so that the kernels of zxc_batch_device.hip and the CPU tests run the same lines. An item is judged as zxc_decompress
 * (zxc_host.c) judges the same bytes with the item's effective capacity; where the call departs from it, the function says so. */
#ifndef ZXC_BATCH_H
#define ZXC_BATCH_H
#include "zxc_container.h"

#define ZB_SLOT_PAD 64u     /* behind every staged slot: the decoders store up to 32 bytes past out_len, and slots stay 16-aligned */
#define ZB_COPY_CHUNK 8192u /* destination bytes one wavefront of the copy-out moves */
#define ZB_REC_BYTES 128u   /* work area per item: zb_rec_t */
#define ZB_JOB_BYTES 56u    /* work area per job besides its slot: two zxc_dev_job_t and two statuses */
#define ZB_WORK_FIXED 1536u /* work area besides items and jobs: alignment of the four parts and of the caller's pointer */

/* Per-item state: what zc_ctl_t is to zxc_mi355x_decompress_device, and the two item fields the later stages need. */
typedef struct zb_rec {
    zc_ctl_t c;       /* (seek and eof_at stay 0: the table is not used; event stays ZC_NO_EVENT, zb_verdict_item finds it) */
    uint64_t cap;     /* the item's effective capacity */
    uint64_t dst_off;
    uint64_t rsv[4];
} zb_rec_t;

/* ---- the call's shape, known to the host before any byte of the item table or of an archive */
typedef struct zb_shape {
    uint32_t J, n_jobs, slot_stride, copy_chunks; /* jobs per item; n_items J; bytes per slot; copy-out chunks per job */
    uint64_t o_rec, o_jobs, o_status, o_stage, bytes; /* work-area offsets from its 256-byte aligned base */
} zb_shape_t;
/* -> 0, ZXC_ERROR_BAD_BLOCK_SIZE, or ZXC_ERROR_MEMORY (more jobs than a launch counts). J = ceil(max_capacity / bs) + 1 is
 * zc_shape's n_max + 1 for the largest item: an archive with more blocks cannot fit, and the extra job lets a failing block
 * behind a full destination keep its precedence over DST_TOO_SMALL. */
ZC_FN int zb_shape(uint32_t n_items, uint64_t max_capacity, uint32_t block_size, zb_shape_t* s) {
    if (!zc_block_size_ok(block_size)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    uint64_t J = max_capacity / block_size + (max_capacity % block_size != 0) + 1u;
    if (n_items && (J > 0x7FFFFFFEull || J * n_items > 0x7FFFFFFEull)) return ZXC_ERROR_MEMORY;
    if (J > 0x7FFFFFFEull) J = 0x7FFFFFFEull; /* (no item: nothing is sized by it) */
    s->J = (uint32_t)J;
    s->n_jobs = (uint32_t)(J * n_items);
    s->slot_stride = block_size + ZB_SLOT_PAD;
    s->copy_chunks = (block_size + 15u + ZB_COPY_CHUNK - 1u) / ZB_COPY_CHUNK; /* a copy of n bytes spans < n + 16 from its aligned start */
    uint64_t o = 0;
    s->o_rec = o;    o = zc_round_up(o + (uint64_t)n_items * sizeof(zb_rec_t), 256u);
    s->o_jobs = o;   o = zc_round_up(o + 2ull * s->n_jobs * sizeof(zxc_dev_job_t), 256u); /* two tables: see zc_ctl_t.sel */
    s->o_status = o; o = zc_round_up(o + 2ull * s->n_jobs * 4u, 256u);
    s->o_stage = o;  o += (uint64_t)s->n_jobs * s->slot_stride;
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}

/* ---- an item. Its effective capacity: what the item allows, what the launch was sized for, what d_dst holds behind dst_off. */
ZC_FN uint64_t zb_cap(zxc_dev_item_t it, uint64_t max_capacity, uint64_t dst_capacity) {
    if (it.dst_off > dst_capacity) return 0;
    const uint64_t room = dst_capacity - it.dst_off;
    uint64_t cap = it.dst_capacity < max_capacity ? it.dst_capacity : max_capacity;
    if (cap > room) cap = room;
    return cap;
}
/* Departure: an item shorter than a file header and a footer, or one that does not lie inside d_src[0, src_capacity) (compared
 * without overflow), is ZXC_ERROR_SRC_TOO_SMALL, and none of its bytes is read. */
ZC_FN int zb_src_ok(zxc_dev_item_t it, uint64_t src_capacity) {
    return it.src_size >= ZC_FILE_HDR + ZC_FOOTER && it.src_off <= src_capacity && it.src_size <= src_capacity - it.src_off;
}
/* Block i of an item decodes straight to its place d_dst + dst_off + i bs: the place is 16-byte aligned (d_dst is), and the slot
 * plus the 32 bytes the decoders may store behind it end inside the item's own capacity. */
ZC_FN int zb_direct(uint64_t dst_off, uint32_t i, uint32_t block_size, uint64_t cap) {
    return ((dst_off + (uint64_t)i * block_size) & 15u) == 0 && ((uint64_t)i + 1u) * block_size + 32u <= cap;
}
/* Job i of item r (job_index = r J + i) for the block whose header is at archive offset comp_off of d_src. out_len is a whole
 * block, as frame_source of zxc_host.c has it. The launch's d_out is one base for both areas: d_dst = base + dst_rel, staged
 * slot job_index = base + stage_rel + job_index slot_stride. */
ZC_FN zxc_dev_job_t zb_job(uint64_t comp_off, uint32_t comp_size, uint32_t i, uint64_t job_index, uint64_t dst_off, uint64_t cap,
                           uint32_t block_size, uint64_t dst_rel, uint64_t stage_rel) {
    zxc_dev_job_t j;
    j.comp_off = comp_off;
    j.out_off = zb_direct(dst_off, i, block_size, cap) ? dst_rel + dst_off + (uint64_t)i * block_size
                                                       : stage_rel + job_index * ((uint64_t)block_size + ZB_SLOT_PAD);
    j.comp_size = comp_size;
    j.out_len = block_size;
    return j;
}
/* an item answered before any of its blocks: the record of a call whose head stage decided */
ZC_FN void zb_rec_final(zb_rec_t* rec, int64_t result) {
    zc_ctl_t* c = &rec->c;
    c->head_result = result; c->total = 0; c->eof_at = 0; c->event = ZC_NO_EVENT; c->final = 1; c->file_ck = 0; c->verify = 0; c->sel = 0;
    c->stored_hash = 0; c->nb = 0; c->seek = 0; c->found = 0; c->done = 0; c->saw_eof = 0; c->tail_err = 0; c->ghash = 0;
}

/* ---- plan: item r of the table. The source bounds, then zxc_decompress's head over the item's bytes with its effective capacity
 * (zc_head_dict: the empty-frame probe, the file header, the block-size departure, the dictionary rule), then the block chain
 * from offset 16 as frame_source follows it (zc_chain_next), for at most the ceil(cap / bs) + 1 <= J blocks that
 * zxc_mi355x_decompress_device would look at with that capacity. The seek table is not looked at: the walk is the rule
 * zxc_decompress itself follows, an item has few blocks, and the items are walked in parallel. The jobs go into item r's J
 * entries of the table the head picked (jobs[sel n_jobs + r J + i]); the entries behind the blocks found, and all J of the other
 * table, are left as they are (the caller zeroed them: comp_size 0 is answered with an error status and nothing is read). The
 * global hash is folded by the walk. have_dict / have_id: the caller's dictionary and its zxc_dict_id. */
ZC_FN void zb_plan_item(const uint8_t* src, uint64_t src_capacity, zxc_dev_item_t it, uint32_t r, uint32_t J, uint32_t n_jobs,
                        uint64_t max_capacity, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint64_t dst_rel,
                        uint64_t stage_rel, int have_dict, uint32_t have_id, zb_rec_t* rec, zxc_dev_job_t* jobs) {
    zc_ctl_t* c = &rec->c;
    const uint64_t cap = zb_cap(it, max_capacity, dst_capacity);
    rec->cap = cap; rec->dst_off = it.dst_off; rec->rsv[0] = rec->rsv[1] = rec->rsv[2] = rec->rsv[3] = 0;
    if (!zb_src_ok(it, src_capacity)) { zb_rec_final(rec, ZXC_ERROR_SRC_TOO_SMALL); return; }
    const uint8_t* arc = src + it.src_off;
    zc_head_dict(arc, it.src_size, cap, block_size, want_verify, J, c, have_dict, have_id);
    c->seek = 0; c->eof_at = 0;
    if (c->final) return;
    uint64_t lim = cap / block_size + (cap % block_size != 0) + 1u;
    if (lim > J) lim = J; /* (cap <= max_capacity: never, and the item's J entries hold what is written) */
    const uint64_t first = (uint64_t)r * J;
    zxc_dev_job_t* tab = jobs + (uint64_t)c->sel * n_jobs + first;
    zc_chain_t ch = {ZC_FILE_HDR, 0, 0, 0, 0};
    uint32_t n = 0;
    while (n < lim) {
        const uint64_t at = ch.ip;
        const uint32_t cs = zc_chain_next(arc, it.src_size, c->file_ck, c->verify, &ch);
        if (cs) { tab[n] = zb_job(it.src_off + at, cs, n, first + n, it.dst_off, cap, block_size, dst_rel, stage_rel); n++; }
        if (ch.done) break;
    }
    c->found = n; c->done = ch.done; c->saw_eof = ch.saw_eof; c->tail_err = ch.tail_err; c->ghash = ch.ghash;
}

/* bytes of block i of the item that a copy-out moves from its slot to d_dst + dst_off + i bs (0: none, or the block went straight) */
ZC_FN uint32_t zb_copy_bytes(const zb_rec_t* rec, uint32_t i, int32_t status, uint32_t block_size) {
    if (rec->c.final || i >= rec->c.found || zb_direct(rec->dst_off, i, block_size, rec->cap)) return 0;
    return zc_tail_bytes(i, status, block_size, rec->cap);
}

/* ---- verdict: the item's result from its record and the J statuses of its table (status[sel n_jobs + r J ..]): the first
 * zc_block_event over the blocks found against the item's capacity, then zc_verdict's order. */
ZC_FN int64_t zb_verdict_item(const zb_rec_t* rec, const int32_t* status, uint32_t block_size) {
    zc_ctl_t c = rec->c;
    if (c.final) return c.head_result;
    for (uint32_t i = 0; i < c.found; i++) {
        const int32_t ev = zc_block_event(i, status[i], c.found, c.done, block_size, rec->cap);
        if (ev != 0) { c.event = zc_event_key(i, ev); break; }
    }
    return zc_verdict(&c, c.found ? status[c.found - 1u] : 0, block_size);
}
#endif
