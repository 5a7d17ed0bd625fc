/* zxc_appendv.h — the rules of zxc_mi355x_compress_appendv_device on top of zxc_append.h: one call appends the concatenation of a
 * table of (base, len) entries that lies in device memory. Plain inline C that hipcc and a host C compiler both take, so that the
 * kernels of zxc_append_device.hip and the CPU tests run the same lines: the scratch's shape and its closed-form bound, the table
 * check, the search of the entry that holds a virtual offset, the plan of a chunk over a virtual source, the place of each job
 * (where it lies, or an image in the scratch) and where byte k of a virtual range comes from.
 *
 * The virtual source of a call is the concatenation X of its entries, total bytes; starts[r] is the offset of entry r in X
 * (starts[n_iov] = total), so entry r is X[starts[r], starts[r + 1]). The host knows only n_iov and total: it cuts X into chunks
 * exactly as an append cuts its source into pieces (zap_piece_len, zap_plan_piece), so grids, carry and block count are the host's.
 * What the device decides is where a job's bytes are read: a whole block that lies inside ONE entry with the encoder's over-read
 * inside that same entry is encoded where it lies (the entry, not the chunk, bounds the over-read: nothing is promised readable
 * behind an entry); every other whole block is gathered into an image of the scratch with ZAP_PAD zero bytes behind it. The head
 * that completes the waiting block and the tail are gathered into the session's carry areas as zxc_append_prep_kernel copies them.
 *
 * Scratch, from its 256-byte aligned base: the call's control word, starts[0 .. n_iov], per tile of 1024 entries a sum and the
 * flags of the check, and J = max_piece / block_size + 2 images of block_size + 256 bytes. In closed form the size is at most
 *     8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + J x (block_size + 256) + 4096          (ZAV_TILE_BYTES, ZAV_IMAGE_SLACK, ZAV_FIXED)
 *
 * The rules of zxc_mi355x_compress_appendv_dict_device, the same call in a session begun with a dictionary, stand at the end: the
 * scratch without images (zav_shape_dict) and the gather of [dict | block] images from the entries (zav_prep_images). */
#ifndef ZXC_APPENDV_H
#define ZXC_APPENDV_H
#include "zxc_append.h"

#define ZAV_TILE_BYTES 16u    /* scratch per tile of 1024 entries: its sum, its flags */
#define ZAV_IMAGE_SLACK 256u  /* an image is block_size + ZAP_PAD bytes, rounded up to the scratch's 256 */
#define ZAV_FIXED 4096u       /* the control word, the alignment of the four parts and of the caller's pointer */
#define ZAV_NULL 1u           /* flags of the check: an entry with len > 0 and base == 0 ... */
#define ZAV_BIG 2u            /* ... an entry longer than total */
#define ZAV_NO_JOB 0xFFFFFFFFu

/* ---- the scratch */
typedef struct zav_ctl {
    int32_t status; /* 0, or the table's error: then no kernel of the call reads an entry, encodes or gathers a block */
    uint32_t rsv;
    uint64_t sum;   /* the lengths added up (saturating) */
} zav_ctl_t;
typedef struct zav_shape {
    uint32_t J, n_tiles, image, rsv; /* images; ceil(n_iov / 1024); bytes per image */
    uint64_t o_starts, o_tile_sum, o_tile_flags, o_images, bytes;
} zav_shape_t;
/* -> 0, or ZXC_ERROR_BAD_BLOCK_SIZE for what zap_shape refuses of these arguments */
ZC_FN int zav_shape(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, zav_shape_t* s) {
    if (!zc_block_size_ok(block_size) || max_piece < block_size) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t J = max_piece / block_size + 2u;
    if (J > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->J = (uint32_t)J;
    s->n_tiles = (uint32_t)(((uint64_t)n_iov + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS);
    s->image = (uint32_t)zc_round_up((uint64_t)block_size + ZAP_PAD, 256u);
    s->rsv = 0;
    uint64_t o = 256u; /* zav_ctl_t */
    s->o_starts = o;     o = zc_round_up(o + 8ull * ((uint64_t)n_iov + 1u), 256u);
    s->o_tile_sum = o;   o = zc_round_up(o + 8ull * s->n_tiles, 256u);
    s->o_tile_flags = o; o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_images = o;     o += J * s->image;
    s->bytes = o + 256u; /* (the caller's d_scratch may have any alignment) */
    return 0;
}
/* the closed form the header states */
ZC_FN uint64_t zav_scratch_bound(uint32_t n_iov, uint64_t max_piece, uint32_t block_size) {
    const uint64_t J = max_piece / block_size + 2u;
    return 8ull * ((uint64_t)n_iov + 1u) + ZAV_TILE_BYTES * (((uint64_t)n_iov + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS) +
           J * ((uint64_t)block_size + ZAV_IMAGE_SLACK) + ZAV_FIXED;
}

/* ---- the table check. The lengths are added up saturating at 2^64 - 1, which keeps the order of the sum and `total` whatever the
 * entries say (total itself is below 2^52: the session's max_total is); min(a + b, 2^64 - 1) is associative, so tiles may add in
 * any grouping. Precedence: a zero base with a length, then an entry longer than total or a sum above it, then a sum below it. */
ZC_FN uint64_t zav_sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}
ZC_FN uint32_t zav_entry_flags(uint64_t base, uint64_t len, uint64_t total) {
    return ((len > 0 && base == 0) ? ZAV_NULL : 0u) | (len > total ? ZAV_BIG : 0u);
}
ZC_FN int zav_table_status(uint32_t flags, uint64_t sum, uint64_t total) {
    if (flags & ZAV_NULL) return ZXC_ERROR_NULL_INPUT;
    if ((flags & ZAV_BIG) || sum > total) return ZXC_ERROR_OVERFLOW;
    if (sum < total) return ZXC_ERROR_SRC_TOO_SMALL;
    return 0;
}
/* An error of the table becomes the session's unless it has one already. */
ZC_FN void zav_fold_status(zap_ctl_t* c, int status) {
    if (status < 0 && c->status >= 0) c->status = status;
}
/* The scan in series (tests; the kernels do the same per tile in parallel): starts[0 .. n_iov] -> the table's status. */
ZC_FN int zav_scan_serial(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint64_t* starts) {
    uint64_t sum = 0;
    uint32_t flags = 0;
    for (uint32_t r = 0; r < n_iov; r++) {
        starts[r] = sum;
        flags |= zav_entry_flags(iov[r].base, iov[r].len, total);
        sum = zav_sat_add(sum, iov[r].len);
    }
    starts[n_iov] = sum;
    return zav_table_status(flags, sum, total);
}

/* ---- the entry that holds a virtual offset: the largest r in [lo, hi] with starts[r] <= x, for starts[lo] <= x < starts[hi + 1].
 * An upper bound over the start offsets, so empty entries (starts[r] == starts[r + 1]) are never the answer. */
ZC_FN uint32_t zav_find(const uint64_t* starts, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (starts[mid] <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

/* ---- the plan of a chunk: m <= max_piece bytes of X at virtual offset v, behind `carry` waiting bytes. Blocks, head, tail and the
 * swap of the carry areas are zap_plan_piece's (its direct / staged split is not used: the place of a whole block is the
 * device's, zav_in_place). Prep runs one workgroup per job and one more: workgroup w's task is zav_task. */
typedef struct zav_chunk {
    zap_piece_t p;
    uint64_t v;
} zav_chunk_t;
ZC_FN void zav_plan_chunk(uint32_t carry, uint64_t m, uint32_t block_size, uint64_t v, zav_chunk_t* c) {
    zap_plan_piece(carry, m, block_size, &c->p);
    c->v = v;
}
ZC_FN uint32_t zav_groups(const zav_chunk_t* c) { return c->p.nb + 1u; }

enum { ZAV_TO_CARRY = 1, ZAV_TO_NEXT = 2, ZAV_BLOCK = 3 };
/* X[vlo, vlo + len): gathered into the carry area at `at` (the head that completes the waiting block, or with no block completed
 * all the chunk's bytes), into the other carry area (the tail), or a whole block, in place or into image `at`. job: the job-table
 * entry the workgroup writes (ZAV_NO_JOB: none). */
typedef struct zav_task {
    uint32_t kind, at, len, job;
    uint64_t vlo;
} zav_task_t;
ZC_FN zav_task_t zav_task(const zav_chunk_t* c, uint32_t w) {
    const zap_piece_t* p = &c->p;
    zav_task_t t = {ZAV_TO_CARRY, p->carry, 0u, ZAV_NO_JOB, c->v};
    if (w < p->nb) {
        t.job = w;
        if (p->carry && w == 0) { t.len = p->cp[0].len; return t; }
        const uint32_t i = w - (p->carry ? 1u : 0u);
        t.kind = ZAV_BLOCK; t.at = i; t.len = p->block_size; t.vlo = c->v + p->first + (uint64_t)i * p->block_size;
        return t;
    }
    if (p->nb == 0) { t.len = (uint32_t)p->n; return t; }
    t.kind = ZAV_TO_NEXT; t.at = 0; t.len = p->tail; t.vlo = c->v + p->n - p->tail;
    return t;
}
/* A whole block that starts `off` bytes into an entry of len_r bytes is encoded where it lies exactly when the block and the
 * encoder's over-read end inside that entry. */
ZC_FN int zav_in_place(uint64_t off, uint64_t len_r, uint32_t block_size) {
    return off + block_size + ZAP_OVERREAD <= len_r;
}

/* ---- the gather, destination-driven. cnt <= 16 bytes of X from virtual offset x on go to d; [e_lo, e_hi] are entries that hold
 * the range (narrowed once per workgroup). One 16-byte load of any alignment and one aligned 16-byte store when cnt == 16 (the
 * caller then passes a 16-byte aligned d) and the bytes lie inside one entry; else byte by byte from consecutive entries, past
 * empty ones, whose base is not looked at. Reads exactly the bytes it delivers. The cursor is the thread's: the entry its last
 * unit ended in, X[lo, hi) at base (lo == hi: none yet); a unit that starts in that entry again needs no search and no load of
 * the table, which is every unit but a few when the entries are large. */
typedef struct zav_u128 { uint64_t a, b; } zav_u128_t;
typedef struct zav_cursor {
    uint64_t lo, hi, base;
    uint32_t r, rsv;
} zav_cursor_t;
ZC_FN void zav_fetch(uint8_t* d, uint32_t cnt, uint64_t x, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t e_lo, uint32_t e_hi,
                     zav_cursor_t* cur) {
    if (x < cur->lo || x >= cur->hi) {
        cur->r = zav_find(starts, e_lo, e_hi, x);
        cur->lo = starts[cur->r]; cur->hi = starts[cur->r + 1u]; cur->base = iov[cur->r].base;
    }
    uint64_t off = x - cur->lo;
    if (cnt == 16u && x + 16u <= cur->hi) {
        zav_u128_t v;
        __builtin_memcpy(&v, (const uint8_t*)(uintptr_t)cur->base + off, 16);
        __builtin_memcpy(__builtin_assume_aligned(d, 16), &v, 16);
        return;
    }
    for (uint32_t k = 0; k < cnt; k++) {
        if (cur->lo + off == cur->hi) {
            do { cur->r++; cur->lo = cur->hi; cur->hi = starts[cur->r + 1u]; } while (cur->hi == cur->lo);
            cur->base = iov[cur->r].base;
            off = 0;
        }
        d[k] = ((const uint8_t*)(uintptr_t)cur->base)[off++];
    }
}
/* Unit u of the copy X[vlo, vlo + n) -> d[0, n), d of any alignment: the bytes whose destination addresses lie in
 * [A + 16 u, A + 16 u + 16), A = d rounded down to 16. ceil(((d & 15) + n) / 16) units cover the copy. */
ZC_FN uint64_t zav_units(const uint8_t* d, uint64_t n) { return (((uint64_t)(uintptr_t)d & 15u) + n + 15u) / 16u; }
ZC_FN void zav_gather_unit(uint8_t* d, uint64_t n, uint64_t vlo, uint64_t u, const zxc_dev_iov_t* iov, const uint64_t* starts,
                           uint32_t e_lo, uint32_t e_hi, zav_cursor_t* cur) {
    const uint64_t a = (uint64_t)(uintptr_t)d & 15u, end = 16u * u + 16u;
    const uint64_t lo = 16u * u < a ? 0u : 16u * u - a, hi = end - a < n ? end - a : n; /* (end > a: u counts from the unit d lies in) */
    if (lo < hi) zav_fetch(d + lo, (uint32_t)(hi - lo), vlo + lo, iov, starts, e_lo, e_hi, cur);
}

/* ---- prep of one chunk: what thread t of the `threads` (>= ZAP_PAD) of workgroup w does. The task's range is gathered into its
 * carry area or, a whole block, left where it lies (zav_in_place) or gathered into image `at` of `images` (`image` bytes each),
 * every gathered range with ZAP_PAD zero bytes behind it; thread 0 writes the job's table entry (src_off is an address, the encode
 * launch's base is 0). The search for a unit's entry is narrowed once per workgroup to the entries [e_lo, e_hi] that meet the
 * range, and a thread owns units t, t + threads, ...: a block made of thousands of tiny entries is gathered by all threads at
 * once. `status` is the table's verdict (zav_ctl_t): after an error every job is unused (len 0: its encode wave leaves at once)
 * and neither the table nor an entry is read. starts[0 .. n_iov] is the scan's. */
ZC_FN void zav_prep(const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, const zav_chunk_t* c, uint32_t w,
                    uint32_t t, uint32_t threads, uint8_t* carry, uint8_t* next, uint8_t* images, uint32_t image, zxc_enc_job_t* jobs) {
    const zxc_enc_job_t unused = {0u, 0u, 0u};
    if (status < 0) {
        if (t == 0 && w < c->p.nb) jobs[w] = unused;
        return;
    }
    const zav_task_t k = zav_task(c, w);
    uint8_t* d = k.kind == ZAV_TO_CARRY ? carry + k.at : k.kind == ZAV_TO_NEXT ? next + k.at : images + (uint64_t)k.at * image;
    zxc_enc_job_t job = {(uint64_t)(uintptr_t)(k.kind == ZAV_BLOCK ? d : carry), c->p.block_size, 0u};
    if (k.len) {
        const uint32_t e_lo = zav_find(starts, 0u, n_iov - 1u, k.vlo);
        const uint64_t off = k.vlo - starts[e_lo], len_r = starts[e_lo + 1u] - starts[e_lo];
        if (k.kind == ZAV_BLOCK && zav_in_place(off, len_r, c->p.block_size)) {
            job.src_off = iov[e_lo].base + off;
            if (t == 0) jobs[k.job] = job;
            return;
        }
        const uint32_t e_hi = zav_find(starts, e_lo, n_iov - 1u, k.vlo + k.len - 1u);
        const uint64_t units = zav_units(d, k.len);
        zav_cursor_t cur = {0u, 0u, 0u, 0u, 0u};
        for (uint64_t u = t; u < units; u += threads) zav_gather_unit(d, k.len, k.vlo, u, iov, starts, e_lo, e_hi, &cur);
    }
    if (t < ZAP_PAD) d[k.len + t] = 0u;
    if (t == 0 && k.job != ZAV_NO_JOB) jobs[k.job] = job;
}

/* ---- the same call in a session with a dictionary of dict_size bytes (zxc_mi355x_compress_appendv_dict_device). Every block of
 * such a session is encoded from a [dict | block] image in the session's own image area (zxc_append.h), so the call's scratch
 * holds no images: the control word, starts[0 .. n_iov] and the tile words, at most
 *     8 x (n_iov + 1) + 16 x ceil(n_iov / 1024) + 4096                                              (ZAV_TILE_BYTES, ZAV_FIXED)
 * dict_size == 0 (a session without a dictionary through that call): the shape and the bound above. */
ZC_FN int zav_shape_dict(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, uint32_t dict_size, zav_shape_t* s) {
    const int rc = zav_shape(n_iov, max_piece, block_size, s);
    if (rc != 0 || dict_size == 0) return rc;
    s->image = 0;
    s->bytes = s->o_images + 256u;
    return 0;
}
ZC_FN uint64_t zav_scratch_bound_dict(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, uint32_t dict_size) {
    if (dict_size == 0) return zav_scratch_bound(n_iov, max_piece, block_size);
    return 8ull * ((uint64_t)n_iov + 1u) + ZAV_TILE_BYTES * (((uint64_t)n_iov + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS) + ZAV_FIXED;
}

/* d[0, n) = s[0, n), both of any alignment: thread t of `threads` moves the 16 bytes at 16 t, 16 (t + threads), ... */
ZC_FN void zav_copy(uint8_t* d, const uint8_t* s, uint32_t n, uint32_t t, uint32_t threads) {
    for (uint32_t o = 16u * t; o < n; o += 16u * threads) {
        if (o + 16u <= n) {
            zav_u128_t v;
            __builtin_memcpy(&v, s + o, 16);
            __builtin_memcpy(d + o, &v, 16);
        } else {
            for (uint32_t k = o; k < n; k++) d[k] = s[k];
        }
    }
}
/* d[0, n) = X[vlo, vlo + n), d of any alignment: the workgroup's share of thread t. The search is narrowed once to the entries
 * [e_lo, e_hi] that meet the range; the thread owns units t, t + threads, ... (zav_gather_unit). Reads exactly those bytes. */
ZC_FN void zav_gather(uint8_t* d, uint64_t n, uint64_t vlo, const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, uint32_t t,
                      uint32_t threads) {
    if (!n) return;
    const uint32_t e_lo = zav_find(starts, 0u, n_iov - 1u, vlo), e_hi = zav_find(starts, e_lo, n_iov - 1u, vlo + n - 1u);
    const uint64_t units = zav_units(d, n);
    zav_cursor_t cur = {0u, 0u, 0u, 0u, 0u};
    for (uint64_t u = t; u < units; u += threads) zav_gather_unit(d, n, vlo, u, iov, starts, e_lo, e_hi, &cur);
}

/* Prep of the jobs [j0, j0 + n) of a chunk that completes blocks (c->p is zap_plan_piece_images', nb > 0), which the encoder takes
 * in one launch over the session's image area: what thread t of the `threads` (>= ZAP_PAD) of workgroup w does. Workgroup w < n
 * builds image w at images + w x (block_size + dict_size): the dictionary, then the bytes of job j0 + w from the one or two places
 * zap_job_images names, its ZAP_SRC segment being X[c->v + off, + len) gathered straight into the image (the carried block: the
 * waiting bytes of `carry`, then the head of X, which is copied nowhere else); thread 0 writes the job's table entry, the image's
 * offset from `images`. Workgroup n, which only the first launch of a chunk has (j0 == 0), gathers the tail into the other carry
 * area with ZAP_PAD zero bytes behind it. No block is encoded where it lies: an image is a copy by construction, and its over-read
 * is served by the next image or by ZC_IMAGE_PAD. After a table error (status < 0) every job is unused and nothing else is read
 * or written: not the table, not an entry, not starts. */
ZC_FN void zav_prep_images(const zxc_dev_iov_t* iov, const uint64_t* starts, uint32_t n_iov, int status, const zav_chunk_t* c, uint32_t j0,
                           uint32_t n, uint32_t w, uint32_t t, uint32_t threads, const uint8_t* dict, uint32_t dict_size,
                           const uint8_t* carry, uint8_t* next, uint8_t* images, zxc_enc_job_t* jobs) {
    const zap_piece_t* p = &c->p;
    if (status < 0) {
        const zxc_enc_job_t unused = {0u, 0u, 0u};
        if (t == 0 && w < n) jobs[j0 + w] = unused;
        return;
    }
    if (w >= n) {
        if (w == n && j0 == 0 && p->cp[2].area == ZAP_NEXT) {
            uint8_t* d = next + p->cp[2].at;
            zav_gather(d, p->tail, c->v + p->n - p->tail, iov, starts, n_iov, t, threads);
            if (t < ZAP_PAD) d[p->tail + t] = 0u;
        }
        return;
    }
    const zap_src2_t s = zap_job_images(p, j0 + w);
    const uint64_t at = (uint64_t)w * ((uint64_t)p->block_size + dict_size);
    uint8_t* d = images + at;
    zav_copy(d, dict, dict_size, t, threads);
    d += dict_size;
    for (uint32_t k = 0; k < 2u; k++) {
        const zap_src_t g = s.seg[k];
        if (g.area == ZAP_CARRY) zav_copy(d, carry + g.off, g.len, t, threads);
        else zav_gather(d, g.len, c->v + g.off, iov, starts, n_iov, t, threads);
        d += g.len;
    }
    if (t == 0) {
        const zxc_enc_job_t job = {at, s.seg[0].len + s.seg[1].len, 0u};
        jobs[j0 + w] = job;
    }
}
#endif
