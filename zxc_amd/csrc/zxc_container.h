/* zxc_container.h — the v8 container, once: constants, little-endian reads and stores, header check bytes, the file header
 * and the block header read and written, the footer, the seek-table rules, the block chain, the header walk and the verdict's
 * precedence. Plain inline C that hipcc and a host C compiler both take: the host API (zxc_host.c and the files included into
 * it), the kernels of the device-to-device calls and the CPU tests run the same lines, so "what zxc_decompress / zxc_compress
 * does for the same bytes" holds by construction. Where a device call departs from the host API, the function says so.
 * Nothing here writes through a pointer it was not given, and every read lies inside src[0, src_size). */
#ifndef ZXC_CONTAINER_H
#define ZXC_CONTAINER_H
#include <stdint.h>

#include "../../include/zxc_error.h"
#include "../../include/zxc_mi355x.h" /* zxc_dev_job_t */

#ifdef __HIPCC__
#define ZC_FN __host__ __device__ static inline
#else
#define ZC_FN static inline
#endif

#define ZC_MAGIC 0x9CB02EF5u
#define ZC_VERSION 8u
#define ZC_FILE_HDR 16u
#define ZC_BLK_HDR 8u
#define ZC_FOOTER 12u
#define ZC_BLK_SEK 254u
#define ZC_BLK_EOF 255u
#define ZC_TILE_BLOCKS 1024u          /* blocks per tile of the seek-table and verdict passes */
#define ZC_SEEK_ENTRY_MAX (1u << 22)  /* a seek entry above this sends the archive to the walk (keeps a wave's sum in 32 bits) */
#define ZC_STAGED_MAX 3u              /* blocks decoded into the work area: at most two slots that pass the capacity, and block n_max */
#define ZC_NO_EVENT (~0ull)
#define ZC_DICT_MAX 65535u            /* bytes of a dictionary (zxc_dev_dict_t.size) */

/* The dictionary compress calls encode from [dict | block] images, in chunks that reuse one image area in stream order: */
#define ZC_IMAGE_BYTES (256ull << 20) /* the image area of a chunk stays near this ... */
#define ZC_IMAGE_MIN_BLOCKS 4096u     /* ... but a chunk is never fewer blocks than this */
#define ZC_IMAGE_PAD 64u              /* behind the last image (the encoder's over-read, as zxc_mi355x_encode_dict_work_size) */

/* Per-call state at the start of the work area. */
typedef struct zc_ctl {
    int64_t head_result;  /* final != 0: the call's result, decided by the head stage (file-header error, empty-frame probe) */
    uint64_t total;       /* footer: decoded size */
    uint64_t eof_at;      /* seek path: offset of the EOF block header */
    unsigned long long event; /* min over the blocks found of (index << 32 | code): the first block that ends the call */
    uint32_t final;
    uint32_t file_ck;     /* the archive carries per-block checksums */
    uint32_t verify;      /* ... and the caller wants them checked */
    uint32_t sel;         /* job / status table in use: 1 = the one decoded with verify_trailer = 1 */
    uint32_t stored_hash; /* footer: global hash */
    uint32_t nb;          /* ceil(total / block_size), saturated */
    uint32_t seek;        /* 0 no usable table, 1 probe passed, 2 the entries sum to the EOF block, 3 every block header agrees */
    uint32_t found;       /* blocks in the job table */
    uint32_t done;        /* the chain ended (EOF, bad header, end of bytes) rather than at the job limit */
    uint32_t saw_eof;
    int32_t tail_err;     /* error of the walk, reported only when every block found decodes */
    uint32_t ghash;       /* rotl1-xor fold of the stored per-block checksums */
} zc_ctl_t;

ZC_FN uint32_t zc_rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
ZC_FN uint64_t zc_rd64(const uint8_t* p) { return (uint64_t)zc_rd32(p) | ((uint64_t)zc_rd32(p + 4) << 32); }
ZC_FN uint32_t zc_rotl(uint32_t x, uint32_t r) { return r ? (x << r) | (x >> (32u - r)) : x; }
/* the low n bytes of v, little-endian */
ZC_FN void zc_st_le(uint8_t* p, uint64_t v, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8u * i));
}
/* the global hash over the stored per-block checksums, one trailer at a time in stream order */
ZC_FN uint32_t zc_hash_fold(uint32_t h, uint32_t trailer) { return zc_rotl(h, 1) ^ trailer; }

/* header check bytes (xorshift of the little-endian words; the functions mask the check bytes out themselves) */
ZC_FN uint64_t zc_xs_mix(uint64_t h) {
    h ^= h << 13;
    h ^= h >> 7;
    h ^= h << 17;
    return h;
}
ZC_FN uint8_t zc_hdr_hash8(uint64_t w) {
    const uint64_t h = zc_xs_mix((w & 0x00FFFFFFFFFFFFFFull) ^ 0x9E3779B97F4A7C15ull);
    return (uint8_t)((h >> 32) ^ h);
}
ZC_FN uint16_t zc_hdr_hash16(uint64_t lo, uint64_t hi) {
    const uint64_t h = zc_xs_mix(lo ^ (hi & 0x0000FFFFFFFFFFFFull) ^ 0xD2D84A61D2D84A61ull);
    const uint32_t r = (uint32_t)((h >> 32) ^ h);
    return (uint16_t)((r >> 16) ^ r);
}
/* A block header as one little-endian word: type in byte 0, payload size in bytes 3..6, check byte in byte 7. */
ZC_FN int zc_blk_hdr_ok(uint64_t w) { return (uint8_t)(w >> 56) == zc_hdr_hash8(w); }
ZC_FN uint32_t zc_blk_type(uint64_t w) { return (uint32_t)(w & 0xFFu); }
ZC_FN uint32_t zc_blk_csz(uint64_t w) { return (uint32_t)(w >> 24); }
/* ... and the word of a header with that type and payload size, check byte included */
ZC_FN uint64_t zc_blk_hdr(uint32_t type, uint32_t csz) {
    const uint64_t w = (uint64_t)type | (uint64_t)csz << 24;
    return w | (uint64_t)zc_hdr_hash8(w) << 56;
}
/* blocks per chunk of the dictionary compress calls */
ZC_FN uint64_t zc_image_chunk(uint32_t block_size, uint32_t dict_size) {
    const uint64_t c = ZC_IMAGE_BYTES / ((uint64_t)block_size + dict_size);
    return c > ZC_IMAGE_MIN_BLOCKS ? c : ZC_IMAGE_MIN_BLOCKS;
}
/* a block size the format has: a power of two from 4 KiB to 2 MiB */
ZC_FN int zc_block_size_ok(uint64_t bs) { return bs >= (1u << 12) && bs <= (1u << 21) && !(bs & (bs - 1u)); }
ZC_FN uint32_t zc_block_size_lg(uint64_t bs) { /* of a size zc_block_size_ok accepts */
    uint32_t lg = 12;
    while ((1ull << lg) < bs) lg++;
    return lg;
}
/* A seek table is the last thing in front of the footer: [EOF header][SEK header][4 nb bytes][footer], at least the file header
 * in front. -> 1 when both headers are valid, of their types, and the SEK header's size is 4 nb; then *eof_at is the EOF header's
 * offset and *eof its word (whose size field is the caller's to judge). */
ZC_FN int zc_seek_tail(const uint8_t* src, uint64_t src_size, uint64_t nb, uint64_t* eof_at, uint64_t* eof) {
    if (ZC_FILE_HDR + 2u * ZC_BLK_HDR + 4u * nb + ZC_FOOTER > src_size) return 0;
    const uint64_t sek_at = src_size - ZC_FOOTER - 4u * nb - ZC_BLK_HDR, at = sek_at - ZC_BLK_HDR;
    const uint64_t sek = zc_rd64(src + sek_at), w = zc_rd64(src + at);
    if (!zc_blk_hdr_ok(sek) || zc_blk_type(sek) != ZC_BLK_SEK || zc_blk_csz(sek) != 4u * nb) return 0;
    if (!zc_blk_hdr_ok(w) || zc_blk_type(w) != ZC_BLK_EOF) return 0;
    *eof_at = at;
    *eof = w;
    return 1;
}

/* The file header over its 16 bytes: magic, version, log2 of the block size, flags (0x80 per-block checksums, 0x40 a dictionary
 * id in bytes 7..10, low nibble zero), zeros, two check bytes. -> ZXC_OK or the error; block-size log2, checksum flag, dictionary id. */
ZC_FN int zc_file_header(const uint8_t* h, uint32_t* lg, uint32_t* file_ck, uint32_t* dict_id) {
    if (zc_rd32(h) != ZC_MAGIC) return ZXC_ERROR_BAD_MAGIC;
    if (h[4] != ZC_VERSION) return ZXC_ERROR_BAD_VERSION;
    if ((uint16_t)(h[14] | (h[15] << 8)) != zc_hdr_hash16(zc_rd64(h), zc_rd64(h + 8)) || (h[6] & 0x0Fu) != 0) return ZXC_ERROR_BAD_HEADER;
    if (h[5] < 12u || h[5] > 21u) return ZXC_ERROR_BAD_BLOCK_SIZE;
    *lg = h[5];
    *file_ck = (h[6] & 0x80u) ? 1u : 0u;
    *dict_id = (h[6] & 0x40u) ? zc_rd32(h + 7) : 0u;
    return ZXC_OK;
}
/* ... and the two little-endian words of the header with these fields, check bytes included (dict_id counts only with has_dict) */
ZC_FN void zc_file_header_words(uint32_t lg, int file_ck, int has_dict, uint32_t dict_id, uint64_t* lo, uint64_t* hi) {
    const uint64_t flags = (file_ck ? 0x80u : 0u) | (has_dict ? 0x40u : 0u), id = has_dict ? dict_id : 0u;
    *lo = (uint64_t)ZC_MAGIC | (uint64_t)ZC_VERSION << 32 | (uint64_t)lg << 40 | flags << 48 | (id & 0xFFu) << 56;
    *hi = id >> 8;
    *hi |= (uint64_t)zc_hdr_hash16(*lo, *hi) << 48;
}
ZC_FN void zc_put_file_header(uint8_t* p, uint32_t lg, int file_ck, int has_dict, uint32_t dict_id) {
    uint64_t lo, hi;
    zc_file_header_words(lg, file_ck, has_dict, dict_id, &lo, &hi);
    zc_st_le(p, lo, 8);
    zc_st_le(p + 8, hi, 8);
}
/* the footer's 12 bytes: decoded size, global hash (the caller's 0 without checksums) */
ZC_FN void zc_put_footer(uint8_t* p, uint64_t total, uint32_t hash) {
    zc_st_le(p, total, 8);
    zc_st_le(p + 8, hash, 4);
}

/* What an archive of nb blocks needs whatever the encoder writes: header, the smallest block per block, EOF, seek table, footer. */
ZC_FN uint64_t zc_known_size(uint64_t nb, int file_ck, int seekable) {
    return ZC_FILE_HDR + nb * (ZC_BLK_HDR + (file_ck ? 4u : 0u)) + ZC_BLK_HDR + ((seekable && nb) ? ZC_BLK_HDR + 4u * nb : 0u) + ZC_FOOTER;
}

/* Block i of the archive: compressed bytes at comp_off, decoded into slot i of the destination while i < k_direct, else into
 * slot i - k_direct of the staged area (the k split of the caller). out_len is a whole block, as frame_source of zxc_host.c has it. */
ZC_FN zxc_dev_job_t zc_job(uint64_t comp_off, uint32_t i, uint32_t comp_size, uint32_t block_size, uint32_t k_direct) {
    zxc_dev_job_t j;
    j.comp_off = comp_off;
    j.out_off = (uint64_t)(i < k_direct ? i : i - k_direct) * block_size;
    j.comp_size = comp_size;
    j.out_len = block_size;
    return j;
}

/* ---- head: file header, footer, seek-table probe. src_size >= 28. n_jobs = ceil(dst_capacity / block_size) + 1.
 * have_dict / dict_id: the caller's dictionary and its zxc_dict_id. A header with a dictionary id wants one, and that one
 * (zxc_decompress, "zxc_dispatch.c:883-892"): DICT_REQUIRED without, DICT_MISMATCH with another; a dictionary given for a header
 * without an id is not looked at here. */
ZC_FN void zc_head_dict(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint32_t n_jobs,
                        zc_ctl_t* c, int have_dict, uint32_t have_id) {
    const uint8_t* foot = src + src_size - ZC_FOOTER;
    uint32_t lg = 0, dict_id = 0;
    c->head_result = 0; c->total = zc_rd64(foot); c->eof_at = 0; c->event = ZC_NO_EVENT; c->final = 0; c->file_ck = 0; c->verify = 0;
    c->sel = 0; c->stored_hash = zc_rd32(foot + 8); c->nb = 0; c->seek = 0; c->found = 0; c->done = 0; c->saw_eof = 0; c->tail_err = 0;
    c->ghash = 0;
    if (dst_capacity == 0) { /* the empty-frame probe of zxc_decompress */
        c->final = 1;
        c->head_result = zc_rd32(src) != ZC_MAGIC ? (int64_t)ZXC_ERROR_BAD_MAGIC : c->total == 0 ? 0 : (int64_t)ZXC_ERROR_DST_TOO_SMALL;
        return;
    }
    int rc = zc_file_header(src, &lg, &c->file_ck, &dict_id);
    if (rc == ZXC_OK && (1u << lg) != block_size) rc = ZXC_ERROR_BAD_BLOCK_SIZE; /* departure: the grids were sized by the argument */
    if (rc == ZXC_OK && dict_id != 0) {
        if (!have_dict) rc = ZXC_ERROR_DICT_REQUIRED;
        else if (have_id != dict_id) rc = ZXC_ERROR_DICT_MISMATCH;
    }
    if (rc != ZXC_OK) { c->final = 1; c->head_result = rc; return; }
    c->verify = (c->file_ck && want_verify) ? 1u : 0u;
    c->sel = c->verify;
    const uint64_t nb = c->total / block_size + (c->total % block_size != 0);
    c->nb = nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nb;
    uint64_t eof_at = 0, eof = 0;
    if (nb == 0 || nb > n_jobs || !zc_seek_tail(src, src_size, nb, &eof_at, &eof) || zc_blk_csz(eof) != 0) return;
    c->eof_at = eof_at;
    c->seek = 1;
}
/* the head of the call that takes no dictionary */
ZC_FN void zc_head(const uint8_t* src, uint64_t src_size, uint64_t dst_capacity, uint32_t block_size, int want_verify, uint32_t n_jobs,
                   zc_ctl_t* c) {
    zc_head_dict(src, src_size, dst_capacity, block_size, want_verify, n_jobs, c, 0, 0u);
}

/* ---- seek-table path. Entry i is block i's physical size. If every entry is plausible, the entries sum from offset 16 to the EOF
 * block, and the block header at every prefix sum is valid, is no EOF block and has 8 + csz (+4) == entry, then by induction from
 * offset 16 the table's chain is the chain the walk below follows, and the walk would end at that EOF block with no error. */
ZC_FN int zc_seek_entry_ok(uint32_t entry, uint32_t file_ck) { return entry >= ZC_BLK_HDR + 4u * file_ck && entry <= ZC_SEEK_ENTRY_MAX; }
ZC_FN const uint8_t* zc_seek_entries(const uint8_t* src, const zc_ctl_t* c) { return src + c->eof_at + 2u * ZC_BLK_HDR; }
ZC_FN int zc_seek_block_ok(const uint8_t* src, uint64_t off, uint32_t entry, uint32_t file_ck) {
    const uint64_t w = zc_rd64(src + off);
    return zc_blk_hdr_ok(w) && zc_blk_type(w) != ZC_BLK_EOF && (uint64_t)ZC_BLK_HDR + zc_blk_csz(w) + 4u * file_ck == entry;
}
/* block i's part of the global hash: h = rotl(h, 1) ^ t_i folded from 0 over nb trailers is XOR_i rotl(t_i, (nb - 1 - i) mod 32) */
ZC_FN uint32_t zc_hash_term(const uint8_t* src, uint64_t off, uint32_t entry, uint32_t nb, uint32_t i) {
    return zc_rotl(zc_rd32(src + off + entry - 4u), (nb - 1u - i) & 31u);
}
ZC_FN void zc_chain_from_table(zc_ctl_t* c, uint32_t ghash) {
    c->seek = 3; c->found = c->nb; c->done = 1; c->saw_eof = 1; c->tail_err = 0; c->ghash = ghash;
}
/* The three parallel passes in series (tests; the kernels run the same element functions over tiles). -> 1 when the table was used */
ZC_FN int zc_seek_plan(const uint8_t* src, uint32_t block_size, uint32_t k_direct, zc_ctl_t* c, zxc_dev_job_t* jobs) {
    if (c->final || c->seek != 1) return 0;
    const uint8_t* ent = zc_seek_entries(src, c);
    uint64_t sum = 0;
    for (uint32_t i = 0; i < c->nb; i++) {
        const uint32_t e = zc_rd32(ent + 4u * i);
        if (!zc_seek_entry_ok(e, c->file_ck)) { c->seek = 0; return 0; }
        sum += e;
    }
    if (ZC_FILE_HDR + sum != c->eof_at) { c->seek = 0; return 0; }
    c->seek = 2;
    uint64_t off = ZC_FILE_HDR;
    uint32_t h = 0, bad = 0;
    for (uint32_t i = 0; i < c->nb; i++) {
        const uint32_t e = zc_rd32(ent + 4u * i);
        if (!zc_seek_block_ok(src, off, e, c->file_ck)) bad = 1;
        else if (c->verify) h ^= zc_hash_term(src, off, e, c->nb, i);
        jobs[i] = zc_job(off, i, e, block_size, k_direct);
        off += e;
    }
    if (bad) return 0; /* (seek stays 2: the walk clears the table first) */
    zc_chain_from_table(c, h);
    return 1;
}

/* ---- the block chain, as zxc_decompress (frame_source of zxc_host.c) and zc_walk below follow it from offset 16 */
typedef struct zc_chain {
    uint64_t ip;       /* offset of the next block header */
    uint32_t ghash;    /* fold of the trailers of the whole blocks passed (verify only) */
    uint32_t done;     /* the chain ended: EOF block, bad header or end of the bytes */
    uint32_t saw_eof;
    int32_t tail_err;  /* error of the chain itself, reported only when every block in front of it decodes */
} zc_chain_t;
/* One block. -> 0 when the chain ends at c->ip without one: at the end of the bytes, at a header that is cut or fails its check
 * byte (BAD_HEADER), or at an EOF block (which must carry size 0, else BAD_HEADER). Else the block at c->ip is a job of the
 * returned size: its physical 8 + csz (+4) bytes clamped to the bytes left and to 32 bits (the decoder sees "all remaining
 * bytes"; any size >= the physical block is equivalent); its trailer is folded only when the block lies whole inside the
 * bytes, and c->ip moves behind it, or to src_size with done set when the block reaches the end. */
ZC_FN uint32_t zc_chain_next(const uint8_t* src, uint64_t src_size, uint32_t file_ck, uint32_t verify, zc_chain_t* c) {
    if (c->ip >= src_size) { c->done = 1; return 0; }
    const uint64_t rem = src_size - c->ip, w = rem < ZC_BLK_HDR ? 0u : zc_rd64(src + c->ip);
    if (rem < ZC_BLK_HDR || !zc_blk_hdr_ok(w)) { c->tail_err = ZXC_ERROR_BAD_HEADER; c->done = 1; return 0; }
    if (zc_blk_type(w) == ZC_BLK_EOF) {
        if (zc_blk_csz(w) != 0) c->tail_err = ZXC_ERROR_BAD_HEADER;
        c->saw_eof = 1;
        c->done = 1;
        return 0;
    }
    const uint64_t phys = (uint64_t)ZC_BLK_HDR + zc_blk_csz(w) + (file_ck ? 4u : 0u), cs = phys < rem ? phys : rem;
    if (verify && phys <= rem) c->ghash = zc_hash_fold(c->ghash, zc_rd32(src + c->ip + ZC_BLK_HDR + zc_blk_csz(w)));
    if (phys >= rem) { c->ip = src_size; c->done = 1; }
    else c->ip += phys;
    return cs > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cs;
}

/* ---- walk: the chain from offset 16, for at most n_jobs blocks. Jobs behind the blocks found are left as they are
 * (the caller zeroed them: comp_size 0 is answered with an error status and nothing is read). */
ZC_FN void zc_walk(const uint8_t* src, uint64_t src_size, uint32_t block_size, uint32_t k_direct, uint32_t n_jobs, zc_ctl_t* c,
                   zxc_dev_job_t* jobs) {
    zc_chain_t ch = {ZC_FILE_HDR, 0, 0, 0, 0};
    uint32_t n = 0;
    while (n < n_jobs) {
        const uint64_t at = ch.ip;
        const uint32_t cs = zc_chain_next(src, src_size, c->file_ck, c->verify, &ch);
        if (cs) { jobs[n] = zc_job(at, n, cs, block_size, k_direct); n++; }
        if (ch.done) break;
    }
    c->found = n; c->done = ch.done; c->saw_eof = ch.saw_eof; c->tail_err = ch.tail_err; c->ghash = ch.ghash;
}

/* ---- verdict. What block i's status means for the call, given that no earlier block has an event (so every earlier block decoded
 * to exactly block_size and block i starts at i * block_size): 0 nothing, else the call's error. In zxc_decompress's order: the
 * block's own error, then the capacity, then regularity (departure: an irregular frame has no host to fall back to). */
ZC_FN int32_t zc_block_event(uint32_t i, int32_t status, uint32_t found, uint32_t done, uint32_t block_size, uint64_t dst_capacity) {
    if (status < 0) return status;
    const uint64_t at = (uint64_t)i * block_size;
    if (at > dst_capacity || (uint64_t)status > dst_capacity - at) return ZXC_ERROR_DST_TOO_SMALL;
    const int last = done && i + 1u == found;
    if (((uint32_t)status != block_size && !last) || (uint32_t)status > block_size) return ZXC_ERROR_GPU_UNSUPPORTED;
    return 0;
}
ZC_FN unsigned long long zc_event_key(uint32_t i, int32_t code) { return ((unsigned long long)i << 32) | (uint32_t)code; }

/* The call's result from the control word and the last found block's status: first event, then the walk's pending error, then
 * the footer's size, then the global hash. */
ZC_FN int64_t zc_verdict(const zc_ctl_t* c, int32_t last_status, uint32_t block_size) {
    if (c->final) return c->head_result;
    if (c->event != ZC_NO_EVENT) return (int64_t)(int32_t)(uint32_t)c->event;
    if (!c->done) return ZXC_ERROR_DST_TOO_SMALL; /* (more whole blocks than the capacity holds always raise an event) */
    const uint64_t total = c->found ? (uint64_t)(c->found - 1u) * block_size + (uint32_t)last_status : 0u;
    if (c->tail_err) return c->tail_err;
    if (c->saw_eof) {
        if (c->total != total) return ZXC_ERROR_CORRUPT_DATA;
        if (c->verify && c->stored_hash != c->ghash) return ZXC_ERROR_BAD_CHECKSUM;
    }
    return (int64_t)total;
}
/* bytes of staged block i (slot i - k_direct) that belong in the destination */
ZC_FN uint32_t zc_tail_bytes(uint32_t i, int32_t status, uint32_t block_size, uint64_t dst_capacity) {
    const uint64_t at = (uint64_t)i * block_size;
    if (status <= 0 || at >= dst_capacity) return 0;
    uint64_t n = (uint32_t)status < block_size ? (uint32_t)status : block_size;
    if (n > dst_capacity - at) n = dst_capacity - at;
    return (uint32_t)n;
}

/* ---- the call's shape, known to the host before any byte of the archive */
typedef struct zc_shape {
    uint32_t n_jobs, k_direct, n_tiles;
    uint64_t o_tile_sum, o_tile_hash, o_tile_bad, o_jobs, o_status, o_stage, bytes; /* work-area offsets from its 256-byte aligned base */
} zc_shape_t;
ZC_FN uint64_t zc_round_up(uint64_t x, uint64_t a) { return (x + a - 1u) / a * a; }
/* -> 0, or ZXC_ERROR_BAD_BLOCK_SIZE (block size, or more blocks than a launch counts) */
ZC_FN int zc_shape(uint64_t dst_capacity, uint32_t block_size, zc_shape_t* s) {
    if (!zc_block_size_ok(block_size)) return ZXC_ERROR_BAD_BLOCK_SIZE;
    const uint64_t n_max = dst_capacity / block_size + (dst_capacity % block_size != 0);
    if (n_max + 1u > 0x7FFFFFFFull) return ZXC_ERROR_BAD_BLOCK_SIZE;
    s->n_jobs = (uint32_t)n_max + 1u;
    /* slot i takes [i bs, (i + 1) bs + 32) of the destination (the decoders store 16 bytes at a time): inside the capacity for i < k */
    const uint64_t k = dst_capacity >= 32u ? (dst_capacity - 32u) / block_size : 0u;
    s->k_direct = k < s->n_jobs ? (uint32_t)k : s->n_jobs;
    s->n_tiles = (s->n_jobs + ZC_TILE_BLOCKS - 1u) / ZC_TILE_BLOCKS;
    uint64_t o = 256u; /* zc_ctl_t */
    s->o_tile_sum = o;  o = zc_round_up(o + 8ull * s->n_tiles, 256u);
    s->o_tile_hash = o; o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_tile_bad = o;  o = zc_round_up(o + 4ull * s->n_tiles, 256u);
    s->o_jobs = o;      o = zc_round_up(o + 2ull * s->n_jobs * sizeof(zxc_dev_job_t), 256u); /* two tables: see zc_ctl_t.sel */
    s->o_status = o;    o = zc_round_up(o + 2ull * s->n_jobs * 4u, 256u);
    s->o_stage = o;     o += (uint64_t)ZC_STAGED_MAX * block_size + 64u;
    s->bytes = o + 256u; /* (the caller's d_work may have any alignment) */
    return 0;
}
#endif
