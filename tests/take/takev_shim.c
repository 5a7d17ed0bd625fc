/* Test-only view of zxc_amd/csrc/zxc_takev.h for tests/test_decompress_takev_device_cpu.py: the scratch's shape and stated bound,
 * the table's verdict (in series, in any tile grouping, folded into a control word), the in-place rule against a plain walk over
 * the entries, and whole sessions that mix take and takev replayed on the host (takev_replay.h on top of take_replay.h: exactly
 * the functions the entry points and kernels of zxc_take_device.hip call). */
#include <stddef.h>

#include "takev_replay.h"

size_t tv_shape_size(void) { return sizeof(ztv_shape_t); }
size_t tv_place_size(void) { return sizeof(ztv_place_t); }
int tv_shape(uint32_t n_iov, uint64_t max_piece, uint32_t block_size, ztv_shape_t* s) { return ztv_shape(n_iov, max_piece, block_size, s); }
uint64_t tv_scratch_bound(uint32_t n_iov, uint64_t max_piece, uint32_t block_size) { return ztv_scratch_bound(n_iov, max_piece, block_size); }
int tv_scan_serial(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint64_t* starts) { return ztv_scan_serial(iov, n_iov, total, starts); }
/* the verdict with the entries reduced in tiles of `group` entries first, as the three tile passes do */
int tv_scan_grouped(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t total, uint32_t group) {
    uint64_t all = 0;
    uint32_t flags = 0;
    for (uint32_t t = 0; t < n_iov; t += group) {
        uint64_t sum = 0;
        for (uint32_t r = t; r < n_iov && r < t + group; r++) {
            flags |= zav_entry_flags(iov[r].base, iov[r].len, total);
            sum = zav_sat_add(sum, iov[r].len);
        }
        all = zav_sat_add(all, sum);
    }
    return ztv_table_status(flags, all, total);
}
/* the fold into a control word that starts with these two fields: -> head_result, *final_out */
int64_t tv_fold(uint32_t final, int64_t head_result, int verdict, uint32_t* final_out) {
    zc_ctl_t c;
    memset(&c, 0, sizeof c);
    c.final = final; c.head_result = head_result;
    ztv_fold(&c, verdict);
    *final_out = c.final;
    return c.head_result;
}
uint64_t tv_rule_check(const zxc_dev_iov_t* iov, uint32_t n_iov, uint64_t pos, uint64_t max_piece, uint32_t bs) {
    return tvr_rule_check(iov, n_iov, pos, max_piece, bs);
}
int64_t tv_session(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, int want_verify, int use_table,
                   int have_dict, uint32_t dict_id, const uint8_t* blk_bytes, const uint64_t* blk_at, const int32_t* blk_status,
                   uint32_t n_blocks, const uint64_t* lens, const uint32_t* calls, uint32_t n_calls, uint32_t align, uint8_t* out) {
    return tvr_session(src, src_size, cap, max_piece, bs, want_verify, use_table, have_dict, dict_id, blk_bytes, blk_at, blk_status, n_blocks,
                       lens, calls, n_calls, align, out);
}
/* a session of takev calls in which call `bad_call` gets a table in error (kind 1: a zero base with a length; 2: an entry longer
 * than total; 3: a sum above total; 4: a sum below it): -> the result word; written[0] = 1 when any byte of that call's entries
 * changed, written[1] = 1 when an earlier call's bytes are not the expected ones */
int64_t tv_session_bad_table(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, const uint8_t* blk_bytes,
                             const uint64_t* blk_at, const int32_t* blk_status, uint32_t n_blocks, const uint64_t* lens, uint32_t n_lens,
                             uint32_t per_call, uint32_t bad_call, int kind, const uint8_t* expect, uint32_t* written) {
    tr_session_t s;
    memset(&s, 0, sizeof s);
    s.blk_bytes = blk_bytes; s.blk_at = blk_at; s.blk_status = blk_status; s.n_blocks = n_blocks;
    const int rc = tr_begin(&s, src, src_size, cap, max_piece, bs, 0, 1, 0, 0u);
    if (rc != 0) return rc;
    uint64_t at = 0;
    written[0] = written[1] = 0;
    for (uint32_t e = 0, call = 0; e < n_lens; e += per_call, call++) {
        const uint32_t cnt = n_lens - e < per_call ? n_lens - e : per_call;
        zxc_dev_iov_t* iov = malloc(((size_t)cnt + 1u) * sizeof *iov);
        uint8_t** buf = malloc(((size_t)cnt + 1u) * sizeof *buf);
        uint64_t total = 0;
        for (uint32_t r = 0; r < cnt; r++) {
            buf[r] = malloc(lens[e + r] + 1u);
            memset(buf[r], TR_CANARY, lens[e + r] + 1u);
            iov[r].base = (uint64_t)(uintptr_t)buf[r]; iov[r].len = lens[e + r];
            total += lens[e + r];
        }
        uint64_t promised = total;
        if (call == bad_call) {
            uint32_t r = 0;
            while (r + 1u < cnt && iov[r].len == 0) r++;
            if (kind == 1) iov[r].base = 0;              /* (len > 0: the test's tables keep a non-empty entry in every call) */
            else if (kind == 2) iov[r].len = total + 1u; /* never dereferenced: after the error no entry is touched */
            else if (kind == 3) promised = total - 1u;
            else promised = total + 1u;
            if (promised > s.cap - s.pos) promised = s.cap - s.pos;
        }
        if (promised <= s.cap - s.pos && tvr_takev(&s, iov, cnt, promised) != ZXC_OK) s.bad = 1; /* (a call that no longer fits is left out) */
        for (uint32_t r = 0; r < cnt; r++) {
            const uint64_t n = lens[e + r];
            if (call == bad_call) { for (uint64_t b = 0; b <= n; b++) if (buf[r][b] != TR_CANARY) written[0] = 1; }
            else if (call < bad_call && memcmp(buf[r], expect + at, n) != 0) written[1] = 1;
            at += n;
            free(buf[r]);
        }
        free(buf); free(iov);
    }
    if (s.pos < cap) { /* the session is still taken to the capacity */
        uint8_t* rest = malloc(cap - s.pos + 1u);
        if (tr_take(&s, rest, cap - s.pos) != ZXC_OK) s.bad = 1;
        free(rest);
    }
    const int64_t r = tr_end(&s);
    tr_free(&s);
    return r;
}
/* what the head stage decides for these bytes: -> file_ck | verify << 1 | final << 2 */
uint32_t tv_head(const uint8_t* src, uint64_t src_size, uint64_t cap, uint32_t bs, int want_verify) {
    zc_ctl_t c;
    zc_head(src, src_size, cap, bs, want_verify, 1u, &c);
    return c.file_ck | c.verify << 1 | c.final << 2;
}
/* (take_replay.h's own checks, kept referenced: the header's functions are static) */
int tv_plan_check(uint64_t pos, uint64_t n, uint64_t room, uint32_t align, uint32_t bs, uint64_t max_piece) {
    return tr_plan_check(pos, n, room, align, bs, max_piece);
}
int64_t tv_take_session(const uint8_t* src, uint64_t src_size, uint64_t cap, uint64_t max_piece, uint32_t bs, const uint8_t* blk_bytes,
                        const uint64_t* blk_at, const int32_t* blk_status, uint32_t n_blocks, const uint64_t* lens, uint32_t n_lens, uint8_t* out) {
    return tr_session(src, src_size, cap, max_piece, bs, 0, 1, 0, 0u, blk_bytes, blk_at, blk_status, n_blocks, lens, n_lens, 0u, out);
}
