/* zxc_dev.h — types shared by the HIP kernels and the host-side C-ABI shim. */
#ifndef ZXC_DEV_H
#define ZXC_DEV_H
#include "../../include/zxc_mi355x.h" /* zxc_dev_job_t */

/* Device-side status that is not a reference zxc_error_t value: the block is valid
 * but uses a section coding this kernel cannot decode yet (maps to
 * ZXC_ERROR_GPU_UNSUPPORTED on the host; never a silent CPU fallback). */
#define ZXC_DEV_E_UNSUPPORTED (-101)
#define ZXC_DEV_DEFER (-103)      /* lean kernel only, never stored: the block goes to the full kernel's list */
#define ZXC_DEV_E_INTERNAL (-102) /* kernel self-check tripped (a bug, never an input property) */

/* One workgroup's input of the job-table encode entries (zxc_encode_jobs_kernel_*, zxc_encode_kernel.hip): len bytes, at most a
 * block, at the launch's base pointer + src_off (with a dictionary: a [dict | block] image there). len 0: an unused job. */
typedef struct zxc_enc_job {
    uint64_t src_off;
    uint32_t len;
    uint32_t pad;
} zxc_enc_job_t;

/* Levels 6-7, launches without a dictionary: the launch-order pass (zxc_order_scatter_kernel) sorts every block into one
 * of three classes. The PivCo sections of PRE blocks are decoded by the workgroup section kernels (zxc_pivco_dir.inc) into a
 * per-launch scratch buffer, one work record per section; the blocks are then executed by the lean kernel's second entry
 * like blocks with raw sections. rc_lit / rc_tok are the sections' verdicts (literals first, as the one-wave path orders them). */
#define ZXC_DEV_CLS_LEAN 0u /* raw sections (and every block the lean kernel can name an error for) */
#define ZXC_DEV_CLS_FULL 1u /* RLE literals, oversized or malformed coded sections: the one-wave full kernel */
#define ZXC_DEV_CLS_PRE 2u
#define ZXC_DEV_CLS_LEAN_RLE 3u /* RLE-coded literals, raw tokens, header valid: zxc_rle_expand_kernel expands the literals into the
                                 * block's share of the launch's RLE scratch (lit_off, 16-byte units; verdict in rc_lit), the lean
                                 * kernel then runs the block like one with raw sections */
typedef struct {
    uint32_t lit_off; /* decoded literals at scratch + 16 * lit_off + 16 */
    uint32_t tok_off; /* decoded tokens at scratch + 16 * tok_off */
    int16_t rc_lit, rc_tok;
    uint32_t cls;
} zxc_dev_pre_t;
typedef struct {          /* one coded section on a size class's work list */
    uint64_t src_off;     /* its payload in the compressed buffer */
    uint32_t psize, n;    /* payload bytes (128-byte header included), symbols */
    uint32_t out_off4;    /* decoded bytes at scratch + 4 * out_off4 */
    uint32_t rc_slot;     /* verdict: ((int16_t*)pre)[rc_slot] */
    uint32_t pad[2];
} zxc_dev_sec_t;
/* Control words behind the launch-order buffer's order[] (zxc_hip_shim.hip): */
/* trailer_bytes argument of the decode kernels: 4 = a per-block checksum trails every block; with this bit on top, the checksums are
 * verified by zxc_block_checksum_kernel beside the decode (nine blocks per wavefront) and zxc_checksum_merge_kernel writes the verdicts:
 * the decode kernels only account for the trailer's bytes (round 6) */
#define ZXC_DEV_TRAILER_ELSEWHERE 0x80000000u
#define ZXC_DEV_CTL_WORDS 32u
#define ZXC_DEV_CTL_PRE 0u     /* [0] PRE blocks listed, [1] next to hand out (lean kernel, second entry) */
#define ZXC_DEV_CTL_CURSOR 2u  /* scratch handed out so far, 16-byte units */
#define ZXC_DEV_CTL_WANTED 3u  /* blocks that qualify for PRE, scratch or no scratch (the next launch's plan: zxc_hip_shim.hip) */
#define ZXC_DEV_CTL_SEC 4u     /* [4 + 2 c] sections listed in size class c, [5 + 2 c] next to hand out */
#define ZXC_DEV_CTL_RLE_CURSOR 10u /* RLE scratch handed out so far, 16-byte units (saturating like CURSOR) */
#define ZXC_DEV_CTL_RLE_WANTED 11u /* RLE scratch all LEAN_RLE candidates of the launch would take (sizes the next launch's buffer) */
#define ZXC_DEV_CTL_RLE_LIST 12u   /* [12] LEAN_RLE blocks listed (job indices from the END of the PRE entries array, backwards), [13] next to hand out */

/* Scratch slot of a block with a coded (RLE / PivCo) section, shared by the kernels, the shim's pool and the CPU emulator:
 * [0, R) expanded literals (from +16) | [R, 2R) the section decoder's odd-depth level buffer | [2R, stride) decoded tokens
 * (level 7); R = block_size + 64 bytes of slack. */
#define ZXC_DEV_SLOT_REGION(bs) ((bs) + 64u)
#define ZXC_DEV_SLOT_STRIDE(bs) ((2u * ZXC_DEV_SLOT_REGION(bs) + (bs) / 5u + 16u + 64u + 255u) & ~255u)

/* Host only, plain C (the shim, the CPU emulator, tests). A stream's launch-order buffer, u32 words: [128 histogram + cursors |
 * list: count, next, n entries | order[n] | ctl | PRE job indices[n] | section records, 3 size classes x 2 n x 8 words, 32-byte
 * aligned | pre[n] x 4 words | ck_bad: one byte per block, checksum mismatch]; the shim zeroes [0, 130) and ctl per launch. */
typedef struct { size_t list, order, ctl, pre_ent, secs, pre, ck_bad, words; } zxc_dev_ord_layout_t;
static inline zxc_dev_ord_layout_t zxc_dev_ord_layout(uint32_t n_jobs) {
    const size_t n = n_jobs, ctl = 130u + 2u * n, pre_ent = ctl + ZXC_DEV_CTL_WORDS, secs = (pre_ent + n + 7u) & ~(size_t)7u;
    const zxc_dev_ord_layout_t l = {128u, 130u + n, ctl, pre_ent, secs, secs + 48u * n, secs + 52u * n, secs + 52u * n + (n + 3u) / 4u};
    return l;
}

/* Launch order of a long launch, shared by the launch-order pass, the shim and the CPU emulator: sorted position pos (heaviest
 * first, zxc_order_scatter_kernel's counting sort) -> index in order[]. The last T = min(n, 2 slots) sorted positions, the
 * lightest blocks, stay where they are: they are the launch's tail, where heaviest-first still decides when it ends. The head
 * H = n - T is dealt like a deck: its sorted run cut into ZXC_DEV_ORDER_MIX_ROWS rows (the first q of C, the others of C - 1
 * positions, H = rows (C - 1) + q), read column by column, so every window of the launch holds every weight class. The row
 * count is an odd prime: workgroup ids go round-robin to the 8 XCDs, and index c rows + r lands on XCD (5 c + r) mod 8, no
 * XCD keeps a row. A bijection on [0, n); the identity for n <= 2 slots and for slots == 0 (no mixing). */
#ifndef EXP_ORDER_MIX_ROWS
#define ZXC_DEV_ORDER_MIX_ROWS 61u
#else /* (A/B builds only, behind the gate of zxc_experiments.h) */
#define ZXC_DEV_ORDER_MIX_ROWS EXP_ORDER_MIX_ROWS
#endif
#ifdef __HIPCC__
__host__ __device__
#endif
static inline uint32_t zxc_dev_order_mix(uint32_t pos, uint32_t n, uint32_t slots) {
    const uint64_t tail = 2ull * slots;
    if (slots == 0u || n <= tail) return pos;
    const uint32_t head = n - (uint32_t)tail, rows = ZXC_DEV_ORDER_MIX_ROWS;
    if (pos >= head) return pos;
    const uint32_t c_long = (head + rows - 1u) / rows, q = head - rows * (c_long - 1u); /* 1 <= q <= rows */
    uint32_t r, c;
    if (pos < q * c_long) { r = pos / c_long; c = pos % c_long; }
    else { const uint32_t p = pos - q * c_long; r = q + p / (c_long - 1u); c = p % (c_long - 1u); } /* (q < rows: c_long >= 2) */
    return c * rows + r;
}

/* Decode launch plans. TWO_PASS (no dictionary, no strict capacity): the lean kernel over every block beside the full kernel over
 * the blocks only it decodes, on helper streams; TWO_PASS_PRE: also the section kernels and the lean kernel's second entry. With
 * the checksums apart (ck_apart), a block whose checksum fails is still decoded into its own output slot: those bytes are
 * undefined, its status is ZXC_ERROR_BAD_CHECKSUM, and nothing is written outside the slot. */
enum { ZXC_DEV_PLAN_FULL, ZXC_DEV_PLAN_DICT, ZXC_DEV_PLAN_TWO_PASS, ZXC_DEV_PLAN_TWO_PASS_PRE };
#define ZXC_DEV_DBG_NO_TWO_PASS 0x40000000u /* debug flags of experiment builds */
#define ZXC_DEV_DBG_NO_ORDER 0x80000000u
typedef struct {
    uint32_t kind, ordered, ck_apart, trailer_bytes; /* ZXC_DEV_PLAN_*; the launch-order pass runs; checksums by their own kernel
                                                      * beside the decode; the decode kernels' argument */
    uint64_t pscratch_bytes, rscratch_bytes; /* section / RLE scratch wanted (0: none) */
} zxc_dev_plan_t;
typedef struct { /* all u32, flags 0 / 1 */
    uint32_t dict, cap_override, n_jobs, max_slots, debug, verify_trailer, block_size;
    uint32_t slot, helpers, hint, hint0, hint1; /* the stream's launch-order slot, its helper streams, its hint page and words */
    uint32_t ck_inline, no_rle_scratch, rle_lean_max_jobs, no_pre; /* ZXC_MI355X_CK_INLINE / _NO_RLE_SCRATCH set; ZXC_RLE_LEAN_MAX_JOBS; EXP_NO_PRE */
    uint32_t order_failed, pscratch_failed, rscratch_failed; /* what provisioning the chosen plan could not grant */
} zxc_dev_plan_in_t;

/* Every downgrade is a rule here (what the stream has, what provisioning could not grant). The two-pass plan follows the last
 * launch on the stream (hint0: its PRE-qualified blocks, 0xFFFFFFFF before the first): if none (levels 1-5), no section kernels,
 * whose idle LDS cost the lean kernel 5-30 % beside it, 2 % in front (profiles/r3z_*). Any plan decodes any input. */
static inline zxc_dev_plan_t zxc_dev_plan_choose(const zxc_dev_plan_in_t* in) {
    const uint64_t gib = (uint64_t)1 << 30, n = in->n_jobs, bs = in->block_size;
    const int two_pass = !in->dict && !in->cap_override && !(in->debug & ZXC_DEV_DBG_NO_TWO_PASS);
    const int wants_order = two_pass || (in->n_jobs > in->max_slots && !(in->debug & ZXC_DEV_DBG_NO_ORDER));
    zxc_dev_plan_t p = {in->dict ? ZXC_DEV_PLAN_DICT : ZXC_DEV_PLAN_FULL, wants_order && in->slot && !in->order_failed, 0u,
                        in->verify_trailer ? 4u : 0u, 0u, 0u};
    if (!two_pass || !p.ordered || !in->helpers) return p;
    /* section scratch: what this launch can need at most, capped at 1 GiB (blocks beyond it go to the full kernel) */
    p.kind = (!in->hint || in->hint0 != 0u) && !in->no_pre && !in->pscratch_failed ? ZXC_DEV_PLAN_TWO_PASS_PRE : ZXC_DEV_PLAN_TWO_PASS;
    if (p.kind == ZXC_DEV_PLAN_TWO_PASS_PRE) p.pscratch_bytes = n * (bs + bs / 5u + 256u) < gib ? n * (bs + bs / 5u + 256u) : gib;
    /* RLE scratch: a quarter more than the last launch's LEAN_RLE blocks wanted (hint1, 16-byte units; none: full kernel). Only in
     * launches of < rle_lean_max_jobs blocks: in a short launch the one-wave full kernel ends it with these heaviest blocks (9 702
     * blocks: 1.25 -> 0.90 ms with RLE scratch), in a long one it is faster beside the lean kernel (profiles/r4b_rle_variants.log). */
    if (in->hint && n < in->rle_lean_max_jobs && in->hint1 && !in->no_rle_scratch && !in->rscratch_failed) {
        const uint64_t need = ((uint64_t)in->hint1 * 16u * 5u / 4u + 65536u) & ~(uint64_t)4095u, most = n * (bs + 96u) < gib ? n * (bs + 96u) : gib;
        p.rscratch_bytes = need < most ? need : most;
    }
    p.ck_apart = p.kind == ZXC_DEV_PLAN_TWO_PASS && in->verify_trailer && !in->ck_inline;
    if (p.ck_apart) p.trailer_bytes |= ZXC_DEV_TRAILER_ELSEWHERE;
    return p;
}
#endif
