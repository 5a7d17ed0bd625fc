// zxc_seq_lean.inc — the sequence executor of the LEAN decode kernel (included by zxc_decode_kernel.hip).
//
// Same semantics as run_sequences() (reference: zxc_decode_block_glo_impl src/lib/zxc_decompress.c:847-1209, GHI :1231-1469)
// for blocks whose sections are all raw and that use no dictionary: ~99 % of the blocks of levels 1-5. Everything else
// (RLE / PivCo sections, dictionaries, per-block checksums) is handed to the full kernel through a list (zxc_hip_shim.hip).
// What is different, and why (round 3; issue costs: profiles/r3_issue_test.log):
//   * the kernel is built for 8 waves per SIMD: <= 64 VGPRs, 4.8 KiB of LDS per wave (the full kernel: 96 VGPRs, 7.5 KiB,
//     5 waves). A batch is a chain of dependent LDS / memory round trips; more resident waves hide them.
//   * sources older than the ring ("far", ~47 % of the matches on the silesia mix) never depend on the batch: their first
//     two groups are requested right behind the literal loads, before the dependency analysis, with UNCONDITIONAL loads
//     (idle lanes read the block's first bytes) so the compiler can wait for the literals with an exact vmcnt; far lanes
//     are put by their own pass, near lanes by theirs: no per-group source selects, no conditional loads in the loops.
//   * errors are looked for with one compare per lane: positions are monotone over the lanes, so "the last lane stays
//     inside the capacity / the literal stream" covers everybody; the exact, ordered check only runs when that fails.
//   * single-byte varints: lane i holds extras byte cur+i, one DPP shift pairs it with byte cur+i+1, ONE ds_bpermute
//     hands every lane the (up to two) varints it needs.
//   * dependency analysis: one 6-step binary search over packed (end | start << 16) positions relative to the batch,
//     three probes behind it instead of a second search; the redirect passes test readiness on a ballot.
struct __attribute__((aligned(16))) LeanLds : RingLds {
    uint32_t vval[64];   // general varint path: values / positions of at most LEAN_VARINTS varints per batch
    uint32_t vpos[66];
};
#define LEAN_VARINTS 62u
// Finished output leaves the ring in whole KiB (one full 64-lane store instruction each: a vector-memory instruction costs
// this kernel ~2 % of its time whatever it moves), so up to 1 KiB + a partial 16-byte chunk of the previous batches stays
// unflushed in the ring beside the batch: a tile spans at most RING_BYTES - 1024 - 32 bytes.
#define LEAN_TILE_MAX (RING_BYTES - 1056u)

#ifdef ASM_MARKERS  // (design builds: tools/isacount.py counts the instructions between these comments)
#define PHM(i) asm volatile("; PHMARK " #i)
#else
#define PHM(i) do { } while (0)
#endif

__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {  // number of set bits of m below my lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

template <bool GHI>
__device__ __forceinline__ int run_sequences_lean(const LzStreams& S, uint8_t* __restrict__ dst, uint32_t out_len, uint32_t cap,
                                                  LeanLds& L, int lane, const bool strict) {
    const uint32_t n_total = S.n_seq + 1u;  // + pseudo sequence carrying the trailing literals
    const uint32_t n_lit = S.n_lit;
    // The reference's 4x-unrolled loops refuse a varint-extended sequence unless the worst inline output of the batch's
    // remaining sequences + its wild-copy pad still fits behind it (DECODE_GLO_SEQ / DECODE_GHI_SEQ, src/lib/zxc_decompress.c
    // :626-656, :701-727; the oracle's reserve_4x has the derivation): RW = worst inline output per sequence, RD / RLM = the
    // destination / literal margins of those loops. The 4x batches are a PREFIX of the groups of four (all three loop
    // conditions are monotone in the cursors), so "was my group a 4x batch" is the loop condition at the group's first
    // sequence. Not in the strict decoders (zxc_decompress_block_safe rolls such a batch back to its exact loops).
    const uint32_t RW = GHI ? 513u : 33u, RD = GHI ? 2112u : 168u, RLM = GHI ? 1016u : 56u;
    const uint32_t trig_d = strict ? 0u : 3u * RW + 32u, trig_l = strict ? 0u : 3u * (GHI ? 255u : 15u);
    bool carry4x = true;  // (wave-uniform) the group of four that seq_base cuts began in an earlier batch: its 4x condition
    Out O;
    O.dst = dst;
    O.out_len = out_len;
    O.out_pad = (out_len + 15u) & ~15u;
    O.flushed = 0;
    O.dict = nullptr;
    O.dict_size = 0;
    uint32_t p = 0, lp = 0, cur = 0, dead = 0, seq_base = 0;
    uint32_t z_end = RING_BYTES;
    const bool far_en = O.out_pad >= 32u;  // (idle lanes of the unconditional far loads read the block's first 16 bytes)
    if (lane == 0) ZXC_PATH(GHI ? X_LEAN_GHI : X_LEAN);

    for (uint32_t i = (uint32_t)lane; i < 68u; i += 64u) {
        const int v = (int)(i >> 2) - 4 * (int)(i & 3u);
        LDS_ST32((uint8_t*)L.tmask + 4u * i, v <= 0 ? 0u : (v >= 4 ? 0xFFFFFFFFu : ((1u << (8 * v)) - 1u)));
    }
    ring_zero(L, 0u, RING_BYTES, lane);
    wave_lds_fence();

    // literal offsets are biased by 4: a run's grid origin sits up to 3 bytes in front of it, and an unsigned 32-bit
    // offset from a uniform base is the cheap addressing form (SGPR base + VGPR offset, no 64-bit vector arithmetic)
    const uint8_t* const litm4 = S.lit - 4;
    const uint32_t lit_ph = (uint32_t)(uintptr_t)(S.lit - 8) & 3u;
    const uint8_t* const lit_al = S.lit - 8 - lit_ph;  // (at least 20 header bytes sit in front of the literals)
    uint32_t raw_t, raw_o;
    load_seq_raw<GHI>(S, (uint32_t)lane, raw_t, raw_o);
    // extras byte cur + lane, clamped to the stream's last byte (an empty stream: the byte in front of it), as an unsigned
    // offset from ext - 1
    const uint8_t* const extm1 = S.ext - 1;
    uint32_t xw = ld8(extm1 + lane_off((uint32_t)lane + 1u < S.ext_size ? (uint32_t)lane + 1u : S.ext_size));
    __builtin_amdgcn_s_waitcnt(0);

    while (seq_base < n_total) {
        PHM(0);
        const uint32_t s = seq_base + (uint32_t)lane;
        const bool real = s < S.n_seq;
        bool valid = s < n_total;
        if (!real) { raw_t = 0; raw_o = 0; }
        uint32_t ll, ml, off;
        bool escL, escM;
        if (GHI) {
            ll = raw_t >> 24;
            ml = (raw_t >> 16) & 255u;
            off = (raw_t & 0xFFFFu) + 1u;
            escL = real & (ll == 255u);
            escM = real & (ml == 255u);
        } else {
            ll = raw_t >> 4;
            ml = raw_t & 15u;
            off = 1u + raw_o;
            escL = real & (ll == 15u);
            escM = real & (ml == 15u);
        }
        const uint64_t mL = __ballot(escL), mM = __ballot(escM);
        uint32_t kbad = 0xFFFFFFFFu;
        bool parsed = false, fast_vi = false;
        if ((mL | mM) != 0ull && !dead) {
            parsed = true;
            const uint32_t r = mbcnt64(mL) + mbcnt64(mM);          // rank of my first varint
            const uint32_t r2 = r + (escL ? 1u : 0u);              // rank of my match-length varint
            // a batch takes at most LEAN_VARINTS varints (the fast path's window and the general path's tables): later
            // sequences wait for the next batch
            const uint64_t late = __ballot(r2 + (escM ? 1u : 0u) > LEAN_VARINTS);
            uint64_t vm = ~0ull;
            if (late) {
                const int f = __ffsll((unsigned long long)late) - 1;  // (>= 30: sixty varints come from at least thirty lanes)
                vm = (1ull << f) - 1ull;
                valid = valid && lane < f;
                if (lane == 0) ZXC_PATH(L_VARINT_CUT);
            }
            const uint32_t nv = __popcll(mL & vm) + __popcll(mM & vm);
            uint32_t bL = 0, bM = 0;
            if (cur + nv <= S.ext_size) {
                // extras bytes cur+i and cur+i+1 side by side in lane i: varint number r of a single-byte batch IS byte r
                const uint32_t pair = xw | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)xw, 0x130, 0xf, 0xf, false) << 8);  // wave_shl:1
                const uint32_t q = __shfl(pair, (int)(r & 63u));
                bL = q & 255u;
                bM = escL ? (q >> 8) & 255u : bL;
                const bool big = valid && ((escL && bL >= 0x80u) || (escM && bM >= 0x80u));
                fast_vi = __ballot(big) == 0ull;
            }
            if (fast_vi) {
                if (lane == 0) ZXC_PATH(L_VARINT_FAST);
                ll += escL ? bL : 0u;
                ml += escM ? bM : 0u;
            } else {
                if (lane == 0) ZXC_PATH(L_VARINT_GENERAL);
                // (the same in every lane; said so, it and the cursor and the dead flag behind it are scalars, not lane registers)
                kbad = uni(parse_varints(S.ext, S.ext_size, cur, nv, L, lane));
                if (valid && escL && r < kbad) ll += L.vval[r];
                if (valid && escM && r2 < kbad) ml += L.vval[r2];
            }
        }
        PHM(1);
        ml += real ? 5u : 0u;

        // cursors: inclusive scans of (ll+ml) and ll
        uint32_t len = ll + ml;
        const uint32_t Ei = wave_scan_add(len);
        const uint32_t Li = wave_scan_add(ll);
        const uint32_t est = p + (Ei - len);  // where this sequence's literals land
        const uint32_t lst = lp + (Li - ll);  // its first literal
        const bool bad_off = real && off > est + ll;
        int err = 0;
        {
            // Positions grow with the lane: if the last lane's end is inside the capacity and its literals inside the
            // stream, so is everybody's. Only then, and with every offset in range, the batch cannot fail; the last
            // batch of a block (the pseudo sequence) and anything suspicious take the exact, ordered check
            // (reference: OVERFLOW src/lib/zxc_decompress.c:1184, BAD_OFFSET :1190).
            const uint32_t E63 = p + (uint32_t)__builtin_amdgcn_readlane((int)Ei, 63);
            const uint32_t L63 = lp + (uint32_t)__builtin_amdgcn_readlane((int)Li, 63);
            if (seq_base + 64u >= n_total || E63 + trig_d > cap || L63 + trig_l > n_lit || __ballot(bad_off) != 0ull) {
                if (lane == 0) ZXC_PATH(L_EXACT);
                const bool pseudo = valid & !real;  // whatever literals are left
                const bool lit_over = lst > n_lit;
                const uint32_t lit_left = n_lit - lst;
                bool ovf_real = (est > cap) | (len > cap - est) | lit_over | (ll > lit_left);
                if (!strict) {  // the 4x batches' reserve (only batches this close to either end can trip it: trig_d, trig_l)
                    const uint32_t gi = s & 3u;
                    const int gl = lane - (int)gi;  // my group's first sequence (< 0: in an earlier batch)
                    const uint32_t g_est = __shfl(est, gl < 0 ? 0 : gl), g_lst = __shfl(lst, gl < 0 ? 0 : gl);
                    bool g4 = gl >= 0 ? (g_est + RD < cap && n_lit > RLM && g_lst < n_lit - RLM) : carry4x;
                    g4 = g4 && real && S.n_seq - (s - gi) >= 4u;
                    const uint32_t rawl = GHI ? raw_t >> 24 : raw_t >> 4;  // RAW literal-length fields of the sequences behind me in my group
                    const uint32_t r1 = __shfl(rawl, (lane + 1) & 63), r2 = __shfl(rawl, (lane + 2) & 63), r3 = __shfl(rawl, (lane + 3) & 63);
                    const uint32_t rest = (gi < 3u ? r1 : 0u) + (gi < 2u ? r2 : 0u) + (gi < 1u ? r3 : 0u);
                    const bool r_lit = escL && !lit_over && ll + rest > lit_left;
                    const bool r_dst = (escL | escM) && est <= cap && len + (3u - gi) * RW + 32u > cap - est;
                    ovf_real |= g4 & (r_lit | r_dst);
                    // a group that reaches beyond the 64 sequences in hand is judged by the batch that holds all of it
                    if (seq_base + 64u < S.n_seq && lane + (int)(3u - gi) > 63) valid = false;
                }
                const bool ovf_pseudo = (est > cap) | lit_over | (lit_left > cap - est);
                err = (real & bad_off) ? E_BAD_OFFSET : err;
                err = ((real & ovf_real) | (pseudo & ovf_pseudo)) ? E_OVERFLOW : err;
                if (!valid) err = 0;  // (a sequence cut off by the varint limit is judged by the batch that takes it)
                if (pseudo & !ovf_pseudo) { ll = lit_left; len = lit_left; }
            }
        }
        PHM(2);
        const uint32_t M = est + ll;
        const uint32_t E = est + len;

        // how many leading sequences fit a tile of TILE_MAX bytes (errors first, in order)
        const uint64_t fits = __ballot(valid && err == 0 && (E - p) <= LEAN_TILE_MAX);
        uint32_t k = (uint32_t)__ffsll((unsigned long long)~fits);  // 1-based index of first non-fitting lane
        k = k ? k - 1u : 64u;
        {
            const uint64_t em = __ballot(err != 0);
            if (em) {
                const uint32_t e = (uint32_t)__ffsll((unsigned long long)em) - 1u;
                if (e <= k) {
                    if (lane == 0) ZXC_PATH(L_ERR);
                    return __shfl(err, (int)e);  // first failing sequence in stream order
                }
            }
        }

        if ((uint32_t)lane == k && k != 0u && valid && err == 0) ZXC_PATH(L_TILE_CUT);  // (the first sequence beyond the tile; k == 0 is a giant)
        PHM(3);
        // the next batch starts at sequence seq_base + max(k, 1): request its tokens and offsets now
        uint32_t nraw_t, nraw_o;
        load_seq_raw<GHI>(S, seq_base + (k ? k : 1u) + (uint32_t)lane, nraw_t, nraw_o);
        if (parsed) {
            const uint32_t kk = k ? k : 1u;
            const uint64_t km = (kk >= 64u) ? ~0ull : ((1ull << kk) - 1ull);
            const uint32_t used = __popcll(mL & km) + __popcll(mM & km);
            if (fast_vi) cur += used;
            else if (kbad < used) {
                if (lane == 0) ZXC_PATH(L_DEAD);
                dead = 1;
                cur = S.ext_size;
            }
            else cur = uni(L.vpos[used]);
        }
        const uint32_t xi1 = cur + 1u + (uint32_t)lane;  // (cur ends at most one varint window behind a block's section: no wrap)
        const uint32_t nxw = ld8(extm1 + lane_off(xi1 < S.ext_size ? xi1 : S.ext_size));

        PHM(4);
        if (k == 0u) {
            // ---- one giant sequence (> LEAN_TILE_MAX bytes): the whole wave walks it in pieces (plain stores)
            if (lane == 0) ZXC_PATH(L_GIANT);
            __builtin_amdgcn_s_waitcnt(0);
            flush_to(L, O, p, lane);  // (everything finished so far: the pieces below fill the ring)
            const uint32_t gll = uni(ll), gml = uni(ml), goff = uni(off);
            uint32_t donel = 0;
            while (donel < gll) {
                const uint32_t n = (gll - donel < TILE_MAX) ? gll - donel : TILE_MAX;
                if (lane == 0) ZXC_PATH(L_GIANT_LIT_PIECE);
                coop_copy<false>(L, O, p + donel, 0, S.lit + lp + donel, n, 0, lane);
                donel += n;
                flush_to(L, O, p + donel, lane);
            }
            if (gml) {
                if (lane == 0) ZXC_PATH(L_GIANT_MATCH);
                __builtin_amdgcn_s_waitcnt(0);  // earlier flush stores must have left before reading them back
                coop_match<false>(L, O, p + gll, gml, goff, 0, true, lane);
            }
            p += gll + gml;
            lp += gll;
            k = 1;
            z_end = (p + 15u) & ~15u;
            if (p + (uint32_t)lane < z_end) ring_wr8(L, p + (uint32_t)lane, 0u);
        } else {
            const bool mine = (uint32_t)lane < k;
            const uint32_t tile_end = (uint32_t)__builtin_amdgcn_readlane((int)E, (int)(k - 1u));
            const uint32_t z_new = (tile_end + 15u) & ~15u;
            const uint32_t ring_lo = z_new > RING_BYTES ? z_new - RING_BYTES : 0u;
            if (z_new > z_end) {
                ring_zero(L, z_end, z_new, lane);
                z_end = z_new;
            }

            PHM(5);
            // ---- requests. Literal run: group g = the 16 bytes at output position (est & ~3) + 16 g, from literal offset
            // lst - (est & 3) + 16 g (loads take any alignment: the bytes arrive on the destination's dword grid).
            const uint32_t la = est & 3u;
            const uint32_t le = la + ll;  // end of the run on its grid
            const bool lshort = mine & (ll - 1u < LIT_MED);  // (0 < ll <= LIT_MED)
            // Lane predicates are straight-line code: & and | on values in registers, one unsigned compare for a range. And the
            // literal passes carry no mask beside the run: les is its end for the lanes of the group path and 0 for everybody
            // else (le >= 1 there), so every later "lshort && le > x" is ONE compare of it.
            const uint32_t les = lshort ? le : 0u;
            const uint32_t lo = lst - la + 4u;  // offset from litm4
            // Group 0 (the one most lanes need) is fetched dword-ALIGNED: an unaligned 16-byte gather costs the CU's address
            // pipeline 4 clocks per active lane, an aligned one 1.3 (profiles/r3_vmem_test.log). Four aligned dwords and a fifth
            // for the lanes whose last bytes sit there; v_alignbyte moves them onto the destination grid.
            const uint32_t lob = lo + 4u + lit_ph;           // offset from lit_al = (S.lit - 8) rounded down to a dword
            const uint32_t ldl = lob & 3u;
            const v4u lv0 = ld128(lit_al + lane_off(lshort ? (lob & ~3u) : 8u));
            const bool lv5 = (ldl != 0u) & (les > 12u);  // the run's last bytes of group 0 sit in a fifth aligned dword
            const uint32_t lv0e = ld32(lit_al + lane_off(lv5 ? (lob & ~3u) + 16u : 8u));
            const v4u lv1 = ld128(litm4 + lane_off(les > 16u ? lo + 16u : 4u - lit_ph));
            if (lshort) ZXC_PATH(L_LIT_GROUP);
            if (lv5) ZXC_PATH(L_LIT_5TH);
            const v4u lv2 = ld128(litm4 + lane_off(les > 32u ? lo + 32u : 4u - lit_ph));

            // Match: group g = 16 bytes at (M & ~3) + 16 g, from source position qsrc - (M & 3) + 16 g.
            const uint32_t ma = M & 3u;
            const uint32_t me = ma + ml;
            const uint32_t mg = M - ma;
            const uint32_t qa = M - off;  // (my lanes: off <= M, checked above)
            const bool overlap = off < ml;
            bool pending = mine & (ml != 0u);
            // Far: the source starts behind the ring. It ends at least 350 bytes before the batch (ring_lo <= p - 497,
            // ml <= MATCH_MED), all of it was flushed by earlier batches (a wave's stores and loads reach L2 in program
            // order), it cannot overlap its destination and depends on nothing in this batch: every group comes from the
            // block's own output in memory, the first two are requested here.
            // (round 5: output leaves the ring in whole KiB — see the flush at the batch's end — so the source must also END inside what
            //  has been flushed; a source that straddles the flushed mark, ~3 % of them, takes the near path's whole-wave copy)
            // (no && here: every clause is arithmetic on registers, and a short-circuit chain costs this loop two nested exec
            // regions. 4 <= qa < ring_lo is one unsigned compare against ring_lo - 4, clamped at 0 where the ring still holds all.)
            const uint32_t sgf = qa - ma;
            const uint32_t far_hi = ring_lo > 4u ? ring_lo - 4u : 0u;
            const bool far_ok = far_en & pending & (qa - 4u < far_hi) & (ml <= MATCH_MED) & (qa + ml <= O.flushed) &
                                (sgf + ((me + 15u) & ~15u) + 4u <= O.out_pad);
            const uint32_t mef = far_ok ? me : 0u;  // like les: the match's end on its grid on the far lanes (me >= 1), 0 elsewhere
            // (The NO_* markers restate far_ok's clauses: naming the clauses once changes the kernel's register allocation. Only
            // L_FAR_GROUP observes far_ok itself, so every case that asks for a NO_* marker also pins L_FAR_GROUP's exact count.)
            if (pending && qa < ring_lo) {  // a source behind the ring: the group path, or which guard sends it to the near paths
                if (far_ok) ZXC_PATH(L_FAR_GROUP);
                if (!far_en) ZXC_PATH(L_FAR_OFF);
                if (ml > MATCH_MED) ZXC_PATH(L_FAR_NO_ML);
                if (qa < 4u) ZXC_PATH(L_FAR_NO_QA4);
                if (qa + ml > O.flushed) ZXC_PATH(L_FAR_NO_FLUSHED);
                if ((qa - ma) + ((me + 15u) & ~15u) + 4u > O.out_pad) ZXC_PATH(L_FAR_NO_EDGE);
            }
            const uint32_t fdl = sgf & 3u;  // (the block's slot is 16-byte aligned: the source's phase against the destination grid)
            v4u fr0 = {0, 0, 0, 0}, fr1 = {0, 0, 0, 0};
            uint32_t fr0e = 0;
            if (far_en) {  // wave-uniform. Group 0 dword-aligned like the literals'; group 1 is wanted by few lanes.
                // (uniform base + 32-bit lane offset, like the literal loads)
                fr0 = ld128(dst + lane_off(far_ok ? (sgf & ~3u) : 0u));
                const bool fr5 = (fdl != 0u) & (mef > 12u);
                fr0e = ld32(dst + lane_off(fr5 ? (sgf & ~3u) + 16u : 0u));
                if (fr5) ZXC_PATH(L_FAR_5TH);
                fr1 = ld128(dst + lane_off(mef > 16u ? sgf + 16u : 0u));
            }

            // ---- dependencies. Sequence i may only copy once every earlier match of this batch that overlaps its
            // source [qa, qb) is finished: lanes ja .. jb-1.
            const uint32_t qb = (qa + ml < M) ? qa + ml : M;
            uint64_t need = 0;
            uint32_t qsrc = qa;
            const bool inb = pending & !far_ok & (qb > p);  // the source reaches into this batch
            if (__ballot(inb)) {
                // positions relative to the batch: 12 bits each (a tile spans at most TILE_MAX < 4096 bytes)
                const uint32_t key = mine ? ((E - p) | ((M - p) << 16)) : 0xFFFFFFFFu;
                const uint32_t xa = qa > p ? qa - p : 0u;
                uint32_t ja = 0;  // lanes with E <= qa
#pragma unroll
                for (int st = 32; st >= 1; st >>= 1) {
                    const uint32_t t = __shfl(key, (int)(ja + st - 1u)) & 0xFFFFu;
                    if (t <= xa) ja += st;
                }
                // lanes ja, ja+1, ... overlap the source while their match starts in front of its end
                const uint32_t k0 = __shfl(key, (int)(ja & 63u)), k1 = __shfl(key, (int)((ja + 1u) & 63u)),
                               k2 = __shfl(key, (int)((ja + 2u) & 63u));
                const uint32_t xb = qb - p;
                const bool o0 = (k0 >> 16) < xb;
                const bool o1 = o0 & (ja + 1u < 64u) & ((k1 >> 16) < xb);
                const bool o2 = o1 & (ja + 2u < 64u) & ((k2 >> 16) < xb);
                uint32_t jb = ja + (o0 ? 1u : 0u) + (o1 ? 1u : 0u);
                if (o2) jb = (uint32_t)lane;  // a source over more than two earlier matches: wait for everything in front
                if (inb && o2) ZXC_PATH(L_WAIT_ALL);
                need = (inb & (jb > ja)) ? (((jb >= 64u) ? ~0ull : ((1ull << jb) - 1ull)) & ~((1ull << ja) - 1ull)) : 0ull;
                // Redirect: when my whole source sits inside ONE earlier match j of this batch (within its first period) and
                // j has no pending dependency itself, my bytes equal j's source bytes at the same displacement: read those
                // instead and drop the dependency — unless they are behind the ring (not requested: wait for j instead).
                const uint32_t jM = p + (k0 >> 16), jE = p + (k0 & 0xFFFFu);
                const uint32_t jo = __shfl(off, (int)(ja & 63u));
                const bool simple = (need != 0ull) & (jb == ja + 1u) & (off >= ml) & (qa >= jM) & (qb <= jE) & (qb - jM <= jo);
#pragma unroll
                for (int pass = 0; pass < REDIRECT_PASSES; pass++) {
                    const uint64_t rm = __ballot(need == 0ull);
                    const uint32_t jq = __shfl(qsrc, (int)(ja & 63u));
                    const uint32_t nq = jq + (qa - jM);
                    // (restates the condition below, for the same reason: the case pins L_REDIRECT0's exact count beside it)
                    if (simple && need != 0ull && ((rm >> (ja & 63u)) & 1ull) && !(nq >= ring_lo && (int32_t)nq >= 0)) ZXC_PATH(L_REDIRECT_NO_RING);
                    const bool redir = simple & (need != 0ull) & (((rm >> (ja & 63u)) & 1ull) != 0ull) & (nq >= ring_lo) & ((int32_t)nq >= 0);
                    if (redir) ZXC_PATH(pass == 0 ? L_REDIRECT0 : L_REDIRECT1);
                    qsrc = redir ? nq : qsrc;
                    need = redir ? 0ull : need;
                }
            }
            PHM(7);
            const uint32_t sg = qsrc - ma;  // the match's source on the destination's dword grid
            const bool nearl = pending & !far_ok;
            const bool inring = nearl & (qsrc >= ring_lo);  // (the others: far but too long / too close to the block's edges for the group path)
            const bool shortp = overlap & (off < 16u);      // a period shorter than a group
            const bool stepable = inring & (ml <= MATCH_MED) & !shortp;
            const bool bytewise = inring & shortp & (ml <= BYTEWISE_MAX);
            const bool is_long = nearl & !stepable & !bytewise;
            bool far_waited = false;

            PHM(8);
            // ---- literals: one masked ds_or group per 16 bytes of grid (the far groups stay in flight)
            {
                const uint32_t lg = est - la;
                {
                    const uint32_t t = group_take(les, 0u);
                    v4u d;
                    d.x = __builtin_amdgcn_alignbyte(lv0.y, lv0.x, ldl);
                    d.y = __builtin_amdgcn_alignbyte(lv0.z, lv0.y, ldl);
                    d.z = __builtin_amdgcn_alignbyte(lv0.w, lv0.z, ldl);
                    d.w = __builtin_amdgcn_alignbyte(lv0e, lv0.w, ldl);
                    d = group_keep_first(L, d, t);
                    d.x &= head_mask(la);
                    ring_or_group(L, lg, d);
                }
                if (lanes_gt(les, 16u)) ring_or_group(L, lg + 16u, group_keep_first(L, lv1, group_take(les, 16u)));
                if (lanes_gt(les, 32u)) ring_or_group(L, lg + 32u, group_keep_first(L, lv2, group_take(les, 32u)));
#pragma unroll 1
                for (uint32_t go = 48u; go < LIT_MED + 4u; go += 32u) {  // two groups per step, both requested by every lane
                    const bool actA = les > go, actB = les > go + 16u;
                    if (lanes_gt(les, go) == 0ull) break;
                    const v4u lvA = ld128(litm4 + lane_off(actA ? lo + go : 4u - lit_ph));
                    const v4u lvB = ld128(litm4 + lane_off(actB ? lo + go + 16u : 4u - lit_ph));
                    ring_or_group(L, lg + go, group_keep_first(L, lvA, group_take(les, go)));
                    ring_or_group(L, lg + go + 16u, group_keep_first(L, lvB, group_take(les, go + 16u)));
                }
                uint64_t lm = __ballot(mine & (ll > LIT_MED));
                while (lm) {
                    const int j = __ffsll((unsigned long long)lm) - 1;
                    lm &= lm - 1ull;
                    const uint32_t jl = (uint32_t)__builtin_amdgcn_readlane((int)ll, j), je = (uint32_t)__builtin_amdgcn_readlane((int)est, j),
                                   js = (uint32_t)__builtin_amdgcn_readlane((int)lst, j);
                    if (lane == 0) ZXC_PATH(L_LIT_LONG);
                    coop_copy<false>(L, O, je, 0, S.lit + js, jl, 0, lane);
                }
            }

            PHM(9);
            // ---- far matches: their own pass (nothing in this batch can be their source)
            if (lanes_gt(mef, 0u)) {
                {
                    const uint32_t t = group_take(mef, 0u);
                    v4u d;
                    d.x = __builtin_amdgcn_alignbyte(fr0.y, fr0.x, fdl);
                    d.y = __builtin_amdgcn_alignbyte(fr0.z, fr0.y, fdl);
                    d.z = __builtin_amdgcn_alignbyte(fr0.w, fr0.z, fdl);
                    d.w = __builtin_amdgcn_alignbyte(fr0e, fr0.w, fdl);
                    d = group_keep_first(L, d, t);
                    d.x &= head_mask(ma);
                    ring_or_group(L, mg, d);
                }
                if (lanes_gt(mef, 16u)) ring_or_group(L, mg + 16u, group_keep_first(L, fr1, group_take(mef, 16u)));
#pragma unroll 1
                for (uint32_t go = 32u; go < MATCH_MED + 4u; go += 32u) {  // two groups per step, both requested by every lane
                    const bool actA = mef > go, actB = mef > go + 16u;
                    if (lanes_gt(mef, go) == 0ull) break;
                    const v4u fA = ld128(dst + lane_off(actA ? sgf + go : 0u));
                    const v4u fB = ld128(dst + lane_off(actB ? sgf + go + 16u : 0u));
                    ring_or_group(L, mg + go, group_keep_first(L, fA, group_take(mef, go)));
                    ring_or_group(L, mg + go + 16u, group_keep_first(L, fB, group_take(mef, go + 16u)));
                }
            }
            pending = nearl;  // (the far lanes are done)
            wave_lds_fence();

            PHM(10);
            // ---- near matches: rounds over the dependency masks
            for (uint32_t round = 0;; round++) {
                const uint64_t dm = __ballot(!pending);
                if (dm == ~0ull) break;
                if (round > 70u) return ZXC_DEV_E_INTERNAL;  // cannot happen: the lowest pending lane is always ready
                const bool can = pending & ((dm & need) == need);
                const bool sa = can & stepable;
                if (sa) ZXC_PATH(L_STEPABLE);
                const uint32_t mes = sa ? me : 0u;  // (like les and mef: the lanes that step this round)
                if (lanes_gt(mes, 0u)) {
#pragma unroll 1
                    for (uint32_t go = 0; go < MATCH_MED + 4u; go += 16u) {
                        const bool act = mes > go;
                        if (lanes_gt(mes, go) == 0ull) break;
                        v4u d = ring_rd128(L, act ? sg + go : 0u);
                        d = group_keep_first(L, d, group_take(mes, go));
                        if (go == 0u) d.x &= head_mask(ma);
                        ring_or_group(L, mg + go, d);
                    }
                }
                PHM(11);
                // short period (off < 16, off < ml <= 32): byte loop over the period [M-off, M)
                const bool sb = can & bytewise;
                if (sb) ZXC_PATH(L_BYTEWISE);
                const uint32_t mlb = sb ? ml : 0u;
                if (lanes_gt(mlb, 0u)) {
                    uint32_t r = 0;
#pragma unroll 1
                    for (uint32_t t = 0; t < BYTEWISE_MAX; t++) {
                        const bool act = t < mlb;  // (the byte stores stay masked: an idle lane has no harmless byte to store)
                        if (lanes_gt(mlb, t) == 0ull) break;
                        if (act) {
                            ring_wr8(L, M + t, ring_rd8(L, qa + r));
                            r = (r + 1u == off) ? 0u : r + 1u;
                        }
                    }
                }
                // long: the whole wave copies one match at a time
                uint64_t lm = __ballot(can & is_long);
                if (lm) wave_lds_fence();
                while (lm) {
                    const int j = __ffsll((unsigned long long)lm) - 1;
                    lm &= lm - 1ull;
                    const uint32_t jM = (uint32_t)__builtin_amdgcn_readlane((int)M, j), jml = (uint32_t)__builtin_amdgcn_readlane((int)ml, j),
                                   joff = (uint32_t)__builtin_amdgcn_readlane((int)off, j);
                    if (jM - joff < ring_lo && !far_waited) { __builtin_amdgcn_s_waitcnt(0); far_waited = true; }
                    if (lane == 0) ZXC_PATH(L_LONG);
                    if (lane == 0 && jM - joff < ring_lo) ZXC_PATH(L_LONG_FAR);
                    coop_match<false>(L, O, jM, jml, joff, ring_lo, false, lane);
                }
                pending = pending & !can;
                wave_lds_fence();
                PHM(12);
                // few sequences left: finish them one by one, in stream order, with the whole wave (a byte per lane)
                uint64_t pm = __ballot(pending);
                if (pm != 0ull && __popcll(pm) <= SPARSE_MAX) {
                    const uint64_t longm = __ballot(is_long);
                    if (lane == 0) ZXC_PATH(L_SPARSE);
                    while (pm) {
                        const int j = __ffsll((unsigned long long)pm) - 1;
                        pm &= pm - 1ull;
                        const uint32_t jM = (uint32_t)__builtin_amdgcn_readlane((int)M, j),
                                       jml = (uint32_t)__builtin_amdgcn_readlane((int)ml, j),
                                       joff = (uint32_t)__builtin_amdgcn_readlane((int)off, j);
                        const uint32_t jq = jM - joff;
                        if (((longm >> j) & 1ull) || jq < ring_lo) {
                            if (jq < ring_lo && !far_waited) { __builtin_amdgcn_s_waitcnt(0); far_waited = true; }
                            if (lane == 0) ZXC_PATH(L_SPARSE_COOP);
                            coop_match<false>(L, O, jM, jml, joff, ring_lo, false, lane);
                            continue;
                        }
                        const bool ovl = joff < jml;  // period joff: byte t comes from the first period, t mod joff
                        if (lane == 0) ZXC_PATH(ovl ? L_SPARSE_OVL : L_SPARSE_PLAIN);
                        const float rcp = __builtin_amdgcn_rcpf((float)joff);
                        for (uint32_t t0 = 0; t0 < jml; t0 += 64u) {
                            const uint32_t t = t0 + (uint32_t)lane;
                            uint32_t r = t;
                            if (ovl) {
                                const uint32_t qd = (uint32_t)((float)t * rcp);
                                r = t - qd * joff;
                                if ((int32_t)r < 0) r += joff;
                                if (r >= joff) r -= joff;
                            }
                            if (t < jml) ring_wr8(L, jM + t, ring_rd8(L, jq + r));
                        }
                        wave_lds_fence();
                    }
                    pending = false;
                    break;
                }
            }
            PHM(13);
            p = tile_end;
            lp = (uint32_t)__builtin_amdgcn_readlane((int)(lst + ll), (int)(k - 1u));
            __builtin_amdgcn_s_waitcnt(0);  // (only the flush stores stay outstanding across the loop edge)
            // Whole KiB only: one full 64-lane store instruction per KiB (round 4 flushed every finished 16-byte chunk: 87 store
            // instructions per 64 KiB block instead of 64, and a vector-memory instruction is what a batch pays for: +1-2 %,
            // profiles/r5e_*). Up to 1 KiB + 15 bytes of earlier batches stay in the ring: LEAN_TILE_MAX leaves room for them.
            flush_to(L, O, p & ~1023u, lane);
        }
        PHM(14);
        if (!strict && ((seq_base + k) & 3u) != 0u) {  // (only behind a cut batch: full batches keep seq_base a multiple of 4)
            const uint32_t g = (seq_base + k) & ~3u;   // the group the next batch starts inside
            if (g >= seq_base) {
                const uint32_t ge = (uint32_t)__builtin_amdgcn_readlane((int)est, (int)(g - seq_base)),
                               gl = (uint32_t)__builtin_amdgcn_readlane((int)lst, (int)(g - seq_base));
                carry4x = ge + RD < cap && n_lit > RLM && gl < n_lit - RLM;
                if (lane == 0) ZXC_PATH(L_CARRY4X);
            }
        }
        seq_base += k;
        raw_t = nraw_t;
        raw_o = nraw_o;
        xw = nxw;
        wave_lds_fence();
    }
    flush_to(L, O, p, lane);  // what is left of the last KiB
    // the last chunk may be partial: it only lives in the ring so far
    if ((p & 15u) != 0u && lane == 0) {
        ZXC_PATH(L_PARTIAL_CHUNK);
        const uint32_t cs = p & ~15u;
        for (uint32_t kk = 0; cs + kk < p && cs + kk < out_len; kk++) dst[cs + kk] = (uint8_t)ring_rd8(L, cs + kk);
    }
    return (int)p;
}

// Block body of the lean kernel. Returns the decoded size / a negative zxc_error_t, or ZXC_DEV_DEFER for a block that
// needs the full kernel (a coded literal / token section).
// pd != nullptr: a ZXC_DEV_CLS_PRE block, its coded sections already decoded into pscratch (zxc_pivco_sections_*_kernel) and
// its header checked by classify_block.
__device__ __forceinline__ int decode_lz_block_lean(const uint8_t* data, uint32_t comp_sz, bool ghi, uint8_t* dst, uint32_t out_len,
                                                    uint32_t cap, LeanLds& L, int lane, const zxc_dev_pre_t* pd,
                                                    const uint8_t* pscratch, const bool strict, const uint8_t* rle_lit = nullptr,
                                                    const bool rle_ok = false) {
    if (comp_sz < 12u) return E_BAD_HEADER;
    LzStreams S;
    S.dict = nullptr;
    S.dict_size = 0;
    S.n_seq = uni(ld32(data));
    S.n_lit = uni(ld32(data + 4));
    const uint32_t enc_lit = uni(ld8(data + 8)), enc_tok = uni(ld8(data + 9)), enc_off = uni(ld8(data + 11));
    const uint32_t avail = comp_sz - 12u;
    if (ghi) {
        if (enc_lit != 0u || enc_tok != 0u) return E_CORRUPT;
        const uint64_t consumed = (uint64_t)S.n_lit + 4ull * S.n_seq;
        if (consumed > avail || avail - S.n_lit < 32u) return E_CORRUPT;
        S.lit = data + 12;
        S.tok = S.lit + S.n_lit;
        S.offs = nullptr;
        S.off8 = 0;
        S.ext = S.tok + 4ull * S.n_seq;
        S.ext_size = avail - (uint32_t)consumed;
        return run_sequences_lean<true>(S, dst, out_len, cap, L, lane, strict);
    }
    // GLO: ONE call site of the executor for the three ways a block's streams are found (the executor is inlined: every call
    // site is another copy of it, and the register allocation of the kernel is that of all copies together).
    if (!pd && rle_ok) {
        if (lane == 0) ZXC_PATH(X_SETUP_RLE);
        // RLE-coded literals, raw tokens, header checked (rle_block_for_lean): zxc_rle_expand_kernel has expanded the literals
        // into the launch's RLE scratch (rle_lit; unused when n_lit == 0)
        const uint32_t lit_comp = uni(ld32(data + 12));
        const uint8_t* d = data + 16;
        const uint32_t sz_off = S.n_seq * (enc_off ? 1u : 2u);
        S.lit = S.n_lit ? rle_lit : d;
        S.tok = d + lit_comp;
        S.offs = S.tok + S.n_seq;
        S.off8 = enc_off;
        S.ext = S.offs + sz_off;
        S.ext_size = comp_sz - 16u - (lit_comp + S.n_seq + sz_off);
    } else if (enc_lit != 0u || enc_tok != 0u) {
        if (!pd) return ZXC_DEV_DEFER;  // (also every invalid coding: the full kernel names the error)
        const uint32_t rcs = uni(*(const uint32_t*)&pd->rc_lit);  // {rc_lit, rc_tok}: the literal section's verdict comes first
        if ((int16_t)(rcs & 0xFFFFu) != 0) return (int)(int16_t)(rcs & 0xFFFFu);
        if ((int16_t)(rcs >> 16) != 0) return (int)(int16_t)(rcs >> 16);
        const uint32_t desc = (enc_lit != 0u ? 4u : 0u) + (enc_tok == 2u ? 4u : 0u);
        if (lane == 0) ZXC_PATH(X_SETUP_PRE);
        uint32_t lit_comp = S.n_lit, tok_comp = S.n_seq;
        const uint8_t* d = data + 12;
        if (enc_lit != 0u) { lit_comp = uni(ld32(d)); d += 4; }
        if (enc_tok == 2u) { tok_comp = uni(ld32(d)); d += 4; }
        const uint32_t sz_off = S.n_seq * (enc_off ? 1u : 2u);
        S.lit = enc_lit != 0u ? pscratch + 16ull * uni(pd->lit_off) + 16u : d;
        S.tok = enc_tok != 0u ? pscratch + 16ull * uni(pd->tok_off) : d + lit_comp;
        S.offs = d + lit_comp + tok_comp;
        S.off8 = enc_off;
        S.ext = S.offs + sz_off;
        S.ext_size = comp_sz - 12u - desc - (lit_comp + tok_comp + sz_off);
    } else {
        if (enc_off > 1u) return E_CORRUPT;
        const uint64_t sz_off = (uint64_t)S.n_seq * (enc_off ? 1u : 2u);
        const uint64_t consumed = (uint64_t)S.n_lit + S.n_seq + sz_off;
        if (consumed > avail || avail - S.n_lit < 32u) return E_CORRUPT;
        S.lit = data + 12;
        S.tok = S.lit + S.n_lit;
        S.offs = S.tok + S.n_seq;
        S.off8 = enc_off;
        S.ext = S.offs + sz_off;
        S.ext_size = avail - (uint32_t)consumed;
        if (lane == 0) ZXC_PATH(X_SETUP_RAW);
    }
    return run_sequences_lean<false>(S, dst, out_len, cap, L, lane, strict);
}
