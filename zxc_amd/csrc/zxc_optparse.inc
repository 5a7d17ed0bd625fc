// zxc_optparse.inc — levels 6-7: the price-based optimal parse of a block, for one wavefront (included by zxc_encode_kernel.hip).
// Reference being replaced: zxc_lz77_optimal_parse_glo (src/lib/zxc_compress.c:795-1042) and its literal price
// zxc_opt_estimate_lit_bits (:720-753). Same model, not the same loop:
//   * dp[x] = fewest bits that encode block[0, x). A literal costs `lit` bits (the block's predicted bits per literal), a match of
//     length L costs 24 bits (token + 16-bit offset, ZXC_OPT_MATCH_COST_BASE) + 8 per varint byte of L - 5 - 15; every position
//     offers ONE match — the longest the finder saw there, lazy probes off — in all its lengths 5 .. Lmax (the DP picks where a
//     match should end); positions strictly inside a match of >= 256 bytes offer none (ZXC_OPT_LONG_MATCH_SKIP).
//   * The reference relaxes forward one position at a time. A match ends at least 5 positions ahead, so the literal chain of five
//     consecutive positions can be closed first (scalar unit) and their matches pushed TOGETHER: 12 lanes per position, one
//     candidate length per lane, ds_min_u64 on packed entries {cost : 32 | 0xFFFF - length : 16 | distance : 16} in an LDS window
//     of the next 4096 positions (lengths are capped at 4080 here: a longer match is continued by the one found where it ends).
//     Ties go to the longer match and a match beats a literal of the same cost, like the reference's strict `<` in visiting order.
//   * A position's entry is final when the batch reaches it: its low half is written back over the finder's record of that
//     position (mp[]: one array per block, first "longest match at x", then "how x was reached"). Literal steps carry the length
//     of the literal run that ends there, so the walk back from the block's end takes one step per sequence, through 4096-entry
//     windows staged in LDS; match ends are marked in a bitmap and the emitter turns 64 of them at a time into tokens, offsets,
//     varints and literal runs (the layout zxc_encode_kernel.hip assembles afterwards is unchanged).
#define OPT_MAX_BLOCK 131072u  // blocks up to this size: the bitmap of match ends (one bit per position) lives in the chain ring's 32 KiB
                               // of LDS. Larger blocks (256 KiB - 2 MiB) keep the lazy parse with two probes.
#define OPT_W 4096u         // positions in the DP window
#define OPT_LCAP 4080u      // longest candidate length the DP relaxes
#define OPT_LONG_SKIP 256u  // ZXC_OPT_LONG_MATCH_SKIP
#define OPT_INF 0xFFFFFFFFFFFFFFFFull
#define OPT_CHUNK 60u       // positions per prefetched piece of mp[]: 12 batches of 5
#define OPT_MATCH_BASE 24u  // ZXC_OPT_MATCH_COST_BASE
// ds_min_u64 without a return value (the returning form is waited for)
#ifdef ZXC_LDS_HOOKS  // (the CPU emulator build)
#define OPT_LDS_MIN64(p, v) do { if ((v) < *(p)) *(p) = (v); } while (0)
#else
#define OPT_LDS_MIN64(p, v) ((void)__hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#endif

// LDS traffic between the lanes of the one wave: DS instructions of a wave execute in program order, only the compiler must keep it
// (a workgroup-scope fence drains the LDS queue with s_waitcnt lgkmcnt(0) in every DP batch)
__device__ __forceinline__ void opt_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// log2(v) in 1/1024ths (v >= 1): integer part from the leading bit, ten fraction bits by repeated squaring — integer arithmetic
// only, so that the device and the CPU emulator price a block alike.
__device__ __forceinline__ uint32_t opt_log2_q10(uint32_t v) {
    const uint32_t n = 31u - (uint32_t)__builtin_clz(v);
    uint64_t m = ((uint64_t)v << 31) >> n;  // mantissa in [1, 2) as Q31
    uint32_t frac = 0;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        m = (m * m) >> 31;
        frac <<= 1;
        if (m >= (2ull << 31)) { m >>= 1; frac |= 1u; }
    }
    return (n << 10) | frac;
}

// The block's literal price in bits (1..8): entropy of a strided 4096-byte sample, rounded up. (The reference builds the
// length-limited Huffman code of the same sample and rounds its average length up, zxc_compress.c:720-753; a Huffman code's
// average is within a few hundredths of a bit of the entropy on such samples — 0.05 bit is added before rounding.)
__device__ __forceinline__ uint32_t opt_lit_cost(const uint8_t* __restrict__ blk, uint32_t nblk, uint32_t* __restrict__ hist, int lane) {
    if (nblk < 1024u) return 8u;  // ZXC_OPT_LIT_SAMPLE_MIN
    for (uint32_t i = lane; i < 256u; i += 64u) hist[i] = 0u;
    enc_lds_fence();
    const uint32_t step = nblk > 4096u ? nblk >> 12 : 1u;
    uint32_t sampled = 0;
    for (uint32_t i0 = 0; i0 < nblk; i0 += 64u * step) {
        const uint32_t i = i0 + step * (uint32_t)lane;
        if (i < nblk) atomicAdd(&hist[blk[i]], 1u);
        const uint32_t left = (nblk - i0 + step - 1u) / step;
        sampled += left < 64u ? left : 64u;
    }
    enc_lds_fence();
    uint64_t acc = 0;  // sum of f * log2 f, Q10
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t f = hist[4 * lane + k];
        if (f) acc += (uint64_t)f * opt_log2_q10(f);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)acc, d), hi = __shfl_xor((uint32_t)(acc >> 32), d);
        acc += ((uint64_t)hi << 32) | lo;
    }
    enc_lds_fence();
    // H = log2(sampled) - acc / sampled  (Q10), + 0.05 bit, rounded up
    const uint64_t hq = (uint64_t)opt_log2_q10(sampled) * sampled;
    const uint32_t h_q10 = (uint32_t)((hq > acc ? hq - acc : 0ull) / sampled);
    uint32_t bits = (h_q10 + 51u + 1023u) >> 10;
    if (bits < 1u) bits = 1u;
    return bits > 8u ? 8u : bits;
}

// dp over mp[0 .. nblk): in: mp[x] = length | distance << 16 of the longest match at x (0: none); out: mp[x], x in [1, nblk] = how x
// is reached: (0xFFFF - length) << 16 | distance for a match, 0xFFFF0000 | run for the last of `run` consecutive literals.
__device__ void opt_dp(uint32_t* __restrict__ mp, uint32_t nblk, uint32_t lit, unsigned long long* __restrict__ W, int lane) {
    for (uint32_t i = lane; i < OPT_W; i += 64u) W[i] = OPT_INF;
    enc_lds_fence();
    const uint32_t g = (uint32_t)lane / 12u, t = (uint32_t)lane - 12u * g;  // pushes: 12 lanes per position of the batch (lanes 60-63 idle)
    uint32_t dprev = 0xFFFFFFFFu, prun = 0u;  // dp and literal-run length of the position in front of the batch
    uint32_t c0 = 0;
    uint32_t mcur = ((uint32_t)lane < OPT_CHUNK && (uint32_t)lane < nblk) ? mp[lane] : 0u;
    while (c0 <= nblk) {
        const uint32_t xn = c0 + OPT_CHUNK + (uint32_t)lane;  // the next piece, requested a dozen batches ahead
        const uint32_t mnext = ((uint32_t)lane < OPT_CHUNK && xn < nblk) ? mp[xn] : 0u;
        for (uint32_t q = 0; q < OPT_CHUNK && c0 + q <= nblk; q += 5u) {
            const uint32_t p0 = c0 + q;
            // ---- the batch's five entries; their slots are free for positions + 4096 at once (pushes reach at most + 4084)
            const uint32_t x = p0 + (uint32_t)lane;
            unsigned long long e = OPT_INF;
            if (lane < 5 && x <= nblk) {
                e = W[x & (OPT_W - 1u)];
                W[x & (OPT_W - 1u)] = OPT_INF;
            }
            const uint32_t ehi = (uint32_t)(e >> 32), elo = (uint32_t)e;
            // ---- literal chain (scalar): dp[x] = min(pushed, dp[x - 1] + lit), a match wins a tie
            uint32_t d[5], lo[5], mi[5];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const uint32_t hk = (uint32_t)__builtin_amdgcn_readlane((int)ehi, k), lk = (uint32_t)__builtin_amdgcn_readlane((int)elo, k);
                mi[k] = (uint32_t)__builtin_amdgcn_readlane((int)mcur, (int)(q + (uint32_t)k));
                if (p0 + (uint32_t)k == 0u) { d[k] = 0u; lo[k] = 0u; prun = 0u; }
                else {
                    const uint32_t via = dprev == 0xFFFFFFFFu ? 0xFFFFFFFFu : dprev + lit;
                    if (via < hk) { prun = prun < 0xFFFFu ? prun + 1u : 0xFFFFu; d[k] = via; lo[k] = 0xFFFF0000u | prun; }
                    else { prun = 0u; d[k] = hk; lo[k] = lk; }
                }
                dprev = d[k];
            }
            if (lane < 5 && x >= 1u && x <= nblk) {
                const uint32_t v = lane == 0 ? lo[0] : lane == 1 ? lo[1] : lane == 2 ? lo[2] : lane == 3 ? lo[3] : lo[4];
                mp[x] = v;
            }
            // ---- the five positions' matches, every length of each: one ds_min per candidate
            const uint32_t gm = g == 0u ? mi[0] : g == 1u ? mi[1] : g == 2u ? mi[2] : g == 3u ? mi[3] : g == 4u ? mi[4] : 0u;
            const uint32_t gd = g == 0u ? d[0] : g == 1u ? d[1] : g == 2u ? d[2] : g == 3u ? d[3] : d[4];
            const uint32_t gx = p0 + g;
            uint32_t lmax = gm & 0xFFFFu;
            if (g >= 5u || gx >= nblk || lmax < 5u) lmax = 0u;
            if (lmax > OPT_LCAP) lmax = OPT_LCAP;
            if (lmax > nblk - (gx < nblk ? gx : nblk)) lmax = nblk - (gx < nblk ? gx : nblk);
            const uint32_t dist = gm >> 16;
            for (uint32_t L = 5u + t;; L += 12u) {
                const bool act = L <= lmax;
                if (__ballot(act) == 0ull) break;
                if (act) {
                    const uint32_t v = L - 5u;
                    const uint32_t cost = OPT_MATCH_BASE + (v >= 15u ? 8u * (1u + (v - 15u >= 128u ? 1u : 0u) + (v - 15u >= 16384u ? 1u : 0u)) : 0u);
                    const unsigned long long key = ((unsigned long long)(gd + cost) << 32) | ((0xFFFFu - L) << 16) | dist;
                    OPT_LDS_MIN64(&W[(gx + L) & (OPT_W - 1u)], key);
                }
            }
            opt_fence();
        }
        mcur = mnext;
        c0 += OPT_CHUNK;
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // mp[] is read back by the walk below
}

// Walks the parents from the block's end to its start through LDS windows of 4096 entries; sets bit x of ends[] for every position
// x at which a chosen match ends (ends: (nblk >> 5) + 1 words).
__device__ void opt_backtrack(const uint32_t* __restrict__ mp, uint32_t nblk, uint32_t* __restrict__ win, uint32_t* __restrict__ ends, int lane) {
    for (uint32_t i = lane; i <= (nblk >> 5); i += 64u) ends[i] = 0u;
    enc_lds_fence();
    uint32_t pos = nblk;
    while (pos > 0u) {
        const uint32_t wb = pos >= OPT_W - 1u ? pos - (OPT_W - 1u) : 0u;  // window [wb, pos]
        for (uint32_t i = lane; i <= pos - wb; i += 64u) win[i] = (wb + i) >= 1u ? mp[wb + i] : 0u;
        enc_lds_fence();
        while (pos > 0u && pos >= wb) {
            const uint32_t e = uni(win[pos - wb]);
            const uint32_t len = 0xFFFFu - (e >> 16);
            if (len == 0u) {
                uint32_t run = e & 0xFFFFu;
                if (run == 0u || run > pos) run = run == 0u ? 1u : pos;  // (never: a guard against walking past the start)
                pos -= run;
            } else {
                if (lane == 0) ends[pos >> 5] |= 1u << (pos & 31u);
                pos -= len <= pos ? len : pos;
            }
        }
        enc_lds_fence();
    }
}

// Sequences from the marked match ends, 64 at a time: tokens, 16-bit offsets and varints into their staging areas, literal runs into
// lit_out; then the block's trailing literals. blk = the block's first byte; list = LDS room for one pass' match ends (4096
// positions hold at most 820). Returns false when a staging area would overflow (the caller stores the block RAW).
struct OptOut {
    uint32_t seq_count, lit_count, ext_count, max_off;
};
__device__ bool opt_emit(const uint8_t* __restrict__ blk, const uint32_t* __restrict__ mp, uint32_t nblk, const uint32_t* __restrict__ ends,
                         uint32_t* __restrict__ list, uint8_t* __restrict__ tok_st, uint8_t* __restrict__ off_st, uint8_t* __restrict__ ext_st,
                         uint8_t* __restrict__ lit_out, uint32_t max_seq, uint32_t ext_cap, OptOut& o, int lane) {
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint32_t seq_count = 0, lit_count = 0, ext_count = 0, max_off = 0;
    uint32_t lit_start = 0;  // end of the last emitted match
    const uint32_t n_words = (nblk >> 5) + 1u;
    for (uint32_t base = 0; base <= nblk; base += 4096u) {
        // ---- this pass' match ends, in order, into list[]
        const uint32_t w0 = (base >> 5) + 2u * (uint32_t)lane;
        uint32_t blo = w0 < n_words ? ends[w0] : 0u, bhi = w0 + 1u < n_words ? ends[w0 + 1u] : 0u;
        const uint32_t cnt = (uint32_t)__popc(blo) + (uint32_t)__popc(bhi);
        const uint32_t incl = wave_scan_add(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        uint32_t at = incl - cnt;
        while (blo) { list[at++] = base + 64u * (uint32_t)lane + (uint32_t)__builtin_ctz(blo); blo &= blo - 1u; }
        while (bhi) { list[at++] = base + 64u * (uint32_t)lane + 32u + (uint32_t)__builtin_ctz(bhi); bhi &= bhi - 1u; }
        enc_lds_fence();
        for (uint32_t s0 = 0; s0 < total; s0 += 64u) {
            const uint32_t j = s0 + (uint32_t)lane;
            const bool has = j < total;
            const uint32_t nsel = total - s0 < 64u ? total - s0 : 64u;
            const uint32_t end = has ? list[j] : 0u;
            const uint32_t e = has ? mp[end] : 0xFFFF0000u;
            const uint32_t L = 0xFFFFu - (e >> 16), dist = e & 0xFFFFu;
            const uint32_t start = end - L;
            uint32_t prev_end = (uint32_t)__shfl_up((int)end, 1);
            if (lane == 0) prev_end = lit_start;
            const uint32_t ll = has ? start - prev_end : 0u;
            const uint32_t mlm = has ? L - 5u : 0u;
            uint32_t eb = 0;
            if (has) eb = (ll >= 15u ? varint_len(ll - 15u) : 0u) + (mlm >= 15u ? varint_len(mlm - 15u) : 0u);
            const uint32_t eincl = wave_scan_add(eb);
            const uint32_t etot = (uint32_t)__builtin_amdgcn_readlane((int)eincl, 63);
            const uint32_t lincl = wave_scan_add(ll);
            const uint32_t ltot = (uint32_t)__builtin_amdgcn_readlane((int)lincl, 63);
            if (seq_count + nsel > max_seq || ext_count + etot > ext_cap) return false;
            if (has) {
                const uint32_t sidx = seq_count + (uint32_t)lane;
                tok_st[sidx] = (uint8_t)(((ll < 15u ? ll : 15u) << 4) | (mlm < 15u ? mlm : 15u));
                const uint16_t o16 = (uint16_t)(dist - 1u);
                __builtin_memcpy(off_st + 2u * sidx, &o16, 2);
                uint8_t* x = ext_st + ext_count + eincl - eb;
                if (ll >= 15u) { put_varint(x, ll - 15u); x += varint_len(ll - 15u); }
                if (mlm >= 15u) put_varint(x, mlm - 15u);
            }
            if (__ballot(has && dist > 256u)) max_off = 65535u;
            else if (max_off == 0u) max_off = 1u;
            // literal runs: short ones lane by lane (a byte per step), long ones by the whole wave
            {
                uint8_t* lp = lit_out + lit_count + lincl - ll;
                // (both 16-byte pieces of every run are requested first and the bytes stored from registers: a byte loop of dependent
                // loads waited 2 us per byte. Runs within 32 bytes of the block's end take the whole-wave path below.)
                const bool fastok = has && prev_end + 32u <= nblk;
                const uint8_t* sp = blk + (fastok ? prev_end : 0u);
                const bool shortrun = fastok && ll != 0u && ll <= 32u;
                const v4u a0 = ld128(nblk >= 32u ? sp : blk), a1 = ld128(nblk >= 32u ? sp + 16 : blk);
                const uint32_t wv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
                for (uint32_t k = 0; k < 32u; k++) {
                    if (__ballot(shortrun && k < ll) == 0ull) break;
                    if (shortrun && k < ll) lp[k] = (uint8_t)(wv[k >> 2] >> (8u * (k & 3u)));
                }
                uint64_t lm = __ballot(has && ll != 0u && !shortrun);
                while (lm) {
                    const int q = __builtin_ctzll(lm);
                    lm &= lm - 1ull;
                    const uint32_t qll = (uint32_t)__builtin_amdgcn_readlane((int)ll, q), qpe = (uint32_t)__builtin_amdgcn_readlane((int)prev_end, q),
                                   qat = (uint32_t)__builtin_amdgcn_readlane((int)(lincl - ll), q);
                    for (uint32_t k = lane; k < qll; k += 64u) lit_out[lit_count + qat + k] = blk[qpe + k];
                }
            }
            (void)lt_mask;
            seq_count += nsel;
            ext_count += etot;
            lit_count += ltot;
            lit_start = (uint32_t)__builtin_amdgcn_readlane((int)end, (int)(nsel - 1u));
        }
        enc_lds_fence();
    }
    for (uint32_t k = lit_start + (uint32_t)lane; k < nblk; k += 64u) lit_out[lit_count + (k - lit_start)] = blk[k];  // trailing literals
    lit_count += nblk - lit_start;
    o.seq_count = seq_count;
    o.lit_count = lit_count;
    o.ext_count = ext_count;
    o.max_off = max_off;
    return true;
}
