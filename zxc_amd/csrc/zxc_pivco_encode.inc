// zxc_pivco_encode.inc — PivCo (level-ordered canonical Huffman) section ENCODE for one wavefront.
// Included by zxc_encode_kernel.hip (levels 6-7: literal section, level 7 also the token section).
// Reference being replaced: zxc_huf_build_code_lengths (boundary package-merge, src/lib/zxc_huffman.c:72-340),
// zxc_huf_encode_section / the PivCo writer (:1257-1342); wire format docs/FORMAT.md §5.2.1: 128 bytes of 4-bit
// code lengths, then one run per emitting node of the canonical code tree in BFS order — a bitmap node's run has
// one branch bit per symbol routed through it, a flat root's run D packed bits per symbol.
//
// The decoder (zxc_pivco.inc) merges bottom-up; the encoder is its mirror image, a level-by-level STABLE PARTITION:
//   1. histogram with LDS atomics; Huffman code lengths by 255 wave-wide two-minima reductions over an LDS node
//      table (leaf depth = hops to the root), limited to 11 bits by a Kraft repair (lengthen the deepest codes that
//      are not at the limit, then give the slack back to the most frequent ones);
//   2. canonical codes and the implicit tree (per-depth leaf / node counts give every node by arithmetic, flat
//      roots derived from the lengths exactly like the decoder derives them); per-node symbol counts from the
//      histogram (a symbol's node at depth d is a prefix of its code), run offsets and level-buffer offsets by
//      wave prefix sums -> the section size is known BEFORE a single run is written (the caller's size decision);
//   3. for every depth, every emitting node: 64 symbols per step, ballot of the code bit = the next 8 bytes of the
//      node's run; prefix popcounts scatter the symbols into the children's sequences of the next level buffer
//      (leaf children are dropped); flat roots pack bit-reversed code tails through a small LDS bit buffer.

#define PE_MAXLEN 11
struct PivEnc {  // overlays the match finder's hash tables (dead once the block is parsed)
    uint32_t freq[256];
    uint32_t weight[512];  // Huffman build: leaves 0..255, internal nodes 256.. in creation order; 0xFFFFFFFF = not alive
    uint16_t parent[512];
    uint16_t code[256];
    uint8_t len[256];
    uint8_t sorted[256];   // symbols ordered by (length, symbol)
    uint32_t cnt[256];     // symbols routed through internal node ii
    uint32_t runoff[256];  // bits 0-23: byte offset of the node's run in the body; 24-27: flat depth D; bit 31: covered by a flat ancestor
    uint32_t seqoff[256];  // offset of the node's sequence in its depth's level buffer
    uint32_t first[PE_MAXLEN + 2], L[PE_MAXLEN + 2], N[PE_MAXLEN + 2], ib[PE_MAXLEN + 2], fc[PE_MAXLEN + 2];
    uint32_t bitbuf[24];   // flat-root packing of one 64-symbol step (<= 64 * 11 bits)
};

__device__ __forceinline__ void pe_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t pe_total(uint32_t incl) { return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63); }

// Encodes sym[0..n) into out (128-byte length table + runs). tmpA / tmpB: n bytes of scratch each. Returns the section
// size, or 0 when it would not be smaller than `budget` bytes (nothing usable is written then).
__device__ uint32_t pivco_encode(const uint8_t* __restrict__ sym, uint32_t n, uint8_t* __restrict__ out, uint32_t budget,
                                 uint8_t* __restrict__ tmpA, uint8_t* __restrict__ tmpB, PivEnc& P, int lane) {
    if (n == 0u || budget <= 129u) return 0u;
    // ---- 1. histogram
    for (uint32_t i = lane; i < 256u; i += 64u) P.freq[i] = 0u;
    pe_fence();
    for (uint32_t i0 = 0; i0 < n; i0 += 256u) {  // (four loads in flight)
        uint32_t sv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const uint32_t i = i0 + 64u * (uint32_t)u + (uint32_t)lane; sv[u] = sym[i < n ? i : 0u]; }
#pragma unroll
        for (int u = 0; u < 4; u++) if (i0 + 64u * (uint32_t)u + (uint32_t)lane < n) atomicAdd(&P.freq[sv[u]], 1u);
    }
    pe_fence();
    uint32_t myf[4];
    uint32_t mine_present = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { myf[k] = P.freq[4 * lane + k]; mine_present += myf[k] != 0u; }
    const uint32_t present = wave_sum(mine_present);
    uint32_t myl[4] = {0, 0, 0, 0};
    if (present == 1u) {
        // degenerate table: one symbol of code length 1, the root's run is n zero bits (docs/FORMAT.md §5.2.1)
        const uint32_t nb = (n + 7u) >> 3;
        if (128u + nb >= budget) return 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) myl[k] = myf[k] ? 1u : 0u;
        const uint32_t two = myl[0] | (myl[1] << 4) | (myl[2] << 8) | (myl[3] << 12);
        out[2 * lane] = (uint8_t)two;
        out[2 * lane + 1] = (uint8_t)(two >> 8);
        for (uint32_t i = lane; i < nb; i += 64u) out[128u + i] = 0;
        return 128u + nb;
    }
    // ---- 2. Huffman code lengths: repeatedly join the two lightest live nodes
    for (uint32_t i = lane; i < 512u; i += 64u) {
        P.weight[i] = (i < 256u && P.freq[i]) ? P.freq[i] : 0xFFFFFFFFu;
        P.parent[i] = 0xFFFFu;
    }
    pe_fence();
    for (uint32_t t = 0; t + 1u < present; t++) {
        const uint32_t newid = 256u + t;
        uint32_t wsum = 0;
#pragma unroll 1
        for (int r = 0; r < 2; r++) {
            uint64_t best = ~0ull;
            for (uint32_t i = lane; i < newid; i += 64u) {  // (ties: lowest index, so the result is deterministic)
                const uint64_t key = ((uint64_t)P.weight[i] << 16) | i;
                best = key < best ? key : best;
            }
            best = wave_min(best);
            const uint32_t idx = (uint32_t)best & 0xFFFFu;
            wsum += (uint32_t)(best >> 16);
            if (lane == 0) {
                P.weight[idx] = 0xFFFFFFFFu;  // taken
                P.parent[idx] = (uint16_t)newid;
            }
            pe_fence();
        }
        if (lane == 0) P.weight[newid] = wsum;
        pe_fence();
    }
    // leaf depth = hops to the root
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t d = 0;
        if (myf[k]) {
            uint32_t q = 4u * (uint32_t)lane + (uint32_t)k;
            while (P.parent[q] != 0xFFFFu) { q = P.parent[q]; d++; }
        }
        myl[k] = d;
    }
    // ---- limit to PE_MAXLEN bits: Kraft repair (the reference runs a package-merge; any Kraft-exact table is a valid section)
    {
        uint32_t over = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) if (myl[k] > PE_MAXLEN) { myl[k] = PE_MAXLEN; over = 1; }
        if (__ballot(over != 0u)) {
            auto kraft = [&]() -> uint32_t {
                uint32_t s = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) if (myl[k]) s += 1u << (PE_MAXLEN - myl[k]);
                return wave_sum(s);
            };
            uint32_t K = kraft();
            while (K > (1u << PE_MAXLEN)) {  // lengthen the deepest code that is not at the limit (rarest first)
                uint64_t best = ~0ull;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (myl[k] && myl[k] < PE_MAXLEN) {
                        const uint64_t key = ((uint64_t)(PE_MAXLEN - myl[k]) << 48) | ((uint64_t)myf[k] << 16) | (4u * lane + k);
                        best = key < best ? key : best;
                    }
                best = wave_min(best);
                const uint32_t idx = (uint32_t)best & 0xFFFFu;
#pragma unroll
                for (int k = 0; k < 4; k++) if (4u * (uint32_t)lane + (uint32_t)k == idx) myl[k]++;
                K = kraft();
            }
            while (K < (1u << PE_MAXLEN)) {  // give the slack back: shorten the most frequent code whose step still fits
                const uint32_t slack = (1u << PE_MAXLEN) - K;
                uint64_t best = ~0ull;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (myl[k] > 1u && (1u << (PE_MAXLEN - myl[k])) <= slack) {
                        const uint64_t key = ((uint64_t)(0xFFFFFFFFu - myf[k]) << 16) | (4u * lane + k);
                        best = key < best ? key : best;
                    }
                best = wave_min(best);  // (a code at the limit always fits a slack >= 1, so one is found)
                const uint32_t idx = (uint32_t)best & 0xFFFFu;
#pragma unroll
                for (int k = 0; k < 4; k++) if (4u * (uint32_t)lane + (uint32_t)k == idx) myl[k]--;
                K = kraft();
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) P.len[4 * lane + k] = (uint8_t)myl[k];
    // ---- 3. canonical codes: symbols ordered by (length, symbol); codes consecutive, shifted left when the length grows
    uint32_t blc[PE_MAXLEN + 1];
    uint32_t maxlen = 0, run_first = 0, fcv = 0;
    blc[0] = 0;
    uint32_t myc[4] = {0, 0, 0, 0};
    if (lane == 0) P.fc[0] = 0;
#pragma unroll
    for (int l = 1; l <= PE_MAXLEN; l++) {
        const uint32_t mine = (myl[0] == (uint32_t)l) + (myl[1] == (uint32_t)l) + (myl[2] == (uint32_t)l) + (myl[3] == (uint32_t)l);
        const uint32_t incl = wave_scan_add(mine);
        const uint32_t tot = pe_total(incl);
        blc[l] = tot;
        if (tot) maxlen = l;
        fcv = (fcv + blc[l - 1]) << 1;  // first code of length l
        uint32_t at = incl - mine;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (myl[k] == (uint32_t)l) { P.sorted[run_first + at] = (uint8_t)(4 * lane + k); myc[k] = fcv + at; at++; }
        if (lane == 0) { P.first[l] = run_first; P.fc[l] = fcv; }
        run_first += tot;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) P.code[4 * lane + k] = (uint16_t)myc[k];
    // implicit level structure (as zxc_pivco.inc): nodes / leaves per depth, first internal index
    {
        uint32_t I = 1, ibase = 0;
        if (lane == 0) { P.N[0] = 1; P.L[0] = 0; P.ib[0] = 0; }
#pragma unroll
        for (int d = 1; d <= PE_MAXLEN; d++) {
            const bool in = (uint32_t)d <= maxlen;
            const uint32_t Nd = in ? 2u * I : 0u;
            const uint32_t Ld = in ? blc[d] : 0u;
            ibase += I;
            if (lane == 0) { P.N[d] = Nd; P.L[d] = Ld; P.ib[d] = ibase; }
            I = Nd - Ld;
        }
        if (lane == 0) { P.N[PE_MAXLEN + 1] = 0; P.L[PE_MAXLEN + 1] = 0; P.ib[PE_MAXLEN + 1] = ibase; }
    }
    pe_fence();
    // flat roots: maximal complete subtrees of depth >= 2; their strict descendants emit nothing
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Ld = P.L[d], Id = P.N[d] - P.L[d], Bi = P.ib[d];
        const uint32_t Bp = d ? P.ib[d - 1] : 0u;
        for (uint32_t j = lane; j < Id; j += 64u) {
            const uint32_t i = Ld + j;
            uint32_t cov = 0;
            if (d > 0u) cov = (P.runoff[Bp + (i >> 1)] & 0x8F000000u) != 0u;
            uint32_t fd = 0;
            if (!cov) {
                uint32_t lo = 2u * j, hi = lo + 2u;
                for (uint32_t r = 1; d + r <= maxlen; r++) {
                    const uint32_t Lr = P.L[d + r];
                    if (hi <= Lr) { fd = r; break; }
                    if (lo < Lr) break;
                    lo = 2u * (lo - Lr);
                    hi = 2u * (hi - Lr);
                }
                if (fd < 2u) fd = 0;
            }
            P.runoff[Bi + j] = (fd << 24) | (cov ? 0x80000000u : 0u);
            P.cnt[Bi + j] = 0;
        }
        pe_fence();
    }
    // symbols routed through every internal node: a symbol's node at depth d is the d-bit prefix of its code
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!myf[k]) continue;
        for (uint32_t d = 0; d < myl[k]; d++) {
            const uint32_t i = (myc[k] >> (myl[k] - d)) - P.fc[d];  // node index within depth d (0 at the root)
            atomicAdd(&P.cnt[P.ib[d] + i - P.L[d]], myf[k]);
        }
    }
    pe_fence();
    // ---- run offsets (BFS order) and level-buffer offsets; the section size is known here
    uint32_t pcur = 0;
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d];
        uint32_t acc = 0;
        for (uint32_t j0 = 0; j0 < Id; j0 += 64u) {
            const uint32_t j = j0 + (uint32_t)lane;
            const bool have = j < Id;
            const uint32_t ii = Bi + (have ? j : 0u);
            const uint32_t nf = P.runoff[ii];
            const bool emit = have && !(nf & 0x80000000u);
            const uint32_t c = emit ? P.cnt[ii] : 0u;
            const uint32_t D = (nf >> 24) & 15u;
            const uint32_t nbytes = emit ? (D ? (uint32_t)(((uint64_t)c * D + 7u) >> 3) : ((c + 7u) >> 3)) : 0u;
            const uint32_t incl = wave_scan_add(nbytes);
            if (emit) P.runoff[ii] = nf | (pcur + incl - nbytes);
            pcur += pe_total(incl);
            const uint32_t sincl = wave_scan_add(c);
            if (emit) P.seqoff[ii] = acc + sincl - c;
            acc += pe_total(sincl);
        }
    }
    pe_fence();
    const uint32_t total = 128u + pcur;
    if (total >= budget) return 0u;

    // ---- 4. write: length table, then the runs, one depth at a time
    {
        const uint32_t two = myl[0] | (myl[1] << 4) | (myl[2] << 8) | (myl[3] << 12);
        out[2 * lane] = (uint8_t)two;
        out[2 * lane + 1] = (uint8_t)(two >> 8);
    }
    uint8_t* body = out + 128;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint8_t* cur = d == 0 ? sym : ((d & 1u) ? tmpA : tmpB);
        uint8_t* nxt = (d & 1u) ? tmpB : tmpA;
        const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d], Bc = P.ib[d + 1], Lc = P.L[d + 1];
        for (uint32_t j = 0; j < Id; j++) {
            const uint32_t nf = P.runoff[Bi + j];
            if (nf & 0x80000000u) continue;
            const uint32_t c = P.cnt[Bi + j], so = P.seqoff[Bi + j], D = (nf >> 24) & 15u;
            uint8_t* run = body + (nf & 0xFFFFFFu);
            if (D == 0u) {
                const uint32_t c0 = 2u * j, c1 = c0 + 1u;
                const bool m0 = c0 >= Lc, m1 = c1 >= Lc;  // internal children keep their sequences (leaves are dropped)
                uint8_t* q0 = nxt + (m0 ? P.seqoff[Bc + c0 - Lc] : 0u);
                uint8_t* q1 = nxt + (m1 ? P.seqoff[Bc + c1 - Lc] : 0u);
                uint32_t b0 = 0, b1 = 0;
                for (uint32_t k1 = 0; k1 < c; k1 += 256u) {  // four 64-symbol steps per round: their loads are requested together
                    uint32_t sv[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t kk = k1 + 64u * (uint32_t)u + (uint32_t)lane;
                        sv[u] = cur[so + (kk < c ? kk : 0u)];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t k0 = k1 + 64u * (uint32_t)u;
                        if (k0 >= c) break;
                        const uint32_t left = c - k0;
                        const bool valid = (uint32_t)lane < left;
                        const uint32_t s = sv[u];
                        const bool bit = valid && ((P.code[s] >> (P.len[s] - 1u - d)) & 1u);
                        const uint64_t mask = __ballot(bit);
                        const uint32_t nb = ((left < 64u ? left : 64u) + 7u) >> 3;
                        if ((uint32_t)lane < nb) run[(k0 >> 3) + lane] = (uint8_t)(mask >> (8 * lane));
                        const uint32_t below = __popcll(mask & lt_mask);
                        if (valid) {
                            if (bit) { if (m1) q1[b1 + below] = (uint8_t)s; }
                            else if (m0) q0[b0 + ((uint32_t)lane - below)] = (uint8_t)s;
                        }
                        const uint32_t tot1 = __popcll(mask);
                        b1 += tot1;
                        b0 += (left < 64u ? left : 64u) - tot1;
                    }
                }
            } else {
                // flat root: D bits per symbol, bit j = branch at relative depth j = the code's tail read MSB first
                for (uint32_t k0 = 0; k0 < c; k0 += 64u) {
                    const uint32_t left = c - k0;
                    const uint32_t cntg = left < 64u ? left : 64u;
                    const bool valid = (uint32_t)lane < cntg;
                    if (lane < 24) P.bitbuf[lane] = 0u;
                    pe_fence();
                    if (valid) {
                        const uint32_t s = cur[so + k0 + lane];
                        const uint32_t tail = P.code[s] & ((1u << D) - 1u);
                        const uint32_t v = __builtin_bitreverse32(tail) >> (32u - D);
                        const uint32_t bp = (uint32_t)lane * D;
                        atomicOr(&P.bitbuf[bp >> 5], v << (bp & 31u));
                        if ((bp & 31u) + D > 32u) atomicOr(&P.bitbuf[(bp >> 5) + 1u], v >> (32u - (bp & 31u)));
                    }
                    pe_fence();
                    const uint32_t nb = (cntg * D + 7u) >> 3;  // (<= 88)
                    uint8_t* o = run + ((uint64_t)k0 * D >> 3);
                    for (uint32_t q = lane; q < nb; q += 64u) o[q] = (uint8_t)(P.bitbuf[q >> 2] >> (8u * (q & 3u)));
                    pe_fence();
                }
            }
        }
        // the next depth reads what this one wrote (ordinary stores, cached loads)
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    return total;
}
