// zxc_pivco_dir.inc — PivCo sections decoded by a whole workgroup out of LDS (levels 6-7). Included by zxc_decode_kernel.hip
// after zxc_pivco.inc (whose piv_tree builds the implicit canonical tree). Reference behaviour: zxc_huf_decode_section
// (src/lib/zxc_huffman.c:2447-2457); format: docs/FORMAT.md §5.2.1.
//
// The one-wave decoder (zxc_pivco.inc) rebuilds a section bottom-up through level buffers in global memory: ~9 K L1 -> L2
// requests and ~110 K instructions per level-7 block, 85 % of that kernel's issue slots (profiles/r3s_l7_issue_counters.txt).
// This one keeps no level buffers at all. A PivCo section is a wavelet tree: every internal node's run is the bitmap that
// routes the node's symbols to its children, so the symbol at output position k is found by walking DOWN from the root:
//     at a bitmap node with run R:  bit = R[idx];  idx' = rank_bit(R, idx)  (ones / zeros in front of idx);  go to that child
//     at a flat root (complete subtree of depth D): the D-bit code at R[idx * D ..] names the leaf;  at a leaf: its symbol.
// Every position is independent of every other. What makes the walk cheap is a RANK DIRECTORY over the whole section body,
// tree or no tree: the body is staged in LDS as 64-bit words W[], cum[i] = ones in front of word i (mod 2^16: a node holds
// < 2^16 symbols), so rank(p) = cum[p >> 6] + popcount(W[p >> 6] below bit p & 63) is two LDS reads for ANY bit position p,
// and a node's rank is a difference of two of those. The directory also replaces pass 1's popcount loops: a bitmap node's
// ones = rank(end) - rank(start) tells its children's symbol counts, which give the next depth's run offsets.
//
// One workgroup per SECTION (a block's literal and token sections are two independent work items). Per section:
//   1  waves 1.. copy the body into W[] and prefix-sum its popcounts; wave 0 builds the tree from the 128-byte header
//   2  wave 0: run offsets + child counts, depth by depth (rank differences); waves 1..: the flat roots' code -> symbol tables
//   3  all: four walkers per thread, each over its own run of consecutive positions; a walker stores a dword per four symbols
// Global traffic: the section body in once, the decoded bytes out once.
// Steps 1-2 are chains of dependent LDS / memory round trips run by one or two waves (~30 us a section, measured on the first,
// 512-thread-only build: profiles/r3y_sections_kernel_trace_v1.log), so what a CU needs is MANY sections in flight: three
// builds of the same code by LDS footprint — small (128 threads, 8 KiB of body: every token section, short literal
// sections; ~10 workgroups per CU), medium (256 threads, 36 KiB; 3 per CU), large (512 threads, 56 KiB; 2 per CU) — each
// with its own work list, written by the launch-order pass (zxc_dev_sec_t: one 32-byte record per section).

#define PDIR_N_MAX 65535u  // symbols per section (16-bit ranks)
#define PDIR_BODY_OF(THREADS, ITERS) (8u * ((uint32_t)(ITERS) * ((uint32_t)(THREADS) - 64u) - 1u))
#define PDIR_SMALL_ITERS 16  // (PDIR_*_THREADS: zxc_kernels.h, the shim launches with them)
#define PDIR_MEDIUM_ITERS 24
#define PDIR_LARGE_ITERS 16
#define PDIR_SMALL_BODY PDIR_BODY_OF(PDIR_SMALL_THREADS, PDIR_SMALL_ITERS)      //  8184 bytes of section body
#define PDIR_MEDIUM_BODY PDIR_BODY_OF(PDIR_MEDIUM_THREADS, PDIR_MEDIUM_ITERS)   // 36856
#define PDIR_LARGE_BODY PDIR_BODY_OF(PDIR_LARGE_THREADS, PDIR_LARGE_ITERS)      // 57336

// size class of a section with `body` bytes behind its 128-byte header: 0 small, 1 medium, 2 large, 3 = the one-wave decoder
__device__ __forceinline__ uint32_t pdir_class(uint32_t body) {
    return body <= PDIR_SMALL_BODY ? 0u : body <= PDIR_MEDIUM_BODY ? 1u : body <= PDIR_LARGE_BODY ? 2u : 3u;
}

template <int THREADS, int ITERS>
struct PdirLds {
    static constexpr uint32_t kStagers = THREADS - 64;      // waves 1..
    static constexpr uint32_t kSlices = THREADS / 64 - 1;   // staging waves
    static constexpr uint32_t kWords = ITERS * kStagers;    // words of LDS for the body, the last one used a zero guard
    uint64_t W[kWords];            // the section body; W[nw] = 0 (rank of the body's end, and the flat codes' second dword)
    uint16_t cum[kWords];          // ones in W[0 .. i), mod 2^16
    uint32_t cnt[PIV_INT];         // symbols routed through the internal node
    uint32_t runoff[PIV_INT];      // bits 0-23: byte offset of the node's run in the body; 24-27: flat depth D or 0; bit 31: covered
    uint16_t rank0[PIV_INT];       // rank of the run's first bit
    uint16_t c2sb[PIV_INT];        // flat root: first entry of its code -> symbol table in c2s[]
    uint64_t nrec[PIV_INT];        // the walk's view of a node, one LDS read (pdir_records)
    uint8_t len[256];
    uint8_t sorted[256];           // symbols ordered by (length, symbol)
    uint8_t c2s[256];              // all flat roots' tables (their leaves are disjoint: <= 256 entries)
    uint32_t first[PIV_MAXLEN + 2], L[PIV_MAXLEN + 2], N[PIV_MAXLEN + 2], ib[PIV_MAXLEN + 2];
    uint32_t wsum[ITERS * kSlices]; // staging: popcount of each (round, wave) slice, then its exclusive prefix
    int32_t rc_tree, rc_pass1;
    uint32_t maxlen, single;       // single: 0 = a real tree, 1 = the one-symbol table, 2 = a malformed one
    uint32_t item;
};

template <typename PL>
__device__ __forceinline__ uint32_t pdir_rank(const PL& P, uint32_t p) {  // ones in body bits [0, p), mod 2^16 (p <= 8 * body size)
    const uint32_t w = p >> 6;
    return (uint32_t)P.cum[w] + (uint32_t)__popcll(P.W[w] & ((1ull << (p & 63u)) - 1ull));
}

// Wave 0: run offsets and child counts, top-down. Returns 0 or E_CORRUPT (a run outside the body).
template <typename PL>
__device__ __forceinline__ int pdir_pass1(PL& P, int lane, uint32_t n, uint32_t bsize, uint32_t maxlen) {
    if (lane == 0) P.cnt[0] = n;
    wave_lds_fence();
    uint32_t pcur = 0;
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d], Bc = P.ib[d + 1], Lc = P.L[d + 1];
        for (uint32_t j0 = 0; j0 < Id; j0 += 64u) {
            const uint32_t j = j0 + lane;
            const bool have = j < Id;
            const uint32_t ii = Bi + (have ? j : 0u);
            const uint32_t nf = P.runoff[ii];
            const bool emit = have && !(nf & 0x80000000u);
            const uint32_t c = emit ? P.cnt[ii] : 0u;
            const uint32_t D = emit ? ((nf >> 24) & 15u) : 0u;
            const uint32_t nbytes = emit ? (D ? (uint32_t)(((uint64_t)c * D + 7u) >> 3) : ((c + 7u) >> 3)) : 0u;
            const uint32_t incl = wave_scan_add(nbytes);
            const uint32_t ro = pcur + incl - nbytes;
            if (__ballot(emit && (ro > bsize || nbytes > bsize - ro))) return E_CORRUPT;
            pcur += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (emit) {
                const uint32_t r0 = pdir_rank(P, 8u * ro);
                P.runoff[ii] = nf | ro;
                P.rank0[ii] = (uint16_t)r0;
                if (D == 0u) {  // children 2j, 2j+1 of depth d+1: only internal ones keep a count
                    const uint32_t ones = (pdir_rank(P, 8u * ro + c) - r0) & 0xFFFFu;
                    const uint32_t c0 = 2u * j, c1 = c0 + 1u;
                    if (c0 >= Lc) P.cnt[Bc + c0 - Lc] = c - ones;
                    if (c1 >= Lc) P.cnt[Bc + c1 - Lc] = ones;
                }
            }
        }
        wave_lds_fence();
    }
    return 0;
}

// Waves 1..: code -> symbol tables of every flat root, packed into c2s[] in node order; table wave `tw` of `ntw` fills every
// ntw-th flat root (all of them run the same prefix sum of the table sizes).
template <typename PL>
__device__ __forceinline__ void pdir_tables(PL& P, int lane, uint32_t maxlen, uint32_t tw, uint32_t ntw) {
    uint32_t tb = 0, nflat = 0;
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d];
        for (uint32_t j0 = 0; j0 < Id; j0 += 64u) {
            const uint32_t j = j0 + lane;
            const bool have = j < Id;
            const uint32_t nf = P.runoff[Bi + (have ? j : 0u)];  // (wave 0 is filling in the offset bits meanwhile: the flags do not change)
            const uint32_t D = (have && !(nf & 0x80000000u)) ? ((nf >> 24) & 15u) : 0u;
            const uint32_t size = D ? 1u << D : 0u;
            const uint32_t incl = wave_scan_add(size);
            const uint32_t base = tb + incl - size;
            if (D && tw == 0u) P.c2sb[Bi + j] = (uint16_t)base;
            tb += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            uint64_t flats = __ballot(D != 0u);
            while (flats) {
                const int fl = __ffsll((unsigned long long)flats) - 1;
                flats &= flats - 1ull;
                const bool mine = nflat % ntw == tw;
                nflat++;
                if (!mine) continue;
                const uint32_t fD = (uint32_t)__builtin_amdgcn_readlane((int)D, fl), fb = (uint32_t)__builtin_amdgcn_readlane((int)base, fl);
                for (uint32_t code = lane; code < (1u << fD); code += 64u) {  // follow the code's bits (LSB first) down the implicit tree
                    uint32_t cur = j0 + (uint32_t)fl, dd = d;
                    for (uint32_t l = 0; l < fD; l++) {
                        const uint32_t child = 2u * cur + ((code >> l) & 1u);
                        dd++;
                        cur = child - ((l + 1u < fD) ? P.L[dd] : 0u);
                    }
                    P.c2s[(fb + code) & 255u] = P.sorted[P.first[dd] + cur];
                }
            }
        }
    }
}

// Everything the walk needs to know about an emitting node, packed by all threads once pass 1 and the tables are done:
//   bits  0-19  bit offset of the node's run in the body     20-23  flat depth D (0: a bitmap node)
//   bits 24-31  flat root: first entry of its table in c2s[];  bitmap node: bit 24 / 25 = child 0 / 1 is a leaf
//   bits 32-47  rank of the run's first bit (mod 2^16)
//   bits 48-55 / 56-63  child 0 / 1: its symbol (leaf) or its index among the internal nodes
template <typename PL>
__device__ __forceinline__ void pdir_records(PL& P, uint32_t tid, uint32_t nthreads, uint32_t maxlen) {
    const uint32_t nint = P.ib[maxlen];  // (no internal node at the deepest level)
    for (uint32_t ii = tid; ii < nint; ii += nthreads) {
        uint32_t d = 0;
        while (d + 1u < maxlen && ii >= P.ib[d + 1]) d++;
        const uint32_t j = ii - P.ib[d], nf = P.runoff[ii];
        if (nf & 0x80000000u) continue;  // covered by a flat ancestor: never visited
        const uint32_t D = (nf >> 24) & 15u;
        uint32_t lo = (8u * (nf & 0xFFFFFFu)) | (D << 20), hi = P.rank0[ii];
        if (D) {
            lo |= ((uint32_t)P.c2sb[ii] & 255u) << 24;
        } else {
            const uint32_t Ld1 = P.L[d + 1], f1 = P.first[d + 1], ib1 = P.ib[d + 1];
#pragma unroll
            for (uint32_t bit = 0; bit < 2u; bit++) {
                const uint32_t ci = 2u * j + bit;
                uint32_t child;
                if (ci < Ld1) {
                    child = P.sorted[f1 + ci];
                    lo |= 1u << (24u + bit);
                } else {
                    child = ib1 + ci - Ld1;
                }
                hi |= (child & 255u) << (16u + 8u * bit);
            }
        }
        P.nrec[ii] = ((uint64_t)hi << 32) | lo;
    }
}

// Decodes one section payload[0 .. psize) -> out[0 .. n) (out: 4-byte aligned, n + 3 bytes writable). Called by ALL threads
// of the workgroup with the same arguments; returns the same value in all of them: 0 or a zxc error.
template <int THREADS, int ITERS>
__device__ __forceinline__ int pdir_decode(const uint8_t* __restrict__ payload_, uint32_t psize, uint32_t n, uint8_t* __restrict__ out_,
                                           PdirLds<THREADS, ITERS>& P) {
    typedef PdirLds<THREADS, ITERS> PL;
    // (arguments of an out-of-line function count as divergent: make them scalar again, so that every branch around a barrier
    // is a scalar branch)
    const uint8_t* __restrict__ payload = uni_ptr(payload_);
    uint8_t* __restrict__ out = uni_ptr(out_);
    psize = uni(psize);
    n = uni(n);
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    const uint32_t wave = uni(tid >> 6);
    if (psize < 128u || n == 0u) return E_CORRUPT;
    const uint8_t* body = payload + 128;
    const uint32_t bsize = psize - 128u, nw = (bsize + 7u) >> 3;
    if (nw + 1u > PL::kWords || n > PDIR_N_MAX) return ZXC_DEV_E_INTERNAL;  // (the launch pass sends such sections to the one-wave decoder)
    const uint32_t nit = (nw + 1u + PL::kStagers - 1u) / PL::kStagers;  // words 0 .. nw: the last one is the zero guard
    uint32_t excl[ITERS];
    // ---- 1. tree (wave 0) | body -> LDS + popcounts (waves 1..)
    if (wave == 0u) {
        PivTree T;
        const int rc = piv_tree(payload, P, lane, T);
        if (lane == 0) {
            P.rc_tree = rc;
            P.maxlen = T.maxlen;
            P.single = T.degenerate ? (T.ok1 ? 1u : 2u) : 0u;
        }
    } else {
        const uint32_t st = tid - 64u;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            excl[it] = 0;
            if ((uint32_t)it < nit) {
                const uint32_t i = (uint32_t)it * PL::kStagers + st;
                uint64_t w = 0;
                if (8u * i + 8u <= bsize) w = g_ld64(body + 8u * i);
                else if (8u * i < bsize)
                    for (uint32_t k = 0; 8u * i + k < bsize; k++) w |= (uint64_t)ld8(body + 8u * i + k) << (8u * k);
                P.W[i] = w;
                const uint32_t pc = (uint32_t)__popcll(w);
                const uint32_t incl = wave_scan_add(pc);
                excl[it] = incl - pc;
                if (lane == 63) P.wsum[(uint32_t)it * PL::kSlices + (wave - 1u)] = incl;
            }
        }
    }
    __syncthreads();
    if (wave == 1u) {  // exclusive prefix over the (round, wave) slices, in word order
        uint32_t carry = 0;
        for (uint32_t c0 = 0; c0 < nit * PL::kSlices; c0 += 64u) {
            const uint32_t idx = c0 + (uint32_t)lane;
            const uint32_t v = idx < nit * PL::kSlices ? P.wsum[idx] : 0u;
            const uint32_t incl = wave_scan_add(v);
            if (idx < nit * PL::kSlices) P.wsum[idx] = carry + incl - v;
            carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    __syncthreads();
    if (wave != 0u) {
        const uint32_t st = tid - 64u;
#pragma unroll
        for (int it = 0; it < ITERS; it++)
            if ((uint32_t)it < nit) P.cum[(uint32_t)it * PL::kStagers + st] = (uint16_t)(excl[it] + P.wsum[(uint32_t)it * PL::kSlices + (wave - 1u)]);
    }
    __syncthreads();
    int rc = (int)uni((uint32_t)P.rc_tree);
    const uint32_t maxlen = uni(P.maxlen), single = uni(P.single);
    // ---- 2. run offsets, child counts (wave 0) | flat tables (waves 1..)
    if (rc == 0) {
        if (wave == 0u) {
            int r1 = 0;
            if (single) {  // one symbol of code length 1: the root's run is n zero bits
                const uint32_t nb = (n + 7u) >> 3;
                if (single == 2u || nb > bsize || pdir_rank(P, n) != 0u) r1 = E_CORRUPT;
            } else {
                r1 = pdir_pass1(P, lane, n, bsize, maxlen);
            }
            if (lane == 0) P.rc_pass1 = r1;
        } else if (!single) {
            pdir_tables(P, lane, maxlen, wave - 1u, PL::kSlices);
        }
        __syncthreads();
        rc = (int)uni((uint32_t)P.rc_pass1);
    }
    if (rc == 0 && !single) {
        pdir_records(P, tid, (uint32_t)THREADS, maxlen);
        __syncthreads();
    }
    // ---- 3. the walk
    if (rc == 0) {
        if (single) {
            const uint32_t v = 0x01010101u * (uint32_t)P.sorted[0];
            for (uint32_t k0 = 4u * tid; k0 < n; k0 += 4u * (uint32_t)THREADS) g_st32(out + k0, v);  // (up to 3 bytes past n: the caller's slack)
        } else {
            // 4 x THREADS walkers, four per lane. A walker that arrives at a symbol takes its next position at once, so no lane
            // idles while the deepest symbol of a batch finishes (a batch of four positions per lane in lock step ran as many
            // steps as the deepest emitting node for every symbol: ~3 x what the symbols need). The step is written without
            // control flow in front of its stores, so that the four walkers of a lane interleave their chains of dependent LDS
            // reads (node record -> body dwords + directory -> next node); an idle walker keeps re-reading the root. A walker
            // packs four symbols into a dword before it stores.
            // Positions are dealt out INTERLEAVED (round 4): walker w = u * THREADS + tid takes the output dwords w, w + NW,
            // w + 2 NW, ... (NW = 4 * THREADS walkers), so the 64 lanes of a store instruction write 64 neighbouring dwords
            // (a few 64-byte sectors while the lanes drift apart by a dword round or two) instead of 64 sectors `per` bytes
            // apart — round 3: 190 M write requests and 2 x write amplification per level-7 launch — and neighbouring lanes
            // read neighbouring bits of every node's run (fewer LDS bank conflicts).
            const uint32_t* W32 = (const uint32_t*)P.W;
            constexpr uint32_t kStride = 16u * (uint32_t)THREADS;  // bytes between a walker's consecutive dwords
            uint32_t pos[4], idx[4], ii[4], acc[4];
            uint32_t act = 0;  // bit u: walker u has positions left
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t first = 4u * ((uint32_t)u * (uint32_t)THREADS + tid);
                const bool in = first < n;
                act |= in ? 1u << u : 0u;
                pos[u] = in ? first : 0u;
                idx[u] = pos[u];
                ii[u] = 0;
                acc[u] = 0;
            }
            while (__ballot(act != 0u)) {
                // (three rounds of LDS reads, each issued for all four walkers before any is used)
                uint64_t rec[4];
                uint32_t pp[4], wa[4], wb[4], cm[4], fsym[4], child[4], nidx[4];
                bool flat[4], done[4];
#pragma unroll
                for (int u = 0; u < 4; u++) rec[u] = P.nrec[ii[u]];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t lo = (uint32_t)rec[u];
                    const uint32_t D = (lo >> 20) & 15u;
                    flat[u] = D != 0u;
                    pp[u] = (lo & 0xFFFFFu) + __umul24(idx[u], flat[u] ? D : 1u);  // (idx < 2^16, D < 16: a 24-bit multiply)
                    const uint32_t q = pp[u] >> 5, qa = flat[u] ? q : q & ~1u;  // a bitmap node reads its aligned 64-bit word, a flat root the two dwords around its code
                    wa[u] = W32[qa];
                    wb[u] = W32[qa + 1u];
                    cm[u] = P.cum[pp[u] >> 6];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t lo = (uint32_t)rec[u], hi = (uint32_t)(rec[u] >> 32);
                    const uint32_t D = (lo >> 20) & 15u;
                    // bitmap node: bit p of the body picks the child, the ones / zeros in front of it inside the run the index there
                    const uint32_t sh5 = pp[u] & 31u;
                    const bool upper = (pp[u] & 32u) != 0u;
                    const uint32_t t = upper ? wb[u] : wa[u];
                    const uint32_t below = (uint32_t)__popc(t & ((1u << sh5) - 1u)) + (upper ? (uint32_t)__popc(wa[u]) : 0u);
                    const uint32_t bit = (t >> sh5) & 1u;
                    const uint32_t ones = (cm[u] + below - (hi & 0xFFFFu)) & 0xFFFFu;
                    child[u] = bit ? hi >> 24 : (hi >> 16) & 255u;
                    nidx[u] = bit ? ones : idx[u] - ones;
                    const bool leaf = ((lo >> (24u + bit)) & 1u) != 0u;
                    done[u] = flat[u] || leaf;
                    // flat root: the D-bit code at bit p names the leaf
                    const uint32_t code = __builtin_amdgcn_alignbit(wb[u], wa[u], sh5) & ((1u << D) - 1u);
                    fsym[u] = P.c2s[flat[u] ? ((lo >> 24) + code) & 255u : 0u];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool on = (act >> u) & 1u, fin = on && done[u];
                    const uint32_t sv = flat[u] ? fsym[u] : child[u];
                    const uint32_t a1 = acc[u] | (sv << (8u * (pos[u] & 3u)));
                    const bool full = (pos[u] & 3u) == 3u;
                    const uint32_t npos = pos[u] + (full ? kStride - 3u : 1u);  // next byte of my dword, or my next dword
                    const bool last = npos >= n;
                    if (fin && (full || last)) g_st32(out + (pos[u] & ~3u), a1);  // (the last dword may reach 3 bytes past n: slack)
                    acc[u] = fin ? (full ? 0u : a1) : acc[u];
                    pos[u] = fin ? npos : pos[u];
                    ii[u] = fin ? 0u : (on ? child[u] : ii[u]);
                    idx[u] = fin ? (last ? 0u : npos) : (on ? nidx[u] : idx[u]);
                    act = (fin && last) ? act & ~(1u << u) : act;
                }
            }
        }
    }
    __syncthreads();  // the next section reuses the tables
    return rc;
}

// The sections on one size class's work list: `hdr` = {entries, next to hand out}, `secs` = the records written by
// zxc_order_scatter_kernel, which has checked every header field behind them (classify_block): the only errors left are the
// sections' own. A fixed grid of workgroups pulls records; the verdict goes to the block's pre[] record (rc_lit / rc_tok).
template <int THREADS, int ITERS>
__device__ __forceinline__ void pdir_sections(const uint8_t* __restrict__ comp, const zxc_dev_sec_t* __restrict__ secs,
                                              uint32_t* __restrict__ hdr, zxc_dev_pre_t* __restrict__ pre, uint8_t* __restrict__ pscratch) {
    __shared__ PdirLds<THREADS, ITERS> P;
    const uint32_t n_items = uni(__hip_atomic_load(hdr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // (every round ENDS with a barrier: with the one-thread store of the verdict as the loop's last statement and the
    // one-thread fetch as its first, the compiler fused the two into one divergent region across the back edge and thread 0
    // met the barriers apart from its wave: a hang on the device)
    for (;;) {
        if (threadIdx.x == 0) P.item = atomicAdd(hdr + 1, 1u);
        __syncthreads();
        const uint32_t item = uni(P.item);
        if (item >= n_items) break;
        const zxc_dev_sec_t* s = secs + item;
        const uint64_t src_off = ((uint64_t)uni((uint32_t)(s->src_off >> 32)) << 32) | uni((uint32_t)s->src_off);
        const uint32_t psize = uni(s->psize), n = uni(s->n), out_off4 = uni(s->out_off4), rc_slot = uni(s->rc_slot);
        const int rc = pdir_decode<THREADS, ITERS>(comp + src_off, psize, n, pscratch + 4ull * out_off4, P);
        if (threadIdx.x == 0) ((int16_t*)pre)[rc_slot] = (int16_t)rc;
        __syncthreads();  // (P.item is rewritten at the top of the next round)
    }
}
extern "C" __global__ void __launch_bounds__(PDIR_SMALL_THREADS, 5)   // (second number: waves per SIMD the register budget must allow)
zxc_pivco_sections_small_kernel(const uint8_t* __restrict__ comp, const zxc_dev_sec_t* __restrict__ secs, uint32_t* __restrict__ hdr,
                                zxc_dev_pre_t* __restrict__ pre, uint8_t* __restrict__ pscratch) {
    pdir_sections<PDIR_SMALL_THREADS, PDIR_SMALL_ITERS>(comp, secs, hdr, pre, pscratch);
}
extern "C" __global__ void __launch_bounds__(PDIR_MEDIUM_THREADS, 3)
zxc_pivco_sections_medium_kernel(const uint8_t* __restrict__ comp, const zxc_dev_sec_t* __restrict__ secs, uint32_t* __restrict__ hdr,
                                 zxc_dev_pre_t* __restrict__ pre, uint8_t* __restrict__ pscratch) {
    pdir_sections<PDIR_MEDIUM_THREADS, PDIR_MEDIUM_ITERS>(comp, secs, hdr, pre, pscratch);
}
extern "C" __global__ void __launch_bounds__(PDIR_LARGE_THREADS, 4)
zxc_pivco_sections_large_kernel(const uint8_t* __restrict__ comp, const zxc_dev_sec_t* __restrict__ secs, uint32_t* __restrict__ hdr,
                                zxc_dev_pre_t* __restrict__ pre, uint8_t* __restrict__ pscratch) {
    pdir_sections<PDIR_LARGE_THREADS, PDIR_LARGE_ITERS>(comp, secs, hdr, pre, pscratch);
}
