// zxc_pivco.inc — PivCo (level-ordered Huffman) section decode for one wavefront.
// Included by zxc_decode_kernel.hip. Reference behaviour: zxc_huf_decode_section
// (src/lib/zxc_huffman.c:2447-2457) = unpack lengths (:960-977) + canonical tree and flat
// roots (:1042-1170) + decode core (:2271-2430); format: docs/FORMAT.md §5.2.1.
//
// Nothing of the CPU structure survives here. With canonical codes the tree is implicit:
// at depth d the N_d nodes in BFS (= wire) order are the L_d leaves (symbols of length d, in
// symbol order) followed by the I_d internal nodes, and internal node j has children 2j, 2j+1
// of depth d+1. So there is no trie to build: per-depth counts give every node id, parent
// and children by arithmetic. The wave then
//   pass 1 (top-down, one depth at a time): run sizes -> prefix sum -> run pointers ->
//          popcount of every bitmap run = its right child's symbol count;
//   pass 2 (bottom-up): every emitting node rebuilds its symbol sequence, 64 symbols per
//          step: a merge is out[k] = bit_k ? R[rank1(k)] : L[rank0(k)] with
//          rank = running base + popcount(bits below my lane) (ballot-style prefix popcount);
//          flat roots unpack D-bit codes through a small LDS table; leaf children are
//          constants and are never materialised.
// Level buffers ping-pong between `out` (even depths; depth 0 = result) and `tmp` (odd).
// Per-node state exists for INTERNAL nodes only (<= 255 of a 256-symbol code), which makes room in LDS for the
// slot -> node map of the small-node path.

#define PIV_MAXLEN 11
#define PIV_INT 256      // internal nodes of a 256-symbol code: <= 255
#define PIV_SMAP 3584u   // slots of the slot -> node map of one group of 64 small nodes (above it: binary search)
#define PIV_INFLIGHT 8   // 64-symbol words of a merge whose child runs are requested together (A/B: 12 and 16 are slower: fewer whole rounds)
#define PIV_FLAT_INFLIGHT 8  // 64-symbol steps of a flat node's code run requested together

#ifdef EXP_PIV_PROF  // experiment only: shader-clock split of the section decoder, per block (tools/abbench.py AB_PIVPROF=1)
__shared__ uint32_t g_piv_prof[16];
#define PIVP(i) do { const uint32_t t_ = (uint32_t)__builtin_readcyclecounter(); if (lane == 0) { g_piv_prof[i] += t_ - g_piv_prof[15]; g_piv_prof[15] = t_; } } while (0)
#define PIVC(i, n) do { if (lane == 0) g_piv_prof[i] += (n); } while (0)
#else
#define PIVP(i) do { } while (0)
#define PIVC(i, n) do { } while (0)
#endif

struct PivLds {  // overlays WaveLds (the ring is idle while a section is being decoded)
    uint32_t cnt[PIV_INT];     // symbols routed through the internal node
    uint32_t runoff[PIV_INT];  // bits 0-23: byte offset of the node's run in the section body; 24-27: flat depth D (complete
                               // subtree rooted here) or 0; bit 31: covered by a flat ancestor (emits nothing)
    uint32_t seqoff[PIV_INT];  // offset of its rebuilt sequence in its depth's buffer
    uint8_t smap[PIV_SMAP];    // pass 2, small nodes: lane of the node that owns output slot s of the current group of 64 nodes
    uint8_t len[256];
    uint8_t sorted[256];       // symbols ordered by (length, symbol)
    uint8_t c2s[256];          // code -> symbol table of the flat root being unpacked
    uint32_t first[PIV_MAXLEN + 2];  // first[l]: index in sorted[] of the first symbol of length l
    uint32_t L[PIV_MAXLEN + 2];      // leaves per depth
    uint32_t N[PIV_MAXLEN + 2];      // nodes per depth
    uint32_t ib[PIV_MAXLEN + 2];     // index of the first internal node of a depth
};

__device__ __forceinline__ uint32_t nt_ld8(const uint8_t* p) { return __builtin_nontemporal_load(p); }
// The same through a pointer the compiler knows to be global memory: inside this out-of-line function the
// buffers are generic pointers, i.e. FLAT accesses, which count against both vmcnt and lgkmcnt and make every
// dependent store wait for all of them (vmcnt(0)); global_load / global_store get exact partial waits.
typedef const uint8_t __attribute__((address_space(1))) * gcptr_t;
typedef uint8_t __attribute__((address_space(1))) * gptr_t;
__device__ __forceinline__ uint32_t g_nt_ld8(const uint8_t* p) { return __builtin_nontemporal_load((gcptr_t)(uintptr_t)p); }
__device__ __forceinline__ void g_st8(uint8_t* p, uint32_t v) { *(gptr_t)(uintptr_t)p = (uint8_t)v; }
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
typedef const u32_unaligned __attribute__((address_space(1))) * gcptr32_t;
typedef u32_unaligned __attribute__((address_space(1))) * gptr32_t;
typedef uint64_t __attribute__((aligned(1))) u64_una;
__device__ __forceinline__ v4u g_ld128(const uint8_t* p) { return *(const v4u_unaligned __attribute__((address_space(1)))*)(uintptr_t)p; }
__device__ __forceinline__ uint64_t g_ld64(const uint8_t* p) { return *(const u64_una __attribute__((address_space(1)))*)(uintptr_t)p; }
__device__ __forceinline__ uint32_t g_nt_ld32(const uint8_t* p) { return __builtin_nontemporal_load((gcptr32_t)(uintptr_t)p); }
__device__ __forceinline__ void g_st32(uint8_t* p, uint32_t v) { *(gptr32_t)(uintptr_t)p = v; }

// One depth of pass 2.
__device__ __forceinline__ void piv_level(PivLds& P, int d, const uint8_t* __restrict__ body, uint32_t bsize,
                                          uint8_t* __restrict__ buf_d, const uint8_t* __restrict__ buf_c, int lane) {
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    auto rd_child = [&](uint32_t idx) -> uint32_t { return g_nt_ld8(buf_c + idx); };
    auto wr = [&](uint32_t idx, uint32_t v) { g_st8(buf_d + idx, v); };
    // One 64-symbol word of a merge takes the next z symbols of the left child and the next o of the right one (z + o =
    // symbols in the word): two CONTIGUOUS byte runs. They are fetched as dwords (lanes 0-15 the left run, lanes 32-47
    // the right one: one request of two cache lines instead of a 64-lane byte gather) and every lane picks its byte
    // across lanes (ds_bpermute).
    // word_request: idx_l / idx_r = buffer indices of the runs' first symbols; leaf children are constants (no load).
    auto word_request = [&](uint64_t mask, uint32_t left, uint32_t idx_l, uint32_t idx_r, bool leaf0, bool leaf1) -> uint32_t {
        const uint32_t o = __popcll(mask), z = (left < 64u ? left : 64u) - o;
        const bool right = lane >= 32;
        const uint32_t nd = ((right ? o : z) + 3u) >> 2;                  // dwords of my half's run
        const uint32_t li = (uint32_t)lane & 31u;
        const uint32_t di = nd == 0u ? 0u : (li < nd ? li : nd - 1u);      // (idle lanes re-read the run's last dword; it may reach 3 bytes past the run: slack)
        const bool skip = right ? leaf1 : leaf0;
        return g_nt_ld32(buf_c + (skip ? 0u : (right ? idx_r : idx_l) + 4u * di));
    };
    auto word_value = [&](uint32_t loaded, uint64_t mask, bool leaf0, bool leaf1, uint32_t sym0, uint32_t sym1) -> uint32_t {
        const uint32_t below = __popcll(mask & lt_mask);
        const bool bit = (mask >> lane) & 1ull;
        const uint32_t rank = bit ? below : (uint32_t)lane - below;
        const uint32_t dw = __shfl(loaded, (int)((bit ? 32u : 0u) + ((rank >> 2) & 15u)));
        const uint32_t by = (dw >> (8u * (rank & 3u))) & 255u;
        return (bit ? leaf1 : leaf0) ? (bit ? sym1 : sym0) : by;
    };
    auto word_store = [&](uint32_t idx, uint32_t v, uint32_t left) {  // symbols of lanes 0..left-1 -> buf_d[idx ..]: dwords + a byte tail
        const uint32_t x1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x55, 0xf, 0xf, false);  // quad_perm: lane 1 of my quad
        const uint32_t x2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xAA, 0xf, 0xf, false);
        const uint32_t x3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xFF, 0xf, 0xf, false);
        const uint32_t packed = v | (x1 << 8) | (x2 << 16) | (x3 << 24);
        if (((uint32_t)lane & 3u) == 0u && (uint32_t)lane + 4u <= left) g_st32(buf_d + idx + lane, packed);
        else if ((uint32_t)lane >= (left & ~3u) && (uint32_t)lane < left) g_st8(buf_d + idx + lane, v);
    };
    const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d], Bc = P.ib[d + 1];
    const uint32_t Lc = P.L[d + 1];
    // Most internal nodes are deep and carry a handful of symbols; walking them one by one costs a
    // memory round trip per node. So per 64 nodes: the few big ones (> 64 symbols) are rebuilt by the
    // whole wave one at a time, all the small ones together, 64 output symbols per step whatever
    // node they belong to (slot -> node by binary search over the prefix sum of the counts).
    uint32_t Lr[PIV_MAXLEN + 1];  // leaves per depth below d (wave-uniform)
#pragma unroll
    for (int l = 0; l <= PIV_MAXLEN; l++) Lr[l] = ((uint32_t)d + 1u + (uint32_t)l <= PIV_MAXLEN + 1u) ? uni(P.L[d + 1 + l]) : 0u;
    for (uint32_t j0 = 0; j0 < Id; j0 += 64u) {
        const uint32_t jn = j0 + (uint32_t)lane;
        const bool nhave = jn < Id;
        const uint32_t nii = Bi + (nhave ? jn : 0u);
        const uint32_t nnf = P.runoff[nii];
        const bool nemit = nhave && !(nnf & 0x80000000u);
        const uint32_t nc = nemit ? P.cnt[nii] : 0u;
        const uint32_t nD = nemit ? ((nnf >> 24) & 15u) : 0u;
        const uint32_t nro = nnf & 0xFFFFFFu;
        const uint32_t nso = nemit ? P.seqoff[nii] : 0u;
        const uint32_t ncs = nc <= 64u ? nc : 0u;
        const uint32_t nincl = wave_scan_add(ncs);
        const uint32_t ntotal = (uint32_t)__builtin_amdgcn_readlane((int)nincl, 63);
        // every small bitmap node's whole run (<= 64 bits) is fetched once by the node's lane: the steps below take it
        // from that lane's registers (two cross-lane reads) instead of a memory round trip per step
        uint64_t nmask = 0;
        if (ncs != 0u && nD == 0u) {
            const uint8_t* nrun = body + nro;
            if (nro + 8u <= bsize) nmask = ld64(nrun);
            else for (uint32_t q = 0; q < ((ncs + 7u) >> 3); q++) nmask |= (uint64_t)ld8(nrun + q) << (8u * q);
            if (ncs < 64u) nmask &= (1ull << ncs) - 1ull;
        }
        const uint32_t nmlo = (uint32_t)nmask, nmhi = (uint32_t)(nmask >> 32);
        // where the node's children keep their sequences (leaf children: unused)
        const uint32_t nc0 = 2u * jn, nc1 = nc0 + 1u;
        const uint32_t nq0 = (ncs != 0u && nD == 0u && nc0 >= Lc) ? P.seqoff[Bc + nc0 - Lc] : 0u;
        const uint32_t nq1 = (ncs != 0u && nD == 0u && nc1 >= Lc) ? P.seqoff[Bc + nc1 - Lc] : 0u;
        // slot -> node: every node lane writes its lane number over its slots (no waits: plain LDS stores), a step then
        // finds its node with ONE LDS read instead of a six-deep binary search across lanes
        const bool mapped = ntotal <= PIV_SMAP;
        if (mapped) {
            for (uint32_t q = 0; q < ncs; q++) P.smap[nincl - ncs + q] = (uint8_t)lane;
            wave_lds_fence();
        }
        for (uint32_t s0 = 0; s0 < ntotal; s0 += 64u) {
            const uint32_t sidx = s0 + (uint32_t)lane;
            const bool valid = sidx < ntotal;
            uint32_t t = 0;  // the node's lane = number of lanes whose inclusive sum is <= sidx
            if (mapped) t = valid ? (uint32_t)P.smap[sidx] : 0u;
            else {
#pragma unroll
                for (int st = 32; st >= 1; st >>= 1) {
                    const uint32_t pv = __shfl(nincl, (int)(t + st - 1u));
                    if (pv <= sidx) t += st;
                }
                t = t > 63u ? 63u : t;
            }
            const uint32_t tc = __shfl(ncs, (int)t), tincl = __shfl(nincl, (int)t), tD = __shfl(nD, (int)t),
                           tro = __shfl(nro, (int)t), tso = __shfl(nso, (int)t), tq0 = __shfl(nq0, (int)t), tq1 = __shfl(nq1, (int)t);
            const uint64_t mask = (uint64_t)__shfl(nmlo, (int)t) | ((uint64_t)__shfl(nmhi, (int)t) << 32);
            const uint32_t k = sidx - (tincl - tc);
            const uint32_t tj = j0 + t;
            const uint8_t* trun = body + tro;
            uint32_t sym = 0;
            if (valid && tD == 0u) {  // merge: bit k of the node's bitmap picks the child, its rank the element
                const bool bit = (mask >> k) & 1ull;
                const uint32_t below = __popcll(mask & ((1ull << k) - 1ull));
                const uint32_t ci = 2u * tj + (bit ? 1u : 0u);
                const uint32_t rank = bit ? below : k - below;
                if (ci < Lc) sym = P.sorted[P.first[d + 1] + ci];
                else sym = rd_child((bit ? tq1 : tq0) + rank);
            } else if (valid) {  // flat root: a tD-bit code, walked down the implicit tree
                const uint32_t fbytes = (uint32_t)(((uint64_t)tc * tD + 7u) >> 3);
                const uint32_t bp = k * tD, byte = bp >> 3;
                uint32_t w = ld8(trun + byte);
                if (byte + 1u < fbytes) w |= ld8(trun + byte + 1u) << 8;
                if (byte + 2u < fbytes) w |= ld8(trun + byte + 2u) << 16;
                const uint32_t code = (w >> (bp & 7u)) & ((1u << tD) - 1u);
                uint32_t cur = tj;
#pragma unroll
                for (int l = 0; l < PIV_MAXLEN; l++) {
                    if ((uint32_t)l < tD) {
                        cur = 2u * cur + ((code >> l) & 1u);
                        if ((uint32_t)l + 1u < tD) cur -= Lr[l];
                    }
                }
                sym = P.sorted[P.first[(uint32_t)d + tD] + cur];
            }
            if (valid) wr(tso + k, sym);
        }
        PIVP(0);
        uint64_t bigm = __ballot(nc > 64u);
        // up to 4096 bits of a big node's run, one 64-bit word per lane, requested by EVERY lane (lanes beyond the run
        // re-read its last word and drop it): an unconditional load can stay in flight across the work on another node
        auto run_words = [&](const uint8_t* runp, uint32_t bits) -> uint64_t {
            const uint32_t nwp = bits >= 4096u ? 64u : (bits + 63u) >> 6;
            const uint32_t wl = (uint32_t)lane < nwp ? (uint32_t)lane : nwp - 1u;
            uint64_t wv = ld64(runp + 8u * wl);  // (the last word may reach up to 7 bytes past the run: inside the block or its slack)
            const uint32_t left = bits - 64u * wl;
            if (left < 64u) wv &= (1ull << left) - 1ull;
            return (uint32_t)lane < nwp ? wv : 0ull;
        };
        uint64_t mw_next = 0;
        if (bigm) {
            const int b0l = __ffsll((unsigned long long)bigm) - 1;
            mw_next = run_words(body + (uint32_t)__builtin_amdgcn_readlane((int)nro, b0l), (uint32_t)__builtin_amdgcn_readlane((int)nc, b0l));
        }
        while (bigm) {
            const int bl = __ffsll((unsigned long long)bigm) - 1;
            bigm &= bigm - 1ull;
            const uint64_t mw_first = mw_next;
            {   // the next big node's words are requested now and arrive while this node is rebuilt
                const int bn = bigm ? __ffsll((unsigned long long)bigm) - 1 : bl;
                mw_next = run_words(body + (uint32_t)__builtin_amdgcn_readlane((int)nro, bn), (uint32_t)__builtin_amdgcn_readlane((int)nc, bn));
            }
            const uint32_t j = j0 + (uint32_t)bl;
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)nc, bl);
            const uint32_t D = (uint32_t)__builtin_amdgcn_readlane((int)nD, bl);
            const uint32_t so = (uint32_t)__builtin_amdgcn_readlane((int)nso, bl);
            const uint8_t* run = body + (uint32_t)__builtin_amdgcn_readlane((int)nro, bl);
            if (D) {
                // code -> symbol: follow the code's bits (LSB first) down the implicit tree
                const uint32_t ncode = 1u << D;
                for (uint32_t code = lane; code < ncode; code += 64u) {
                    uint32_t cur = j, dd = (uint32_t)d;
                    for (uint32_t l = 0; l < D; l++) {
                        const uint32_t child = 2u * cur + ((code >> l) & 1u);
                        dd++;
                        cur = child - ((l + 1u < D) ? P.L[dd] : 0u);
                    }
                    P.c2s[code & 255u] = P.sorted[P.first[dd] + cur];
                }
                wave_lds_fence();
                PIVP(2);
                PIVC(8, 1u);
                PIVC(9, (c + 63u) >> 6);
                const uint32_t m = ncode - 1u;
                // 64 symbols = 64 D bits = 8 D whole bytes of the run: 2 D dwords, fetched by lanes 0 .. 2D-1 as ONE request;
                // each lane then takes its code from two neighbouring dwords across lanes.
                const uint32_t nsteps = (c + 63u) >> 6;
                auto flat_sym = [&](uint32_t ld) -> uint32_t {
                    const uint32_t bp = (uint32_t)lane * D, di = bp >> 5;
                    const uint32_t lo = __shfl(ld, (int)di), hi = __shfl(ld, (int)(di + 1u < 2u * D ? di + 1u : di));
                    return (uint32_t)P.c2s[(uint32_t)((((uint64_t)hi << 32) | lo) >> (bp & 31u)) & m];
                };
                // Whole rounds are software-pipelined: the loads of round r+1 are issued BEFORE the stores of round r, and every
                // load and store of the loop is unconditional (whole steps only, a byte per lane). Vector-memory operations
                // complete in issue order and stores share the loads' counter, so a wait for a load also waits for every
                // older store: with "8 loads, then 8 conditional stores" per iteration each round paid the stores'
                // acknowledgement AND the loads' round trip in series (~8 K clocks per round, measured: this loop and the
                // merge loop below were all of pass 2). With fixed counts the compiler waits exactly (younger loads and
                // stores stay in flight).
                uint32_t sdone = 0;
                {
                    const uint32_t nrounds = (c >> 6) / PIV_FLAT_INFLIGHT;
                    const uint32_t dl = (uint32_t)lane < 2u * D ? (uint32_t)lane : 2u * D - 1u;
                    const uint8_t* runl = run + 4u * dl;
                    if (nrounds) {
                        uint32_t ldA[PIV_FLAT_INFLIGHT], ldB[PIV_FLAT_INFLIGHT];
#pragma unroll
                        for (int u = 0; u < PIV_FLAT_INFLIGHT; u++) ldA[u] = g_nt_ld32(runl + 8u * D * (uint32_t)u);
                        // (two rounds per iteration, the register sets swapped: a copy would have to wait for the loads)
                        auto flat_round = [&](uint32_t (&cur)[PIV_FLAT_INFLIGHT], uint32_t (&nxt)[PIV_FLAT_INFLIGHT], uint32_t r) {
                            const uint32_t nb = (r + 1u < nrounds ? r + 1u : r) * PIV_FLAT_INFLIGHT;  // (after the last round: a harmless re-request)
#pragma unroll
                            for (int u = 0; u < PIV_FLAT_INFLIGHT; u++) nxt[u] = g_nt_ld32(runl + 8u * D * (nb + (uint32_t)u));
#pragma unroll
                            for (int u = 0; u < PIV_FLAT_INFLIGHT; u++)
                                g_st8(buf_d + so + 64u * (r * PIV_FLAT_INFLIGHT + (uint32_t)u) + lane, flat_sym(cur[u]));
                        };
                        uint32_t r = 0;
                        for (; r + 1u < nrounds; r += 2u) {
                            flat_round(ldA, ldB, r);
                            flat_round(ldB, ldA, r + 1u);
                        }
                        if (r < nrounds) flat_round(ldA, ldB, r);
                        sdone = nrounds * PIV_FLAT_INFLIGHT;
                    }
                }
                for (uint32_t s0 = sdone; s0 < nsteps; s0 += PIV_FLAT_INFLIGHT) {  // the remaining (< PIV_FLAT_INFLIGHT whole + one partial) steps
                    uint32_t ldw[PIV_FLAT_INFLIGHT];
#pragma unroll
                    for (int u = 0; u < PIV_FLAT_INFLIGHT; u++) {
                        const uint32_t st = s0 + (uint32_t)u < nsteps ? s0 + (uint32_t)u : nsteps - 1u;
                        const uint32_t left = c - 64u * st < 64u ? c - 64u * st : 64u;
                        const uint32_t nd = (((left * D + 7u) >> 3) + 3u) >> 2;  // dwords holding the step's codes (the last may reach 3 bytes past the run: slack)
                        const uint32_t di = (uint32_t)lane < nd ? (uint32_t)lane : nd - 1u;
                        ldw[u] = g_nt_ld32(run + 8u * D * st + 4u * di);  // (every lane, live step or not: a fixed number of loads in flight)
                    }
#pragma unroll
                    for (int u = 0; u < PIV_FLAT_INFLIGHT; u++) {
                        const uint32_t st = s0 + (uint32_t)u;
                        if (st < nsteps) word_store(so + 64u * st, flat_sym(ldw[u]), c - 64u * st < 64u ? c - 64u * st : 64u);
                    }
                }
                wave_lds_fence();
                PIVP(3);
            } else {
                PIVC(10, 1u);
                PIVC(11, (c + 63u) >> 6);
                const uint32_t i0 = 2u * j, i1 = 2u * j + 1u;
                const bool leaf0 = i0 < Lc, leaf1 = i1 < Lc;
                const uint32_t sym0 = leaf0 ? P.sorted[P.first[d + 1] + i0] : 0u;
                const uint32_t sym1 = leaf1 ? P.sorted[P.first[d + 1] + i1] : 0u;
                const uint32_t q0 = leaf0 ? 0u : P.seqoff[Bc + i0 - Lc];
                const uint32_t q1 = leaf1 ? 0u : P.seqoff[Bc + i1 - Lc];
                PIVP(4);
                uint32_t b0 = 0, b1 = 0;  // symbols already taken from the left / right child
                // 4096 symbols per outer step: every lane fetches one 64-bit word of the node's bitmap, the
                // inner loop takes the words from registers (v_readlane) PIV_INFLIGHT at a time, so the gathers
                // from the children are in flight together and the bitmap costs no round trip per word.
                for (uint32_t kb = 0; kb < c; kb += 4096u) {
                    const uint32_t rem = c - kb;
                    const uint32_t nw = rem >= 4096u ? 64u : (rem + 63u) >> 6;
                    const uint64_t mw = kb == 0u ? mw_first : run_words(run + (kb >> 3), rem);
                    const uint32_t mlo = (uint32_t)mw, mhi = (uint32_t)(mw >> 32);
                    auto maskof = [&](uint32_t w) -> uint64_t {
                        return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mlo, (int)w) |
                               ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mhi, (int)w) << 32);
                    };
                    // whole words, software-pipelined like the flat steps above (loads of round r+1 before the stores of round r,
                    // everything unconditional: a byte per lane)
                    uint32_t wdone = 0;
                    {
                        const uint32_t nrounds = (rem >= 4096u ? 64u : rem >> 6) / PIV_INFLIGHT;
                        if (nrounds) {
                            uint32_t ldA[PIV_INFLIGHT], ldB[PIV_INFLIGHT];
                            uint64_t mkA[PIV_INFLIGHT], mkB[PIV_INFLIGHT];  // (A/B: taking the masks from the lanes again instead of holding them: -8 %)
                            uint32_t rb0 = b0, rb1 = b1, nb0 = b0, nb1 = b1;  // cursors at the start / after the words of round r
#pragma unroll
                            for (int u = 0; u < PIV_INFLIGHT; u++) {
                                mkA[u] = maskof((uint32_t)u);
                                ldA[u] = word_request(mkA[u], 64u, q0 + nb0, q1 + nb1, leaf0, leaf1);
                                const uint32_t t1 = __popcll(mkA[u]);
                                nb1 += t1;
                                nb0 += 64u - t1;
                            }
                            auto word_round = [&](uint32_t (&cur)[PIV_INFLIGHT], uint64_t (&mcur)[PIV_INFLIGHT], uint32_t (&nxt)[PIV_INFLIGHT],
                                                  uint64_t (&mnxt)[PIV_INFLIGHT], uint32_t r) {
                                const bool more = r + 1u < nrounds;  // (after the last round: a harmless re-request of its own words)
                                const uint32_t wb = (more ? r + 1u : r) * PIV_INFLIGHT;
                                const uint32_t tb0 = nb0, tb1 = nb1;
                                uint32_t xb0 = more ? nb0 : rb0, xb1 = more ? nb1 : rb1;
#pragma unroll
                                for (int u = 0; u < PIV_INFLIGHT; u++) {
                                    mnxt[u] = maskof(wb + (uint32_t)u);
                                    nxt[u] = word_request(mnxt[u], 64u, q0 + xb0, q1 + xb1, leaf0, leaf1);
                                    const uint32_t t1 = __popcll(mnxt[u]);
                                    xb1 += t1;
                                    xb0 += 64u - t1;
                                }
#pragma unroll
                                for (int u = 0; u < PIV_INFLIGHT; u++) {
                                    const uint32_t v = word_value(cur[u], mcur[u], leaf0, leaf1, sym0, sym1);
                                    g_st8(buf_d + so + kb + 64u * (r * PIV_INFLIGHT + (uint32_t)u) + lane, v);
                                }
                                rb0 = tb0; rb1 = tb1;
                                nb0 = xb0; nb1 = xb1;
                            };
                            uint32_t r = 0;
                            for (; r + 1u < nrounds; r += 2u) {  // (two rounds per iteration, the register sets swapped: no copies)
                                word_round(ldA, mkA, ldB, mkB, r);
                                word_round(ldB, mkB, ldA, mkA, r + 1u);
                            }
                            if (r < nrounds) word_round(ldA, mkA, ldB, mkB, r);
                            b0 = rb0;
                            b1 = rb1;
                            wdone = nrounds * PIV_INFLIGHT;
                        }
                    }
                    for (uint32_t w0 = wdone; w0 < nw; w0 += PIV_INFLIGHT) {  // the remaining (< PIV_INFLIGHT whole + one partial) words
                        uint32_t ldw[PIV_INFLIGHT], lefts[PIV_INFLIGHT];
                        uint64_t masks[PIV_INFLIGHT];
#pragma unroll
                        for (int u = 0; u < PIV_INFLIGHT; u++) {
                            const uint32_t w = w0 + (uint32_t)u;
                            const uint32_t wi = w < nw ? w : nw - 1u;
                            masks[u] = (w < nw) ? maskof(wi) : 0ull;
                            lefts[u] = w < nw ? rem - 64u * w : 0u;
                            // (requested by every lane, live word or not: a load under a condition makes the compiler wait
                            // for it on the spot, and then only one of the PIV_INFLIGHT round trips would be in flight)
                            ldw[u] = word_request(masks[u], lefts[u], q0 + b0, q1 + b1, leaf0, leaf1);
                            const uint32_t tot1 = __popcll(masks[u]);
                            b1 += tot1;
                            b0 += (lefts[u] >= 64u ? 64u : lefts[u]) - tot1;
                        }
#pragma unroll
                        for (int u = 0; u < PIV_INFLIGHT; u++)
                            word_store(so + kb + 64u * (w0 + (uint32_t)u), word_value(ldw[u], masks[u], leaf0, leaf1, sym0, sym1), lefts[u]);
                    }
                }
                PIVP(5);
            }
        }
    }
}

// Decodes one section into out[0..n). `tmp` is n bytes of scratch. `shared_lens` != nullptr: the
// 128-byte code-length table comes from the dictionary (enc_lit = 3, zxc_huffman.c:2467-2473) and
// the payload has no inline header. Returns 0 or a zxc error.
// The code: lengths -> canonical order, per-depth node / leaf counts, flat roots. Touches P.len / sorted / first / N / L /
// ib / runoff (flags only) / cnt (zeroed). One wave. T.degenerate: a one-symbol table (T.ok1: its length is 1).
struct PivTree { uint32_t maxlen; bool degenerate, ok1; };
template <typename PL>
__device__ __forceinline__ int piv_tree(const uint8_t* __restrict__ lens128, PL& P, int lane, PivTree& T) {
    T.maxlen = 0;
    T.degenerate = false;
    T.ok1 = false;
    // ---- A. code lengths: lane owns symbols 4*lane .. 4*lane+3
    const uint32_t two = ld16(lens128 + 2 * lane);
    uint32_t myl[4] = {two & 15u, (two >> 4) & 15u, (two >> 8) & 15u, (two >> 12) & 15u};
    uint32_t mx = myl[0] > myl[1] ? myl[0] : myl[1];
    mx = mx > myl[2] ? mx : myl[2];
    mx = mx > myl[3] ? mx : myl[3];
    if (__ballot(mx > PIV_MAXLEN)) return E_CORRUPT;
#pragma unroll
    for (int k = 0; k < 4; k++) P.len[4 * lane + k] = (uint8_t)myl[k];
    uint32_t blc[PIV_MAXLEN + 1];
    uint32_t kraft = 0, present = 0, maxlen = 0, run_first = 0;
    blc[0] = 0;
#pragma unroll
    for (int l = 1; l <= PIV_MAXLEN; l++) {
        const uint32_t mine = (myl[0] == (uint32_t)l) + (myl[1] == (uint32_t)l) + (myl[2] == (uint32_t)l) + (myl[3] == (uint32_t)l);
        const uint32_t incl = wave_scan_add(mine);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        blc[l] = tot;
        if (tot) maxlen = l;
        kraft += tot << (PIV_MAXLEN - l);
        present += tot;
        // place my symbols of this length into sorted[] (symbol order within a length)
        uint32_t at = run_first + incl - mine;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (myl[k] == (uint32_t)l) P.sorted[at++] = (uint8_t)(4 * lane + k);
        if (lane == 0) P.first[l] = run_first;
        run_first += tot;
    }
    if (present == 0u) return E_CORRUPT;
    wave_lds_fence();
    T.maxlen = maxlen;
    if (present == 1u) {  // degenerate table: one symbol, code length exactly 1; the root's run is all zero bits (the caller checks)
        T.degenerate = true;
        T.ok1 = blc[1] == 1u;
        return 0;
    }
    if (kraft != (1u << PIV_MAXLEN)) return E_CORRUPT;

    PIVP(12);
    // ---- B. implicit level structure (per-depth node / leaf counts, first internal index)
    {
        uint32_t I = 1, ibase = 0;
        if (lane == 0) { P.N[0] = 1; P.L[0] = 0; P.ib[0] = 0; }
#pragma unroll
        for (int d = 1; d <= PIV_MAXLEN; d++) {
            const bool in = (uint32_t)d <= maxlen;
            const uint32_t Nd = in ? 2u * I : 0u;
            const uint32_t Ld = in ? blc[d] : 0u;
            ibase += I;
            if (lane == 0) { P.N[d] = Nd; P.L[d] = Ld; P.ib[d] = ibase; }
            I = Nd - Ld;  // Kraft equality keeps this >= 0 and ends at 0
        }
        if (lane == 0) { P.N[PIV_MAXLEN + 1] = 0; P.L[PIV_MAXLEN + 1] = 0; P.ib[PIV_MAXLEN + 1] = ibase; }
        wave_lds_fence();
        if (ibase > PIV_INT) return E_CORRUPT;  // (cannot happen with <= 256 symbols and a full code)
    }

    // flat roots: maximal complete subtrees of depth >= 2 (docs/FORMAT.md §5.2.1)
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Ld = P.L[d], Id = P.N[d] - P.L[d], Bi = P.ib[d];
        const uint32_t Bp = d ? P.ib[d - 1] : 0u;
        for (uint32_t j = lane; j < Id; j += 64u) {
            const uint32_t i = Ld + j;  // node index within its depth
            uint32_t cov = 0;
            if (d > 0u) cov = (P.runoff[Bp + (i >> 1)] & 0x8F000000u) != 0u;  // parent is covered or is a flat root
            uint32_t fd = 0;
            if (!cov) {  // follow the node's leaf interval down
                uint32_t lo = 2u * j, hi = lo + 2u;
                for (uint32_t r = 1; d + r <= maxlen; r++) {
                    const uint32_t Lr = P.L[d + r];
                    if (hi <= Lr) { fd = r; break; }  // everything below is a leaf at relative depth r
                    if (lo < Lr) break;                // mixed: not complete
                    lo = 2u * (lo - Lr);
                    hi = 2u * (hi - Lr);
                }
                if (fd < 2u) fd = 0;
            }
            P.runoff[Bi + j] = (fd << 24) | (cov ? 0x80000000u : 0u);
            P.cnt[Bi + j] = 0;
        }
        wave_lds_fence();
    }
    return 0;
}

// Everything in front of pass 2 of the one-wave decoder: the tree, pass 1 (counts, run pointers, popcounts) and the sequence
// offsets. Returns 0 or a zxc error; R.single < 256: the degenerate one-symbol table (the caller fills the output).
struct PivPrep { const uint8_t* body; uint32_t bsize, maxlen, single; };
template <typename PL>
__device__ __forceinline__ int piv_prepare(const uint8_t* __restrict__ payload, uint32_t psize, uint32_t n, PL& P, int lane,
                                           const uint8_t* __restrict__ shared_lens, PivPrep& R) {
    R.single = 256u;
    R.maxlen = 0;
    const uint32_t hdr = shared_lens ? 0u : 128u;
    if (psize < hdr) return E_CORRUPT;
    if (n == 0u) return E_CORRUPT;
    R.body = payload + hdr;
    R.bsize = psize - hdr;
    PivTree T;
    const int trc = piv_tree(shared_lens ? shared_lens : payload, P, lane, T);
    if (trc != 0) return trc;
    const uint32_t maxlen = T.maxlen;
    const uint8_t* body = R.body;
    const uint32_t bsize = R.bsize;
    if (T.degenerate) {
        if (!T.ok1) return E_CORRUPT;
        const uint32_t nb = (n + 7u) >> 3;
        if (nb > bsize) return E_CORRUPT;
        uint32_t bad = 0;
        for (uint32_t i = lane; i < nb; i += 64u) {
            uint32_t b = ld8(body + i);
            if (i == nb - 1u && (n & 7u)) b &= (1u << (n & 7u)) - 1u;
            bad |= b;
        }
        if (__ballot(bad != 0u)) return E_CORRUPT;
        R.single = P.sorted[0];
        return 0;
    }

    PIVP(13);
    // ---- C. pass 1: counts and run pointers, one depth at a time
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
            if (emit) P.runoff[ii] = nf | ro;
            pcur += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            // popcounts: small runs (<= 64 bytes) by their own lane, big ones by the whole wave. Every load below is issued
            // by every lane and none depends on an earlier one (a byte loop with a load per step cost a memory round trip
            // per 4 bytes: ~180 K clocks per section, measured).
            const bool bitmap = emit && D == 0u;
            const bool small = bitmap && nbytes <= 64u;
            uint32_t ones = 0;
            if (bsize >= 64u && __ballot(small && ro + 64u > bsize) == 0ull) {
                // four 16-byte pieces of the lane's run (idle lanes: the body's first bytes), bits beyond the run masked off
                const uint8_t* rp = body + (small ? ro : 0u);
                const v4u a0 = g_ld128(rp), a1 = g_ld128(rp + 16), a2 = g_ld128(rp + 32), a3 = g_ld128(rp + 48);
                const uint32_t cb = small ? c : 0u;
                auto cnt32 = [&](uint32_t w, uint32_t base) -> uint32_t {  // bits [base, base + 32) of the run
                    const uint32_t nb = cb > base ? (cb - base >= 32u ? 32u : cb - base) : 0u;
                    return __popc(w & (nb >= 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u)));
                };
                ones = cnt32(a0.x, 0u) + cnt32(a0.y, 32u) + cnt32(a0.z, 64u) + cnt32(a0.w, 96u) + cnt32(a1.x, 128u) + cnt32(a1.y, 160u) +
                       cnt32(a1.z, 192u) + cnt32(a1.w, 224u) + cnt32(a2.x, 256u) + cnt32(a2.y, 288u) + cnt32(a2.z, 320u) +
                       cnt32(a2.w, 352u) + cnt32(a3.x, 384u) + cnt32(a3.y, 416u) + cnt32(a3.z, 448u) + cnt32(a3.w, 480u);
            } else if (small) {  // a run within 64 bytes of the section's end: byte loop
                const uint8_t* rp = body + ro;
                const uint32_t full = nbytes ? nbytes - 1u : 0u;
                uint32_t k = 0;
                for (; k + 4u <= full; k += 4u) ones += __popc(ld32(rp + k));
                for (; k < full; k++) ones += __popc(ld8(rp + k));
                if (nbytes) {
                    uint32_t last = ld8(rp + full);
                    if (c & 7u) last &= (1u << (c & 7u)) - 1u;
                    ones += __popc(last);
                }
            }
            uint64_t big = __ballot(bitmap && nbytes > 64u);
            while (big) {
                const int bl = __ffsll((unsigned long long)big) - 1;
                big &= big - 1ull;
                const uint32_t bro = (uint32_t)__builtin_amdgcn_readlane((int)ro, bl), bc = (uint32_t)__builtin_amdgcn_readlane((int)c, bl);
                const uint8_t* rp = body + bro;
                const uint32_t nwords = (bc + 63u) >> 6;
                uint32_t part = 0;
                for (uint32_t w0 = 0; w0 < nwords; w0 += 256u) {  // 2 KiB of bitmap per step: four 64-bit words per lane in flight
                    uint64_t x[4];
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const uint32_t wi = w0 + 64u * (uint32_t)t + (uint32_t)lane;
                        x[t] = g_ld64(rp + 8u * (wi < nwords ? wi : nwords - 1u));  // (the last word may reach up to 7 bytes past the run: inside the block or its slack)
                    }
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const uint32_t wi = w0 + 64u * (uint32_t)t + (uint32_t)lane;
                        const uint32_t left = wi < nwords ? bc - 64u * wi : 0u;
                        part += __popcll(x[t] & (left >= 64u ? ~0ull : ((1ull << left) - 1ull)));
                    }
                }
                const uint32_t tot = wave_sum(part);
                if (lane == bl) ones = tot;
            }
            if (bitmap) {  // children 2j, 2j+1 of depth d+1: only internal ones keep a count
                const uint32_t c0 = 2u * j, c1 = c0 + 1u;
                if (c0 >= Lc) P.cnt[Bc + c0 - Lc] = c - ones;
                if (c1 >= Lc) P.cnt[Bc + c1 - Lc] = ones;
            }
        }
        wave_lds_fence();
    }
    PIVP(14);
    // sequence offsets inside each depth's buffer: only emitting (internal, uncovered) nodes are materialised
    for (uint32_t d = 0; d < maxlen; d++) {
        const uint32_t Id = P.N[d] - P.L[d], Bi = P.ib[d];
        uint32_t acc = 0;
        for (uint32_t j0 = 0; j0 < Id; j0 += 64u) {
            const uint32_t j = j0 + lane;
            const uint32_t ii = Bi + (j < Id ? j : 0u);
            const bool emit = j < Id && !(P.runoff[ii] & 0x80000000u);
            const uint32_t c = emit ? P.cnt[ii] : 0u;
            const uint32_t incl = wave_scan_add(c);
            if (emit) P.seqoff[ii] = acc + incl - c;
            acc += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    wave_lds_fence();

    R.maxlen = maxlen;
    return 0;
}

// Decodes one section: payload[0..psize) -> out[0..n) (tmp: scratch of >= n bytes; shared_lens: the dictionary's 128-byte
// code-length table for enc_lit = 3, zxc_huffman.c:2467-2473, the payload then has no inline header). Returns 0 or a zxc error.
// (The unnamed last parameter is unused: it keeps the function's symbol, and so the code object, as it was; it goes with the
// decode kernels' dbg.)
__device__ int pivco_decode(const uint8_t* __restrict__ payload_, uint32_t psize, uint8_t* __restrict__ out_, uint32_t n,
                            uint8_t* __restrict__ tmp_, PivLds& P, int lane, const uint8_t* __restrict__ shared_lens_,
                            uint32_t) {
    const uint8_t* __restrict__ payload = uni_ptr(payload_);
    uint8_t* __restrict__ out = uni_ptr(out_);
    uint8_t* __restrict__ tmp = uni_ptr(tmp_);
    const uint8_t* __restrict__ shared_lens = uni_ptr(shared_lens_);
    psize = uni(psize);
    n = uni(n);
    PivPrep R;
    const int prc = piv_prepare(payload, psize, n, P, lane, shared_lens, R);
    if (prc != 0) return prc;
    if (R.single < 256u) {
        for (uint32_t i = lane; i < n; i += 64u) out[i] = (uint8_t)R.single;
        return 0;
    }
    const uint8_t* body = R.body;
    const uint32_t bsize = R.bsize, maxlen = R.maxlen;
    PIVP(6);
    // ---- D. pass 2: rebuild sequences bottom-up
    for (int d = (int)maxlen - 1; d >= 0; d--) {
        uint8_t* const buf_d = (d & 1) ? tmp : out;
        const uint8_t* const buf_c = (d & 1) ? out : tmp;  // children live one depth down
        piv_level(P, d, body, bsize, buf_d, buf_c, lane);
        __builtin_amdgcn_s_waitcnt(0);  // this depth's stores are out before the next depth gathers them (nt loads: L2)
        wave_lds_fence();
        PIVP(7);
    }
    return 0;
}
