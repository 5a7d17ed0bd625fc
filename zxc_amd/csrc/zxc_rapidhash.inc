// zxc_rapidhash.inc — block checksum for one wavefront: rapidhash v3 (the reference vendors
// it: src/lib/vendors/rapidhash.h; zxc_checksum folds the 64-bit hash hi^lo to 32 bits,
// src/lib/zxc_internal.h:1353-1359). Restated from the published algorithm: the bulk loop is
// seven independent 16-byte lanes per 112-byte stripe — here literally seven SIMD lanes, each
// carrying one accumulator (the algorithm has no more parallelism than that: every accumulator is a
// serial chain over the stripes); the <= 112-byte tail and the finaliser run wave-uniform.
__device__ __forceinline__ uint64_t rh_mix(uint64_t a, uint64_t b) { return (a * b) ^ __umul64hi(a, b); }

__device__ uint32_t wave_checksum32(const uint8_t* __restrict__ p, uint32_t len, int lane) {
    const uint64_t S[8] = {0x2d358dccaa6c78a5ull, 0x8bb84b93962eacc9ull, 0x4b33a62ed433d4a3ull, 0x4d5a2da51de1aa47ull,
                           0xa0761d6478bd642full, 0xe7037ed1a0b428dbull, 0x90ed1765281c388cull, 0xaaaaaaaaaaaaaaaaull};
    uint64_t seed = rh_mix(S[2], S[1]);  // seed 0: seed ^= mix(seed ^ S2, S1)
    uint64_t a = 0, b = 0;
    uint64_t i = len;
    if (len <= 16u) {
        if (len >= 4u) {
            seed ^= len;
            if (len >= 8u) { a = ld64(p); b = ld64(p + len - 8); }
            else { a = ld32(p); b = ld32(p + len - 4); }
        } else if (len > 0u) {
            a = ((uint64_t)p[0] << 45) | p[len - 1];
            b = p[len >> 1];
        }
    } else {
        if (len > 112u) {
            const uint32_t T = (len - 1u) / 112u;  // stripes consumed by the do/while (i > 112) loop
            uint64_t s = seed;
            uint64_t sk = S[0];
#pragma unroll
            for (int k = 1; k < 7; k++) if (lane == k) sk = S[k];
            if (lane < 7) {
                // The accumulator chain is serial (two 64-bit multiplies per stripe), the loads are not: eight
                // stripes are requested together so that the chain runs at multiplier latency, not memory latency.
                const uint8_t* q = p + 16 * lane;
                uint32_t t = 0;
                for (; t + 8u <= T; t += 8u, q += 896) {
                    uint64_t lo[8], hi[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) { lo[j] = ld64(q + 112 * j); hi[j] = ld64(q + 112 * j + 8); }
#pragma unroll
                    for (int j = 0; j < 8; j++) s = rh_mix(lo[j] ^ sk, hi[j] ^ s);
                }
                for (; t < T; t++, q += 112) s = rh_mix(ld64(q) ^ sk, ld64(q + 8) ^ s);
            }
            uint64_t x = (lane < 7) ? s : 0ull;  // seed ^= see1..see6 (all seven XORed together)
#pragma unroll
            for (int d = 4; d >= 1; d >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)x, d), hi = __shfl_xor((uint32_t)(x >> 32), d);
                x ^= ((uint64_t)hi << 32) | lo;
            }
            const uint32_t lo0 = __builtin_amdgcn_readfirstlane((uint32_t)x), hi0 = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
            seed = ((uint64_t)hi0 << 32) | lo0;
            p += 112ull * T;
            i -= 112ull * T;
        }
        if (i > 16) {
            seed = rh_mix(ld64(p) ^ S[2], ld64(p + 8) ^ seed);
            if (i > 32) {
                seed = rh_mix(ld64(p + 16) ^ S[2], ld64(p + 24) ^ seed);
                if (i > 48) {
                    seed = rh_mix(ld64(p + 32) ^ S[1], ld64(p + 40) ^ seed);
                    if (i > 64) {
                        seed = rh_mix(ld64(p + 48) ^ S[1], ld64(p + 56) ^ seed);
                        if (i > 80) {
                            seed = rh_mix(ld64(p + 64) ^ S[2], ld64(p + 72) ^ seed);
                            if (i > 96) seed = rh_mix(ld64(p + 80) ^ S[1], ld64(p + 88) ^ seed);
                        }
                    }
                }
            }
        }
        a = ld64(p + i - 16) ^ i;
        b = ld64(p + i - 8);
    }
    a ^= S[1];
    b ^= seed;
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    const uint64_t h = rh_mix(lo ^ S[7], hi ^ S[1] ^ i);
    return (uint32_t)(h ^ (h >> 32));
}

// ------------------------------------------------------------------ nine blocks per wavefront (round 6)
#define RH_GROUP_DEPTH 8   // stripes of loads in flight per lane. (Round 6 also tried to fit the kernel BESIDE six lean waves per SIMD — 32 VGPRs: depth 1
                           // still needs 34-36, one granule too many — so its waves take the place of decode waves while they run.)
// The bulk loop has seven accumulators per block and no more: hashed inside the decode kernels, 57 of a wave's 64 lanes idle through
// ~290 stripes of two 64-bit multiplies each (the checksummed decode cost 10.5 % of the launch in rounds 4-5). Here lanes 7 g .. 7 g + 6
// hash block g of nine (lane 63 idles), every lane of a group carrying one accumulator of ITS block; the <= 112-byte tail and the
// finaliser are computed by all seven lanes of the group alike (same inputs, same result). Returns the group's checksum in every lane
// of the group; len / p are per lane (equal within a group), T_max = the wave's longest bulk loop.
__device__ __forceinline__ uint64_t rh_group7_xor(uint64_t x, int lane, int sub) {
    // XOR over the seven lanes of my group: gather the other six (groups are not aligned to anything a DPP pattern knows)
    uint64_t r = x;
    const int base = lane - sub;
#pragma unroll
    for (int k = 1; k < 7; k++) {
        const int from = base + (sub + k >= 7 ? sub + k - 7 : sub + k);
        const uint32_t lo = __shfl((uint32_t)x, from), hi = __shfl((uint32_t)(x >> 32), from);
        r ^= ((uint64_t)hi << 32) | lo;
    }
    return r;
}
__device__ __forceinline__ uint32_t group_checksum32(const uint8_t* __restrict__ p, uint32_t len, int lane, const bool on) {
    const uint64_t S[8] = {0x2d358dccaa6c78a5ull, 0x8bb84b93962eacc9ull, 0x4b33a62ed433d4a3ull, 0x4d5a2da51de1aa47ull,
                           0xa0761d6478bd642full, 0xe7037ed1a0b428dbull, 0x90ed1765281c388cull, 0xaaaaaaaaaaaaaaaaull};
    const int sub = lane % 7;
    uint64_t seed = rh_mix(S[2], S[1]);
    uint64_t a = 0, b = 0;
    uint64_t i = len;
    const uint32_t T = (on && len > 112u) ? (len - 1u) / 112u : 0u;  // stripes of my block's bulk loop
    uint32_t Tmax = T;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t t = __shfl_xor(Tmax, d); Tmax = t > Tmax ? t : Tmax; }
    Tmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)Tmax);  // (a scalar: the loop's bound costs no vector register)
    {
        uint64_t s = seed, sk = S[0];
#pragma unroll
        for (int k = 1; k < 7; k++) if (sub == k) sk = S[k];
        // A lane's 16 bytes of a stripe start at p + 112 t + 16 sub: any byte alignment, and a byte-unaligned vector load costs the CU's
        // address path a clock or more per LANE (profiles/r3_vmem_test.log) — beside a decode that keeps that path 84 % busy. So the
        // lanes load 16-byte ALIGNED chunks (chunk k = the block's aligned base + 16 k; lane sub of stripe t holds chunk 7 t + sub), take
        // the chunk behind theirs from their neighbour (lane + 1; the group's last lane: the group's first lane, next stripe) and shift
        // the pair by the block's byte phase: 9 loads of ~2 lines per group instead of 16 serialised ones per 8 stripes.
        const uint32_t ph = (uint32_t)(uintptr_t)p & 15u;
        const uint8_t* pa = p - ph + 16 * sub;
#define RH_FIRST (lane - sub)
#define RH_R (ph & 3u)
        for (uint32_t t = 0; t < Tmax; t += RH_GROUP_DEPTH) {
            v4u A[RH_GROUP_DEPTH + 1];
#pragma unroll
            for (int j = 0; j < RH_GROUP_DEPTH + 1; j++) {
                // (stripe T = the chunk behind the bulk loop's last byte: only the group's first lane needs it, and its 16 bytes end at most
                //  15 bytes behind the payload; every other lane stays inside the bulk loop's bytes)
                const uint32_t tend = sub == 0 ? T : T - 1u;
                const uint32_t tj = t + (uint32_t)j < tend ? t + (uint32_t)j : tend;
                A[j] = T ? *(const v4u*)(pa + 112ull * tj) : (v4u){0, 0, 0, 0};
            }
#pragma unroll
            for (int j = 0; j < RH_GROUP_DEPTH; j++) {
                v4u B;  // the chunk behind mine
                {
                    const uint32_t n0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)A[j].x, 0x130, 0xf, 0xf, false), n1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)A[j].y, 0x130, 0xf, 0xf, false),
                                   n2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)A[j].z, 0x130, 0xf, 0xf, false), n3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)A[j].w, 0x130, 0xf, 0xf, false);  // wave_shl:1
                    const uint32_t w0 = __shfl(A[j + 1].x, RH_FIRST), w1 = __shfl(A[j + 1].y, RH_FIRST), w2 = __shfl(A[j + 1].z, RH_FIRST), w3 = __shfl(A[j + 1].w, RH_FIRST);
                    B.x = sub == 6 ? w0 : n0; B.y = sub == 6 ? w1 : n1; B.z = sub == 6 ? w2 : n2; B.w = sub == 6 ? w3 : n3;
                }
                // dwords ph / 4 .. ph / 4 + 4 of {A[j], B}, shifted by ph % 4 bytes
                uint32_t W0 = A[j].x, W1 = A[j].y, W2 = A[j].z, W3 = A[j].w, W4 = B.x, W5 = B.y, W6 = B.z, W7 = B.w;
                if (ph & 8u) { W0 = W2; W1 = W3; W2 = W4; W3 = W5; W4 = W6; W5 = W7; }
                if (ph & 4u) { W0 = W1; W1 = W2; W2 = W3; W3 = W4; W4 = W5; }
                const uint32_t d0 = __builtin_amdgcn_alignbyte(W1, W0, RH_R), d1 = __builtin_amdgcn_alignbyte(W2, W1, RH_R),
                               d2 = __builtin_amdgcn_alignbyte(W3, W2, RH_R), d3 = __builtin_amdgcn_alignbyte(W4, W3, RH_R);
                const uint64_t lo = (uint64_t)d0 | ((uint64_t)d1 << 32), hi = (uint64_t)d2 | ((uint64_t)d3 << 32);
                const uint64_t m = rh_mix(lo ^ sk, hi ^ s);
                s = t + (uint32_t)j < T ? m : s;
            }
        }
        const uint64_t x = rh_group7_xor(s, lane, sub);
        if (T) seed = x;
    }
    if (!on) return 0u;
    p += 112ull * T;
    i -= 112ull * T;  // (behind every cross-lane operation: idle groups took part in them)
    if (len <= 16u) {
        if (len >= 4u) {
            seed ^= len;
            if (len >= 8u) { a = ld64(p); b = ld64(p + len - 8); }
            else { a = ld32(p); b = ld32(p + len - 4); }
        } else if (len > 0u) {
            a = ((uint64_t)p[0] << 45) | p[len - 1];
            b = p[len >> 1];
        }
    } else {
        if (i > 16) {
            seed = rh_mix(ld64(p) ^ S[2], ld64(p + 8) ^ seed);
            if (i > 32) {
                seed = rh_mix(ld64(p + 16) ^ S[2], ld64(p + 24) ^ seed);
                if (i > 48) {
                    seed = rh_mix(ld64(p + 32) ^ S[1], ld64(p + 40) ^ seed);
                    if (i > 64) {
                        seed = rh_mix(ld64(p + 48) ^ S[1], ld64(p + 56) ^ seed);
                        if (i > 80) {
                            seed = rh_mix(ld64(p + 64) ^ S[2], ld64(p + 72) ^ seed);
                            if (i > 96) seed = rh_mix(ld64(p + 80) ^ S[1], ld64(p + 88) ^ seed);
                        }
                    }
                }
            }
        }
        a = ld64(p + i - 16) ^ i;
        b = ld64(p + i - 8);
    }
    a ^= S[1];
    b ^= seed;
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    const uint64_t h = rh_mix(lo ^ S[7], hi ^ S[1] ^ i);
    return (uint32_t)(h ^ (h >> 32));
}
