// zxc_dict_device.hip — zxc_mi355x_dict_prepare_device: the id of a dictionary that lies in device memory, computed on the device.
//
// zxc_dict_id (zxc_host.c: dict_id_of) = rapidhash v3 of the content, seed 0, folded hi ^ lo to 32 bits; with a 128-byte shared
// literal table, rapidhash of the table seeded with that value, folded again. The id is what binds an archive to its dictionary:
// zxc_mi355x_compress_dict_device writes it into the file header, the decompress calls compare it with the header's. Computed
// here, once per dictionary, it lets all of them run without the host ever reading the dictionary or the archive.
//
// One wavefront. wave_checksum32 of zxc_rapidhash.inc is the same algorithm with seed 0 built in; this is its seeded sibling,
// kept in this file because the decode and encode kernels include that one and their code does not change for this call.
// The bulk loop is seven independent accumulators, one per lane, over at most 585 stripes of 112 bytes (65 535 bytes); the
// <= 112-byte tail and the finaliser run wave-uniform. Every load lies inside p[0, len).
#include "zxc_device_util.h"  // the host-side plumbing; zxc_container.h: ZC_DICT_MAX

#define DI_HUF_BYTES 128u
#define DI_DEPTH 8  // stripes of loads in flight per lane: the accumulator chain then runs at multiplier latency

__device__ __forceinline__ uint64_t di_ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint64_t di_ld32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t di_mix(uint64_t a, uint64_t b) { return (a * b) ^ __umul64hi(a, b); }

// rapidhash v3 of p[0, len) with `seed`, folded to 32 bits; the same value in every lane.
__device__ uint32_t di_wave_hash32(const uint8_t* __restrict__ p, uint32_t len, uint64_t seed, int lane) {
    const uint64_t S[8] = {0x2d358dccaa6c78a5ull, 0x8bb84b93962eacc9ull, 0x4b33a62ed433d4a3ull, 0x4d5a2da51de1aa47ull,
                           0xa0761d6478bd642full, 0xe7037ed1a0b428dbull, 0x90ed1765281c388cull, 0xaaaaaaaaaaaaaaaaull};
    seed ^= di_mix(seed ^ S[2], S[1]);
    uint64_t a = 0, b = 0;
    uint64_t i = len;
    if (len <= 16u) {
        if (len >= 4u) {
            seed ^= len;
            if (len >= 8u) { a = di_ld64(p); b = di_ld64(p + len - 8); }
            else { a = di_ld32(p); b = di_ld32(p + len - 4); }
        } else if (len > 0u) {
            a = ((uint64_t)p[0] << 45) | p[len - 1];
            b = p[len >> 1];
        }
    } else {
        if (len > 112u) {
            const uint32_t T = (len - 1u) / 112u;  // stripes consumed by the do / while (i > 112) loop: 112 T <= len - 1
            uint64_t s = seed, sk = S[0];
#pragma unroll
            for (int k = 1; k < 7; k++) if (lane == k) sk = S[k];
            if (lane < 7) {
                const uint8_t* q = p + 16 * lane;
                uint32_t t = 0;
                for (; t + DI_DEPTH <= T; t += DI_DEPTH, q += 112 * DI_DEPTH) {
                    uint64_t lo[DI_DEPTH], hi[DI_DEPTH];
#pragma unroll
                    for (int j = 0; j < DI_DEPTH; j++) { lo[j] = di_ld64(q + 112 * j); hi[j] = di_ld64(q + 112 * j + 8); }
#pragma unroll
                    for (int j = 0; j < DI_DEPTH; j++) s = di_mix(lo[j] ^ sk, hi[j] ^ s);
                }
                for (; t < T; t++, q += 112) s = di_mix(di_ld64(q) ^ sk, di_ld64(q + 8) ^ s);
            }
            uint64_t x = (lane < 7) ? s : 0ull;  // seed = the seven accumulators XORed together
#pragma unroll
            for (int d = 4; d >= 1; d >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)x, d), hi = __shfl_xor((uint32_t)(x >> 32), d);
                x ^= ((uint64_t)hi << 32) | lo;
            }
            const uint32_t lo0 = __builtin_amdgcn_readfirstlane((uint32_t)x), hi0 = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
            seed = ((uint64_t)hi0 << 32) | lo0;
            p += 112ull * T;
            i -= 112ull * T;  // 1..112 (the last 16 bytes below may start in front of p: still inside the buffer)
        }
        if (i > 16) {
            seed = di_mix(di_ld64(p) ^ S[2], di_ld64(p + 8) ^ seed);
            if (i > 32) {
                seed = di_mix(di_ld64(p + 16) ^ S[2], di_ld64(p + 24) ^ seed);
                if (i > 48) {
                    seed = di_mix(di_ld64(p + 32) ^ S[1], di_ld64(p + 40) ^ seed);
                    if (i > 64) {
                        seed = di_mix(di_ld64(p + 48) ^ S[1], di_ld64(p + 56) ^ seed);
                        if (i > 80) {
                            seed = di_mix(di_ld64(p + 64) ^ S[2], di_ld64(p + 72) ^ seed);
                            if (i > 96) seed = di_mix(di_ld64(p + 80) ^ S[1], di_ld64(p + 88) ^ seed);
                        }
                    }
                }
            }
        }
        a = di_ld64(p + i - 16) ^ i;
        b = di_ld64(p + i - 8);
    }
    a ^= S[1];
    b ^= seed;
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    const uint64_t h = di_mix(lo ^ S[7], hi ^ S[1] ^ i);
    return (uint32_t)(h ^ (h >> 32));
}

extern "C" __global__ void __launch_bounds__(64)
zxc_dict_id_kernel(const uint8_t* __restrict__ content, uint32_t size, const uint8_t* __restrict__ huf, uint32_t* __restrict__ id) {
    const int lane = (int)threadIdx.x;
    uint32_t h = di_wave_hash32(content, size, 0ull, lane);
    if (huf) h = di_wave_hash32(huf, DI_HUF_BYTES, (uint64_t)h, lane);
    if (lane == 0) *id = h;
}

extern "C" int zxc_mi355x_dict_prepare_device(const void* d_content, uint32_t size, const void* d_huf, uint32_t* d_id, void* stream) {
    if (!d_content || !d_id || size == 0u) return ZXC_ERROR_NULL_INPUT;
    if (size > ZC_DICT_MAX) return ZXC_ERROR_DICT_TOO_LARGE;
    if (!have_device()) return ZXC_ERROR_GPU_UNAVAILABLE;
    hipLaunchKernelGGL(zxc_dict_id_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)d_content, size,
                       (const uint8_t*)d_huf, d_id);
    return launched() ? ZXC_OK : ZXC_ERROR_GPU_UNAVAILABLE;
}
