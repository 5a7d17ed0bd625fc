// zxc_wave.h — the wave and load primitives of every device source, once: unaligned loads, readfirstlane, the DPP prefix sum,
// the xor-butterfly reductions and the byte copy. HIP only. Included by zxc_decode_kernel.hip, zxc_encode_kernel.hip and
// zxc_device_util.h; the .inc files get it through the file that includes them.
// Not here, on purpose: the LDS fences (each has its own scope and reasoning, next to its users) and the address-space /
// non-temporal loads and stores of zxc_pivco.inc (they select other instructions).
#ifndef ZXC_WAVE_H
#define ZXC_WAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef v4u __attribute__((aligned(1))) v4u_unaligned;

// loads of any byte alignment
__device__ __forceinline__ uint32_t ld8(const uint8_t* p) { return *p; }
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ v4u ld128(const uint8_t* p) { v4u v; __builtin_memcpy(&v, p, 16); return v; }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// wave-wide inclusive prefix sum (64 lanes) on the DPP crossbar: row_shr 1,2,4,8 scan each
// 16-lane row, row_bcast:15 / row_bcast:31 carry the row totals across (gfx9 DPP controls).
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(v), 63); }

// xor butterfly: op folded over all 64 lanes' values, the result in every lane (32-bit values, 64-bit ones as two halves)
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int d) { return __shfl_xor(v, d); }
__device__ __forceinline__ uint64_t lane_xor(uint64_t v, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, lane_xor(v, d));
    return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
    return wave_all(v, [](uint32_t a, uint32_t b) { return a ^ b; });
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
    return wave_all(v, [](T a, T b) { return b < a ? b : a; });
}

// d[0, n) = s[0, n) by `threads` threads, of which this is number t: 16-byte units of any alignment, bytes where the last unit
// passes n. Reads and writes exactly those n bytes.
__device__ __forceinline__ void copy_bytes(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint32_t n, uint32_t t, uint32_t threads) {
    for (uint32_t o = 16u * t; o < n; o += 16u * threads) {
        if (o + 16u <= n) {
            v4u v;
            __builtin_memcpy(&v, s + o, 16);
            __builtin_memcpy(d + o, &v, 16);
        } else {
            for (uint32_t k = o; k < n; k++) d[k] = s[k];
        }
    }
}
#endif
