/* zxc_shuffle.h — the rules of the byte-shuffle filter (include/zxc_mi355x_shuffle.h, kernels and calls in zxc_shuffle_device.hip):
 * the index map, the per-lane move plan of the kernels, and the byte placement inside a lane's registers. Plain inline C that hipcc
 * and a host C compiler both take, so that the kernels and the CPU tests (tests/shuffle/shuffle_replay.h) run the same lines.
 *
 * The transform, per unit (a power of two in [4 KiB, 2 MiB]; the archive calls use the block size). Unit u covers bytes
 * [u unit, min((u + 1) unit, n)); with m its length, E the element size, q = m / E and r = m % E:
 *   out[u unit + k q + i] = in[u unit + i E + k]   for k < E, i < q     (plane k holds byte k of every element)
 * and the last r bytes of the unit are copied. Only the final unit can have r != 0 or q not a multiple of 16.
 *
 * The plan. A group is 16 consecutive elements of one unit: 16 E contiguous bytes on the element side, 16 bytes in each of the E
 * planes. Groups are numbered through the buffer, G = 0 .. groups - 1: first those of the full units (unit / (16 E) each), then the
 * q_last / 16 whole groups of the ragged last unit. Because a full unit holds exactly unit / (16 E) groups, group G's element side
 * starts at byte 16 E G whichever unit it lies in. A wavefront owns ZSH_WAVE_BYTES = 8 KiB of the element side, that is
 * 512 / E groups in 8 / E turns of 64 lanes: in a turn lane l owns group wave x 512 / E + turn x 64 + l, so the 64 lanes' 16-byte
 * accesses to a plane are contiguous (1 KiB; with E = 8 and a 4 KiB unit two runs of 512 bytes, one per unit), and a lane's
 * element side is one run of 16 E bytes. The number of wavefronts, ceil(n / 8 KiB), does not depend on E. What the groups leave
 * over, the last q_last % 16 elements of the ragged unit and its r copied bytes (at most 15 E + E - 1 = 127 bytes), the last
 * wavefront moves a byte at a time: byte j of them by lane j % 64. Every access of a group is 16 bytes wide at whatever alignment
 * the caller's pointer and, in the ragged unit, q_last give it; there is no byte-wide access outside those leftovers. */
#ifndef ZXC_SHUFFLE_H
#define ZXC_SHUFFLE_H
#include "../../include/zxc_mi355x_shuffle.h"
#include "zxc_container.h"

#define ZSH_WAVE_BYTES 8192u /* element-side bytes one wavefront moves */
#define ZSH_GROUP 16u        /* elements of a group: the bytes of one plane access */

ZC_FN int zsh_elem_ok(uint32_t E) { return E == 2u || E == 4u || E == 8u; }
ZC_FN int zsh_unit_ok(uint64_t unit) { return zc_block_size_ok(unit); }

/* where byte p of the plain buffer of n bytes lies in the shuffled one (the definition; the kernels never call it) */
ZC_FN uint64_t zsh_index(uint64_t p, uint64_t n, uint32_t E, uint32_t unit) {
    const uint64_t at = p / unit * unit, m = n - at < unit ? n - at : unit, q = m / E, j = p - at;
    return j >= q * E ? p : at + (j % E) * q + j / E;
}

typedef struct zsh_plan {
    uint64_t groups, full_groups, last_at, waves; /* last_at: where the ragged unit starts (n when there is none) */
    uint32_t E, unit, q_full, q_last, unit_groups, unit_groups_lg, wave_groups, ragged; /* ragged: bytes moved one at a time */
} zsh_plan_t;

/* for arguments zsh_elem_ok and zsh_unit_ok accept */
ZC_FN zsh_plan_t zsh_plan(uint64_t n, uint32_t E, uint32_t unit) {
    zsh_plan_t p;
    const uint64_t n_full = n / unit, m = n - n_full * unit;
    p.E = E; p.unit = unit;
    p.q_full = unit / E; p.q_last = (uint32_t)(m / E);
    p.unit_groups = p.q_full / ZSH_GROUP; /* a power of two, at least 32 */
    p.unit_groups_lg = 0;
    while ((1u << p.unit_groups_lg) < p.unit_groups) p.unit_groups_lg++;
    p.full_groups = n_full * p.unit_groups;
    p.groups = p.full_groups + p.q_last / ZSH_GROUP;
    p.last_at = n_full * unit;
    p.wave_groups = ZSH_WAVE_BYTES / (ZSH_GROUP * E);
    p.waves = n / ZSH_WAVE_BYTES + (n % ZSH_WAVE_BYTES != 0);
    p.ragged = (p.q_last % ZSH_GROUP) * E + (uint32_t)(m % E);
    return p;
}

/* The group lane `lane` of wavefront `wave` owns in turn `turn`: -> 0 when it owns none, else 1 and where the group's 16 E element
 * bytes start, where its 16 bytes of plane 0 start, and the distance from one plane to the next (the unit's q). */
typedef struct zsh_group { uint64_t elem_at, plane_at; uint32_t q; } zsh_group_t;
ZC_FN int zsh_group(const zsh_plan_t* p, uint64_t wave, uint32_t turn, uint32_t lane, zsh_group_t* g) {
    const uint64_t G = wave * p->wave_groups + turn * 64u + lane;
    if (G >= p->groups) return 0;
    g->elem_at = G * (ZSH_GROUP * p->E);
    if (G < p->full_groups) {
        g->plane_at = (G >> p->unit_groups_lg) * p->unit + (G & (p->unit_groups - 1u)) * ZSH_GROUP;
        g->q = p->q_full;
    } else {
        g->plane_at = p->last_at + (G - p->full_groups) * ZSH_GROUP;
        g->q = p->q_last;
    }
    return 1;
}

/* Leftover byte j < ragged of the last unit, which the last wavefront (waves - 1) moves: its place in the plain buffer and in the
 * shuffled one. First plane by plane the bytes of the elements behind the last whole group, then the r copied bytes. */
ZC_FN void zsh_ragged_byte(const zsh_plan_t* p, uint32_t j, uint64_t* plain, uint64_t* shuffled) {
    const uint32_t left = p->q_last % ZSH_GROUP, i0 = p->q_last - left;
    if (j < left * p->E) {
        const uint32_t k = j / left, i = i0 + j % left;
        *plain = p->last_at + (uint64_t)i * p->E + k;
        *shuffled = p->last_at + (uint64_t)k * p->q_last + i;
    } else {
        *plain = *shuffled = p->last_at + (uint64_t)p->q_last * p->E + (j - left * p->E);
    }
}

/* ---- where each byte goes inside a lane: 4 E dwords of 16 elements <-> E planes of 4 dwords, with v_perm_b32 alone.
 * ZSH_PERM(hi, lo, sel): byte b of the result is byte sel.b of the eight bytes {hi, lo}, 0 .. 3 in lo and 4 .. 7 in hi. */
#if defined(__HIP_DEVICE_COMPILE__)
#define ZSH_PERM(hi, lo, sel) __builtin_amdgcn_perm((hi), (lo), (sel))
#else
ZC_FN uint32_t zsh_perm_host(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (uint32_t b = 0; b < 4u; b++) r |= (uint32_t)((both >> (8u * ((sel >> (8u * b)) & 7u))) & 0xFFu) << (8u * b);
    return r;
}
#define ZSH_PERM(hi, lo, sel) zsh_perm_host((hi), (lo), (sel))
#endif

/* the 4 x 4 byte transpose: o[r] byte c = in_c byte r. It is its own inverse. */
ZC_FN void zsh_t4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t* o0, uint32_t* o1, uint32_t* o2, uint32_t* o3) {
    const uint32_t x0 = ZSH_PERM(b, a, 0x05010400u), x1 = ZSH_PERM(b, a, 0x07030602u); /* a0 b0 a1 b1 | a2 b2 a3 b3 */
    const uint32_t y0 = ZSH_PERM(d, c, 0x05010400u), y1 = ZSH_PERM(d, c, 0x07030602u);
    *o0 = ZSH_PERM(y0, x0, 0x05040100u); *o1 = ZSH_PERM(y0, x0, 0x07060302u);
    *o2 = ZSH_PERM(y1, x1, 0x05040100u); *o3 = ZSH_PERM(y1, x1, 0x07060302u);
}
/* e[0, 4 E): the group's element side as dwords; p[4 k + j]: dword j of its 16 bytes of plane k. E is a constant where the
 * kernels call these, so the loops unroll and both arrays stay in registers. */
ZC_FN void zsh_regs_shuffle(const uint32_t* e, uint32_t* p, uint32_t E) {
    if (E == 2u) {
        for (uint32_t j = 0; j < 4u; j++) {
            p[j] = ZSH_PERM(e[2u * j + 1u], e[2u * j], 0x06040200u);
            p[4u + j] = ZSH_PERM(e[2u * j + 1u], e[2u * j], 0x07050301u);
        }
        return;
    }
    const uint32_t w = E / 4u; /* dwords of an element */
    for (uint32_t h = 0; h < w; h++)
        for (uint32_t j = 0; j < 4u; j++)
            zsh_t4(e[(4u * j) * w + h], e[(4u * j + 1u) * w + h], e[(4u * j + 2u) * w + h], e[(4u * j + 3u) * w + h],
                   &p[16u * h + j], &p[16u * h + 4u + j], &p[16u * h + 8u + j], &p[16u * h + 12u + j]);
}
ZC_FN void zsh_regs_unshuffle(const uint32_t* p, uint32_t* e, uint32_t E) {
    if (E == 2u) {
        for (uint32_t j = 0; j < 4u; j++) {
            e[2u * j] = ZSH_PERM(p[4u + j], p[j], 0x05010400u);
            e[2u * j + 1u] = ZSH_PERM(p[4u + j], p[j], 0x07030602u);
        }
        return;
    }
    const uint32_t w = E / 4u;
    for (uint32_t h = 0; h < w; h++)
        for (uint32_t j = 0; j < 4u; j++)
            zsh_t4(p[16u * h + j], p[16u * h + 4u + j], p[16u * h + 8u + j], p[16u * h + 12u + j],
                   &e[(4u * j) * w + h], &e[(4u * j + 1u) * w + h], &e[(4u * j + 2u) * w + h], &e[(4u * j + 3u) * w + h]);
}

/* ---- the archive calls: the chunk and the work areas.
 * ZSH_DEFAULT_PIECE: what max_piece == 0 stands for. A chunk is the stage's size: the extra device memory of a call. 64 MiB is
 * 128 blocks of 512 KiB in an encode or decode launch, one wavefront each. */
#define ZSH_DEFAULT_PIECE (64ull << 20)
/* The chunk of a call over `total` bytes: max_piece (or the default) rounded down to whole blocks, and no more than the source
 * rounded up to whole blocks (one block for an empty one). For a block size the format has and max_piece == 0 or >= block_size. */
ZC_FN uint64_t zsh_piece(uint64_t total, uint64_t max_piece, uint32_t block_size) {
    const uint64_t want = (max_piece ? max_piece : ZSH_DEFAULT_PIECE) / block_size * block_size;
    const uint64_t blocks = total / block_size + (total % block_size != 0);
    if (blocks > 0x7FFFFFFFull) return want; /* (more blocks than a session counts: it refuses them) */
    const uint64_t all = (blocks ? blocks : 1u) * block_size;
    return want < all ? want : all;
}
/* The stage lies behind the session's work area, on the next multiple of 256: session + 256 + piece bytes in all. */
#define ZSH_STAGE_ALIGN 256u
#endif
