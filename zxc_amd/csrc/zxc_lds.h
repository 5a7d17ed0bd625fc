/* zxc_lds.h — the LDS access points of the sequence executor.
 *
 * Every LDS access of run_sequences() and its helpers goes through these, for two reasons:
 * the code says which DS instruction it means (aligned dword / 16-byte accesses, byte stores,
 * ds_or_b32), and a test harness may pre-define ZXC_LDS_HOOKS plus the same names to observe the
 * accesses (tests/wave_emu models the wave's lock-step LDS semantics on a CPU with them).
 * Discipline assumed by callers: a value written by one lane may be read by ANOTHER lane only
 * after wave_lds_fence(); write-after-read between lanes needs nothing (one wave's DS
 * instructions execute in program order). */
#ifndef ZXC_LDS_H
#define ZXC_LDS_H
#ifndef ZXC_LDS_HOOKS
#define LDS_LD8(p) ((uint32_t)*(const uint8_t*)(p))
#define LDS_LD32(p) (*(const uint32_t*)(p))
#define LDS_LD128(p) (*(const v4u*)(p))
#define LDS_ST8(p, v) (*(uint8_t*)(p) = (uint8_t)(v))
#define LDS_ST32(p, v) (*(uint32_t*)(p) = (uint32_t)(v))
#define LDS_ST128(p, v) (*(v4u*)(p) = (v))
/* ds_or_b32 (no return): bytes of different lanes meet in one dword without a read-modify-write in registers */
#define LDS_OR32(p, v) ((void)__hip_atomic_fetch_or((uint32_t*)(p), (uint32_t)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
#endif

/* Path markers. ZXC_PATH(id) names a branch of the sequence executors and their helpers. It expands to nothing in every
 * product and experiment build; the CPU wave emulator's hooks count, per id, the lanes that pass it, and
 * tests/decode_limit_cases.py asks of every crafted block that it reaches the branches it was built for. Wave-uniform events
 * are marked under `lane == 0` so that they count once. Prefixes: X_ which executor / stream set-up ran, L_ the lean executor
 * (zxc_seq_lean.inc), F_ the full executor (run_sequences), C_ the shared helpers. The tests read this list by name. */
enum zxc_path_id {
    X_LEAN, X_LEAN_GHI, X_FULL, X_FULL_GHI, X_SETUP_RLE, X_SETUP_PRE, X_SETUP_RAW,
    L_VARINT_FAST, L_VARINT_GENERAL, L_VARINT_CUT, L_EXACT, L_ERR, L_TILE_CUT, L_DEAD, L_CARRY4X,
    L_GIANT, L_GIANT_LIT_PIECE, L_GIANT_MATCH, L_LIT_GROUP, L_LIT_5TH, L_LIT_LONG,
    L_FAR_GROUP, L_FAR_5TH, L_FAR_NO_ML, L_FAR_NO_QA4, L_FAR_NO_FLUSHED, L_FAR_NO_EDGE, L_FAR_OFF,
    L_WAIT_ALL, L_REDIRECT0, L_REDIRECT1, L_REDIRECT_NO_RING, L_STEPABLE, L_BYTEWISE, L_LONG, L_LONG_FAR,
    L_SPARSE, L_SPARSE_OVL, L_SPARSE_PLAIN, L_SPARSE_COOP, L_PARTIAL_CHUNK,
    F_VARINT_FAST, F_VARINT_GENERAL, F_ERR, F_TILE_CUT, F_DEAD, F_CARRY4X,
    F_GIANT, F_GIANT_LIT_PIECE, F_GIANT_MATCH, F_LIT_GROUP, F_LIT_LONG, F_FROM_DICT,
    F_FAR_PREFETCH, F_FAR_GROUP, F_REDIRECT0, F_REDIRECT1, F_STEPABLE, F_BYTEWISE, F_LONG,
    F_SPARSE, F_SPARSE_OVL, F_SPARSE_PLAIN, F_SPARSE_COOP, F_PARTIAL_CHUNK,
    C_COPY_FAR, C_COPY_DICT_GATHER, C_MATCH_DOUBLE, C_VARINT_TAIL, C_VARINT_BAD,
    ZXC_PATH_COUNT
};
#ifndef ZXC_PATH
#define ZXC_PATH(id) do { } while (0)
#endif
#endif
