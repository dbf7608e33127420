// prio_ladder.h -- the arithmetic of the issue-priority ladder (engine_core.h prio_update): which
// s_setprio level a wave runs at after p of its launch's T hops, and the hop count at which that
// next changes.  Plain C++ (no HIP types; constexpr, so host and device code both call it):
// tests/test_prio_ladder.py compiles this very header with g++.
//
// The ladder has a fixed part and a chunked part, chosen at compile time:
//
//   PRISMA_PRIO_HYBRID_FROM = K (0..4): the first K of the fixed thresholds 5/8, 13/16, 15/16 of T
//     hold as they always did (level 3 below 5/8, 2 below 13/16, 1 below 15/16); from the K-th
//     threshold on the chunked part takes over.  0: chunks from the first hop (the cyclic ladder);
//     4: the fixed thresholds alone (level 0 from 15/16 to the end, no chunks).
//   PRISMA_PRIO_CHUNKS (a power of two): the chunked part's chunks are 2^s hops with
//     2^s <= T / PRISMA_PRIO_CHUNKS < 2^(s+1) (prio_ladder_shift, computed once per launch).  Chunk
//     c, counted from where the chunked part starts, runs at level (3 - K - c) & 3: the level steps
//     down from the fixed part's last one and wraps 0 -> 3, so of two waves less than four chunks
//     apart the one ahead has the lower priority except across the wrap, where the leader meets its
//     own level 0 again four chunks later -- the spread oscillates within about four chunks instead
//     of growing over a long last level.
//
// T below PRISMA_PRIO_CHUNKS: the shift is 31 (one chunk longer than any T: the chunked part is one
// level and never switches).  Only shifts, adds and compares: the same thresholds written with
// 64-bit products cost the headline kernel 2.3 % (profiles/r06_ab/ab_prio.txt, run 3).
#pragma once
#include <stdint.h>

// Shipped: the cyclic ladder with 128 chunks (profiles/prio_ladder/ab_sweep.txt: headline +4.4 %
// and config 3 +2.9 % against the fixed thresholds alone; 256 chunks the same within the same-code
// spread, 64 and 32 less; every hybrid lost 5 % -- after a fixed part at one level the waves are
// further than four chunks apart, where the cyclic levels no longer order them).
#ifndef PRISMA_PRIO_CHUNKS
#define PRISMA_PRIO_CHUNKS 128
#endif
#ifndef PRISMA_PRIO_HYBRID_FROM
#define PRISMA_PRIO_HYBRID_FROM 0
#endif

constexpr uint32_t kPrioNever = 0xffffffffu;         // "no further boundary in this launch"
constexpr uint32_t kPrioChunks = PRISMA_PRIO_CHUNKS, kPrioFrom = PRISMA_PRIO_HYBRID_FROM;
static_assert(kPrioChunks >= 4u && kPrioChunks <= 65536u && (kPrioChunks & (kPrioChunks - 1u)) == 0u,
              "PRISMA_PRIO_CHUNKS is a power of two");
static_assert(kPrioFrom <= 4u, "PRISMA_PRIO_HYBRID_FROM counts fixed thresholds (0..4)");

#define PRIO_INLINE __attribute__((always_inline)) inline

struct PrioStep {
    uint32_t level;                                  // s_setprio operand, 0..3
    uint32_t next;                                   // first p' > p with another level, or kPrioNever
};

// log2 of the chunk length for a launch of T hops (loop-invariant: kept beside T)
PRIO_INLINE constexpr uint32_t prio_ladder_shift(uint32_t T) {
    const uint32_t n = T / kPrioChunks;              // (a power of two: a shift)
    return n ? 31u - (uint32_t)__builtin_clz(n) : 31u;
}

// a boundary as an event loop counts it that started after `base` of the launch's hops (the
// second loop after an episode end inside a launch): loop-local, and still "never" when it is
PRIO_INLINE constexpr uint32_t prio_ladder_local(uint32_t next, uint32_t base) {
    return next == kPrioNever ? next : next - base;
}

// level and next boundary after p of T hops (p < T), shift = prio_ladder_shift(T)
PRIO_INLINE constexpr PrioStep prio_ladder(uint32_t T, uint32_t shift, uint32_t p) {
    const uint32_t t1 = T / 2 + T / 8, t2 = T - T / 8 - T / 16, t3 = T - T / 16;    // t1 <= t2 <= t3
    if (kPrioFrom >= 1u && p < t1) return PrioStep{3u, t1};
    if (kPrioFrom >= 2u && p < t2) return PrioStep{2u, t2};
    if (kPrioFrom >= 3u && p < t3) return PrioStep{1u, t3};
    if (kPrioFrom >= 4u) return PrioStep{0u, kPrioNever};
    const uint32_t from = kPrioFrom == 0u ? 0u : kPrioFrom == 1u ? t1 : kPrioFrom == 2u ? t2 : t3;
    const uint32_t q = p - from, len = 1u << shift;
    const uint32_t left = len - (q & (len - 1u));    // hops to the chunk's end, 1..len
    const uint32_t level = (3u - kPrioFrom - (q >> shift)) & 3u;
    // (the comparison, not p + left < T: the sum can pass 2^32)
    return PrioStep{level, (p < T && left <= T - 1u - p) ? p + left : kPrioNever};
}
