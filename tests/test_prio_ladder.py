"""The issue-priority ladder's arithmetic (prisma_amd/csrc/prio_ladder.h, called by engine_core.h
prio_update): a small g++ program includes the real header and checks, for every launch size T in
1 .. 5000 and 8191, 8192, 8193, 32768, 2^31 - 1, 2^32 - 1 and every progress p in [0, T) (strided
above 2^16), that

  * the level is in 0 .. 3 and the next boundary is > p or the "never" value;
  * walking boundary to boundary from 0 visits the same levels (and boundaries) as evaluating
    each p directly, so a loop that steps over a boundary lands on the level of its progress;
  * for a split base + local = p (an event loop that starts after `base` hops of the launch) the
    loop-local boundary is next - base and > local: every split for T <= 600; above that the
    bases 0, 1, p / 3, p / 2, p - 1 and p for every p, and every base for every 97th p (every
    split of every p would be T^3 / 6 checks per T, 2e10 at T = 5000; the local boundary is
    next - base, so with next > p it holds for every base once it holds for one);
  * the chunk shift is below 32 and the chunk is never empty;

for the shipped defaults and for every point of the sweep (profiles/prio_ladder/ab_sweep.txt:
cyclic 32 .. 256 chunks, hybrid from 5/8 and 13/16 with T/64 and T/128 chunks, the fixed thresholds
alone).  With the shipped defaults at T = 32768, no run of hops at one level in the launch's last
quarter is longer than the chunk."""
import os
import subprocess
import tempfile

import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "prisma_amd", "csrc")

CXX_SRC = r'''
#include <stdio.h>
#include <stdint.h>
#include "prio_ladder.h"

static long bad = 0;
static unsigned long long n = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 5) fprintf(stderr, "line %d: T %u p %u\n", __LINE__, T, p); } } while (0)

static void check_split(uint32_t T, uint32_t p, uint32_t next, uint32_t base) {
    const uint32_t local = p - base, ln = prio_ladder_local(next, base);
    if (next == kPrioNever) CHECK(ln == kPrioNever);
    else CHECK(ln == next - base && ln > local);
}

static void check_T(uint32_t T) {
    const uint32_t shift = prio_ladder_shift(T);
    uint32_t p = 0;
    CHECK(shift < 32u && (1u << shift) >= 1u);
    CHECK(T < kPrioChunks ? shift == 31u : ((1u << shift) <= T / kPrioChunks && T / kPrioChunks < (2ull << shift)));
    const uint32_t stride = T > 65536u ? T / 60000u | 1u : 1u;
    /* the walk: [lo, nx) is the stretch of one level that holds p */
    PrioStep w = prio_ladder(T, shift, 0);
    uint32_t lo = 0;
    unsigned steps = 0;
    for (uint64_t pp = 0; pp < T; pp += stride) {
        p = (uint32_t)pp;
        while (w.next != kPrioNever && p >= w.next) {
            lo = w.next;
            w = prio_ladder(T, shift, lo);
            CHECK(w.next > lo);
            if (++steps > 4u * kPrioChunks + 8u) { CHECK(0); return; }
        }
        const PrioStep d = prio_ladder(T, shift, p);
        n++;
        CHECK(d.level <= 3u);
        CHECK(d.next == kPrioNever || d.next > p);
        CHECK(d.level == w.level && d.next == w.next);
        check_split(T, p, d.next, 0u); check_split(T, p, d.next, p);
        check_split(T, p, d.next, p / 3u); check_split(T, p, d.next, p / 2u);
        if (p) { check_split(T, p, d.next, 1u); check_split(T, p, d.next, p - 1u); }
        if (T <= 600u || (pp / stride) % 97u == 0u) {
            const uint32_t bs = p > 5000u ? p / 5000u : 1u;
            for (uint64_t b = 0; b <= p; b += bs) check_split(T, p, d.next, (uint32_t)b);
        }
    }
}

int main(void) {
    for (uint32_t T = 1; T <= 5000u; ++T) check_T(T);
    const uint32_t more[] = {8191u, 8192u, 8193u, 32768u, 0x7fffffffu, 0xffffffffu};
    for (unsigned i = 0; i < sizeof(more) / sizeof(more[0]); ++i) check_T(more[i]);
    /* the longest run of hops at one level in the last quarter of a 32768-hop launch */
    const uint32_t T = 32768u, shift = prio_ladder_shift(T);
    uint32_t run = 0, longest = 0, prev = 4u;
    for (uint32_t p = T - T / 4u; p < T; ++p) {
        const uint32_t l = prio_ladder(T, shift, p).level;
        run = l == prev ? run + 1u : 1u;
        prev = l;
        if (run > longest) longest = run;
    }
    printf("%llu %ld %u %u %u %u\n", n, bad, kPrioChunks, kPrioFrom, 1u << shift, longest);
    return 0;
}
'''

SWEEP = [(c, 0) for c in (32, 64, 128, 256)] + [(c, k) for k in (1, 2) for c in (64, 128)] + [(64, 4), (4, 0), (1024, 3)]


def _run(flags):
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ladder.cc"), os.path.join(d, "ladder")
        open(src, "w").write(CXX_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", HEADER_DIR, *flags, "-o", exe, src])
        return [int(x) for x in subprocess.check_output([exe], text=True).split()]


def test_shipped_ladder():
    n, bad, chunks, k, chunk, longest = _run([])
    print(f"shipped: PRISMA_PRIO_CHUNKS {chunks}, PRISMA_PRIO_HYBRID_FROM {k}; T 32768: chunk {chunk} hops, "
          f"longest one-level run in the last quarter {longest}")
    assert n > 1.2e7 and bad == 0
    assert chunk == 32768 // chunks
    assert longest <= chunk


@pytest.mark.parametrize("chunks,k", SWEEP)
def test_sweep_points(chunks, k):
    n, bad, c, kk, chunk, _ = _run([f"-DPRISMA_PRIO_CHUNKS={chunks}", f"-DPRISMA_PRIO_HYBRID_FROM={k}"])
    assert (c, kk) == (chunks, k) and chunk == 32768 // chunks
    assert n > 1.2e7 and bad == 0
