"""The device's constant divisions (prisma_amd/csrc/numerics.h div_const: q = a * RN(1/d), then one
FMA correction) equal IEEE division bit for bit for the kernels' operands: a = t ns < 2^42 over
d = 1e9 (ns_to_sec, ns-3's GetSeconds) and a = microseconds < 2^32 over d = 1e6 (the reward's
"%f" times, forwarder.py:360). The oracle divides; the kernels may not diverge from it by an ulp.

The device-only forms of the time code, restated on the host over the whole clock range of a
4095-s episode: div_1e3 and div_1e9 (floor(t * c) cast to 32 bits: right for t < 2^32 * 1000 ns,
not for the 2^42 the header's comment names), engine_core.h ping_send_s and py_micros with its
tie branch (__umul64hi as a 128-bit product) against the oracle's or_py_micros."""
import os
import subprocess
import tempfile

C_SRC = r'''
#include <stdio.h>
#include <stdint.h>
#include <math.h>
/* numerics.h div_const, device branch */
static double div_const(double a, double d, double rd) { double q = a * rd; double e = fma(-q, d, a); return fma(e, rd, q); }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main(void) {
    const double D[2] = {1e9, 1e6}, RD[2] = {1e-9, 1e-6};
    const int BITS[2] = {42, 32};
    long bad = 0, n = 0;
    for (int k = 0; k < 2; ++k) {
        for (int64_t t = 0; t < 4000000; ++t, ++n)                     /* every small operand */
            if (div_const((double)t, D[k], RD[k]) != (double)t / D[k]) bad++;
        for (long i = 0; i < 8000000; ++i) {
            const int sh = (int)(xr() % (uint64_t)BITS[k]) + 1;        /* every magnitude */
            const int64_t t = (int64_t)(xr() & ((1ull << sh) - 1));
            n++; if (div_const((double)t, D[k], RD[k]) != (double)t / D[k]) bad++;
            const int64_t m = (int64_t)(xr() % ((1ull << BITS[k]) / (uint64_t)D[k] + 1)) * (int64_t)D[k]
                              + (int64_t)(xr() % 2001) - 1000;          /* around multiples of d */
            if (m >= 0) { n++; if (div_const((double)m, D[k], RD[k]) != (double)m / D[k]) bad++; }
        }
    }
    printf("%ld %ld\n", n, bad);
    return 0;
}
'''


def test_device_constant_division_equals_ieee_division():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "div.c"), os.path.join(d, "div")
        open(src, "w").write(C_SRC)
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, src, "-lm"])
        n, bad = map(int, subprocess.check_output([exe], text=True).split())
    assert n > 3e7 and bad == 0


C_DEG = r'''
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
/* engine_core.h div_deg: a / d for the node degree d with rd = RN(1/d) */
static float div_deg(float a, float d, float rd) { float q = a * rd; float e = fmaf(-q, d, a); return fmaf(e, rd, q); }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main(void) {
    long bad = 0, n = 0;
    for (int d = 1; d <= 64; ++d) {
        const float fd = (float)d, rd = 1.0f / fd;
        for (uint32_t u = 0x3f800000u; u < 0x40000000u; u += 7u) {      /* the binade [1, 2) */
            float a; memcpy(&a, &u, 4); n++; if (div_deg(a, fd, rd) != a / fd) bad++;
        }
        for (int i = 0; i < 300000; ++i) {                              /* every exponent from 2^-120 */
            uint32_t u = 0x03800000u + (uint32_t)(xr() % (0x7f800000u - 0x03800000u));
            float a; memcpy(&a, &u, 4); n++; if (div_deg(a, fd, rd) != a / fd) bad++;
        }
        for (uint32_t k = 0; k < 400000; ++k) {                         /* integer sums (queued bytes) */
            const float a = (float)k; n++; if (div_deg(a, fd, rd) != a / fd) bad++;
        }
    }
    printf("%ld %ld\n", n, bad);
    return 0;
}
'''


def test_degree_division_equals_ieee_division():
    """engine_core.h div_deg (the memory-resident LayerNorm's mean and variance over the node degree):
    the Markstein correction with RN(1/d) equals IEEE float division for d = 1..64 on a sample here;
    scripts/checks/div_deg_exhaustive.c checks every float >= 2^-120 (0 mismatches)."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "deg.c"), os.path.join(d, "deg")
        open(src, "w").write(C_DEG)
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, src, "-lm"])
        n, bad = map(int, subprocess.check_output([exe], text=True).split())
    assert n > 1e8 and bad == 0


def _run_c(name, src, extra=()):
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, name + ".c"), os.path.join(d, name)
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, c, *extra, "-lm"])
        return [tuple(map(int, line.split())) for line in subprocess.check_output([exe], text=True).splitlines()]


C_FLOOR = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
/* numerics.h div_1e3 and div_1e9, device branches */
static uint64_t div_1e3(uint64_t t) { return (uint64_t)(uint32_t)floor((double)t * 0.001); }
static uint64_t div_1e9(uint64_t t) { return (uint64_t)(uint32_t)floor((double)t * 1e-9); }
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static long n = 0, bad = 0;
static void check(uint64_t t) {
    n++;
    if (div_1e3(t) != t / 1000u) bad++;
    if (div_1e9(t) != t / 1000000000u) bad++;
}
int main(void) {
    const uint64_t LIM = 1000ull << 32;                    /* t / 1000 fits 32 bits below it */
    const uint64_t D[2] = {1000ull, 1000000000ull};
    for (uint64_t t = 0; t < 4000000; ++t) check(t);        /* every small operand */
    for (long i = 0; i < 40000000; ++i) check(xr() % LIM);  /* the whole range */
    for (long i = 0; i < 4000000; ++i) {                    /* every magnitude */
        const int sh = (int)(xr() % 42u) + 1;
        const uint64_t t = xr() & ((1ull << sh) - 1);
        if (t < LIM) check(t);
    }
    for (int k = 0; k < 2; ++k)                             /* multiples of the divisor - 1, + 0, + 1 */
        for (long i = 0; i < 4000000; ++i) {
            const uint64_t m = (xr() % (LIM / D[k])) * D[k];
            if (m) check(m - 1);
            check(m);
            check(m + 1);
        }
    for (uint64_t q = 1; q <= 4096; ++q)                    /* every whole second of an episode */
        for (int64_t o = -2; o <= 2; ++o) check(q * D[1] + (uint64_t)o);
    {                                                       /* the last operands of a 4095-s episode */
        const uint64_t top = (uint64_t)(int64_t)(4095.0 * 1e9 + 0.5) + (1ull << 31);
        for (uint64_t t = top - 1000000; t < top; ++t) check(t);
        for (uint64_t t = LIM - 1000000; t < LIM; ++t) check(t);
    }
    printf("%ld %ld\n", n, bad);
    /* beyond the bound the 32-bit cast is wrong, well inside the 2^42 of the header's comment */
    printf("%d %d\n", div_1e3(LIM) == LIM / 1000u, LIM < (1ull << 42));
    return 0;
}
"""


def test_device_floor_divisions_equal_integer_division():
    """numerics.h div_1e3 / div_1e9, device form: (uint64_t)(uint32_t)floor((double)t * 0.001) and
    ... * 1e-9 equal t / 1000 and t / 10^9 for every t < 2^32 * 1000 = 4.29497e12 ns checked here --
    the operand bound the 32-bit cast sets (at 2^32 * 1000 itself, below the 2^42 of the header's
    comment, div_1e3 is wrong; sim_time_s <= 4095 keeps t 4.9 % inside)."""
    (n, bad), (right_at_bound, bound_below_2_42) = _run_c("floor", C_FLOOR)
    assert n > 7e7 and bad == 0
    assert not right_at_bound and bound_below_2_42


C_PING = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
/* engine_core.h ping_send_s's milliseconds: floor((k + 1) period / 10^6) on the vector unit */
static uint64_t send_ms(int64_t k, int64_t period) {
    return (uint64_t)floor((double)(k + 1) * (double)period * 0x1.0c6f7a0b5ed8ep-20);
}
int main(void) {
    const float IVAL[] = {0.01f, 0.05f, 0.2f, 1.0f, 5.0f, 7.0f, 30.0f, 50.0f, 100.0f, 1000.0f};
    const int64_t end = (int64_t)(4095.0 * 1e9 + 0.5);
    long n = 0, bad = 0;
    for (unsigned i = 0; i < sizeof IVAL / sizeof *IVAL; ++i) {
        const int64_t period = (int64_t)((double)IVAL[i] * 1e9 + 0.5);       /* numerics.h sec_to_ns of the C float */
        for (int64_t k = 0; (k + 1) * period <= end + period; ++k, ++n)      /* every round of the episode, and one */
            if (send_ms(k, period) != (uint64_t)((k + 1) * period) / 1000000u) bad++;
    }
    printf("%ld %ld\n", n, bad);
    return 0;
}
"""


def test_ping_send_time_equals_integer_division():
    """engine_core.h ping_send_s: floor((double)(k + 1) * (double)period_ns * RU(10^-6)) equals
    (k + 1) period_ns / 10^6 at every round of a 4095-s episode, at the ping intervals the suites
    use (0.01 s: 409 500 rounds; 1 s: k up to 4094)."""
    (n, bad), = _run_c("ping", C_PING)
    assert n > 409500 + 81900 + 20475 + 4095 and bad == 0


C_MICROS = r"""
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
uint64_t or_py_micros(int64_t t);                           /* the oracle's (oracle/prisma_oracle.c) */
/* numerics.h py_micros, device branches: div_1e3, ns_to_sec = div_const, __umul64hi */
static uint64_t div_1e3(uint64_t t) { return (uint64_t)(uint32_t)floor((double)t * 0.001); }
static double ns_to_sec(int64_t t) { double a = (double)t, q = a * 1e-9, e = fma(-q, 1e9, a); return fma(e, 1e-9, q); }
static uint64_t umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
static uint64_t py_micros(int64_t t) {
    uint64_t u = div_1e3((uint64_t)t);
    int64_t r = t - (int64_t)u * 1000;
    if (r != 500) return r < 500 ? u : u + 1;
    double x = ns_to_sec(t);
    uint64_t b; memcpy(&b, &x, 8);
    int ex = (int)((b >> 52) & 0x7ff);
    uint64_t mant = (b & 0x000fffffffffffffULL) | (ex ? 0x0010000000000000ULL : 0);
    if (!ex) ex = 1;
    int sh = 1075 - ex;
    const uint64_t k = 2000000ull;
    uint64_t lo = mant * k;
    uint64_t hi = umul64hi(mant, k);
    uint64_t v = 2 * u + 1, rhi, rlo;
    if (sh >= 64) { rhi = v << (sh - 64); rlo = 0; }
    else if (sh == 0) { rhi = 0; rlo = v; }
    else { rhi = v >> (64 - sh); rlo = v << sh; }
    if (hi != rhi) return hi > rhi ? u + 1 : u;
    if (lo != rlo) return lo > rlo ? u + 1 : u;
    return (u & 1) ? u + 1 : u;
}
static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main(void) {
    long n = 0, bad = 0, up = 0, other = 0, obad = 0;
    for (long i = 0; i < 2000000; ++i, ++n) {               /* ties across the whole episode */
        const int64_t t = (int64_t)(xr() % 4095000000ull) * 1000 + 500;
        const uint64_t g = py_micros(t);
        if (g != or_py_micros(t)) bad++;
        if (g == (uint64_t)(t / 1000) + 1) up++;
    }
    for (int64_t t = 500; t < 4000000; t += 1000, ++n)      /* every tie of the first 4 ms */
        if (py_micros(t) != or_py_micros(t)) bad++;
    for (int64_t sec = 4000; sec <= 4095; ++sec)            /* the ties within 1 ms of a late whole second */
        for (int64_t t = sec * 1000000000ll - 1000000 + 500; t < sec * 1000000000ll + 1000000; t += 1000, ++n)
            if (py_micros(t) != or_py_micros(t)) bad++;
    for (long i = 0; i < 4000000; ++i, ++other) {           /* off the tie: the device div_1e3 alone */
        const int64_t t = (int64_t)(xr() % 4095000000000ull);
        if (py_micros(t) != or_py_micros(t)) obad++;
    }
    printf("%ld %ld\n%ld %ld\n%ld %ld\n", n, bad, up, n - up, other, obad);
    return 0;
}
"""


def test_device_py_micros_equals_the_oracle():
    """numerics.h py_micros, device form, against the oracle's or_py_micros on 2e6 ties (t mod 1000 =
    500) across [0, 4095e9] ns, every tie of the first 4 ms and those within 1 ms of every whole
    second from 4000 s to 4095 s; both roundings of a tie occur.  Off the tie, 4e6 more."""
    import oracle as O
    lib = O.build()
    (n, bad), (up, down), (other, obad) = _run_c("micros", C_MICROS, [lib, "-Wl,-rpath," + os.path.dirname(lib)])
    assert n >= 2000000 + 4000 + 96 * 2000 and bad == 0
    assert up > n // 10 and down > n // 10
    assert other == 4000000 and obad == 0
