"""The comparator of the reduced DQN-buffer models' tests (tests/lightq_util.py) checked on its own:
the float64 emulation of fmaf against libm's, and the host restatement at the 64-wide model's
widths (32, 64, 2) bit for bit against the oracle's mlp_q / mlp_action -- which pins the order
conventions of the generic code to the existing oracle."""
import ctypes as C

import numpy as np
import pytest

from prisma_amd.config import engine_params
from prisma_amd.policies import StackedQNet
from prisma_amd.topology import Topology

import lightq_util as LQ


def _topo(name):
    return Topology.example(name, 0, 1.0)


# ---- 1. the fmaf emulation ---------------------------------------------------------------
def _libm_fmaf():
    f = C.CDLL("libm.so.6").fmaf
    f.restype = C.c_float
    f.argtypes = [C.c_float, C.c_float, C.c_float]
    return f


def test_fmaf_emulation_equals_libm():
    fmaf = _libm_fmaf()
    rng = np.random.default_rng(1)
    n = 10 ** 6
    # random bit patterns of moderate exponent (products and sums stay finite), both signs
    def draw():
        e = rng.integers(127 - 20, 127 + 20, n).astype(np.uint32)
        return ((rng.integers(0, 2, n).astype(np.uint32) << 31) | (e << 23)
                | rng.integers(0, 1 << 23, n).astype(np.uint32)).view(np.float32)
    a, b, c = draw(), draw(), draw()
    # a third of the addends cancel most of the product: the hard roundings
    k = n // 3
    c[:k] = -(a[:k].astype(np.float64) * b[:k].astype(np.float64)).astype(np.float32) * np.float32(1 + 2.0 ** -12)
    got = LQ.fmaf32(a, b, c)
    chain = LQ._fma_step(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)).astype(np.float32)
    # every triple through libm
    want = np.fromiter((fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())), dtype=np.float32, count=n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(chain.view(np.uint32), want.view(np.uint32))


def test_fmaf_emulation_half_way_cases():
    """a*b + c within one float64 ulp of an fp32 midpoint: a*b = m + d with m a midpoint of two
    floats near c's sum and |d| far below a float64 ulp of the result, both signs of d."""
    fmaf = _libm_fmaf()
    cases = []
    for e in (0, 5, -9):
        for sign in (1.0, -1.0):
            # c = 2^e (1 + j 2^-23); a*b = 2^(e-24) (1 - 2^-40) or (1 - 2^-30): half an ulp of c less
            # a sliver (2^-64 or 2^-54 of c) that a float64 sum of c and a*b cannot hold, or exactly half
            for j in (0, 1, 2, 12345, (1 << 23) - 1):
                cval = np.float32(2.0 ** e * (1 + j * 2.0 ** -23))
                for a, b in ((np.float32(2.0 ** -12 * (1 + 2.0 ** -20)), np.float32(2.0 ** (e - 12) * (1 - 2.0 ** -20))),
                             (np.float32(2.0 ** -12 * (1 + 2.0 ** -15)), np.float32(2.0 ** (e - 12) * (1 - 2.0 ** -15))),
                             (np.float32(2.0 ** -12), np.float32(2.0 ** (e - 12)))):
                    cases.append((np.float32(sign) * a, b, np.float32(sign) * cval))
                    cases.append((np.float32(-sign) * a, b, np.float32(sign) * cval))
    a, b, c = (np.array(x, dtype=np.float32) for x in zip(*cases))
    exact_near_mid = 0
    for x, y, z in cases:
        s = float(x) * float(y) + float(z)
        exact_near_mid += int((np.float64(s).view(np.int64) & 0x1FFFFFFF) in (0x10000000, 0x0FFFFFFF, 0x10000001))
    assert exact_near_mid >= len(cases) // 4           # the construction does hit the midpoints
    want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in cases], dtype=np.float32)
    assert np.array_equal(LQ.fmaf32(a, b, c).view(np.uint32), want.view(np.uint32))
    chain = LQ._fma_step(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)).astype(np.float32)
    assert np.array_equal(chain.view(np.uint32), want.view(np.uint32))
    # and the plain float64 evaluation gets some of them wrong: the cases do need the rounding to odd
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert np.any(plain.view(np.uint32) != want.view(np.uint32))


def test_fma_chain_equals_its_links():
    """A dense layer's chains (the plain float64 sums first, the doubtful links tested afterwards)
    against fmaf32 link by link: random layers, more rows than one chunk, and a layer whose second
    link lands on an fp32 midpoint, which only the rounding to odd gets right."""
    rng = np.random.default_rng(2)

    def links(h, W):
        acc = np.zeros((h.shape[0], W.shape[1]), dtype=np.float32)
        for i in range(W.shape[0]):
            acc = LQ.fmaf32(h[:, i:i + 1], W[i][None, :], acc)
        return acc

    for n, n_in, n_out in ((1, 40, 32), (7, 64, 64), (300, 9, 5)):
        h = rng.standard_normal((n, n_in)).astype(np.float32)
        W = rng.standard_normal((n_in, n_out)).astype(np.float32)
        got = LQ._fma_chain(h.astype(np.float64), W.astype(np.float64)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), links(h, W).view(np.uint32)), (n, n_in, n_out)
    # link 0 leaves c = 1 + 2^-23 in the accumulator; link 1 adds a b = 2^-24 (1 - 2^-40): half an ulp
    # of c less a sliver that a float64 sum cannot hold
    a, b = np.float32(2.0 ** -12 * (1 + 2.0 ** -20)), np.float32(2.0 ** -12 * (1 - 2.0 ** -20))
    h = np.array([[1.0, a, 0.5]], dtype=np.float32)
    W = np.array([[1 + 2.0 ** -23, 0.25], [b, b], [0.0, 1.0]], dtype=np.float32)
    plain = ((h[:, :1].astype(np.float64) * W[0] + 0.0).astype(np.float32).astype(np.float64)
             + h[:, 1:2].astype(np.float64) * W[1]).astype(np.float32)
    want = links(h[:, :2], W[:2])
    assert plain.view(np.uint32)[0, 0] != want.view(np.uint32)[0, 0]          # (the case does need it)
    got = LQ._fma_chain(h.astype(np.float64), W.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), links(h, W).view(np.uint32))


# ---- 2. the restatement at (32, 64, 2) is the oracle's ------------------------------------
@pytest.mark.parametrize("name", ["abilene", "geant"])
def test_restatement_equals_oracle_at_buffer_widths(oracle_mod, name):
    topo = _topo(name)
    params = engine_params(topo, sim_time_s=1.0)
    w = StackedQNet(topo, "buffer", seed=3, device="cpu").pack().numpy()
    host = LQ.HostMLP(oracle_mod, topo, "buffer")
    o = oracle_mod.OracleSim(topo, params)
    rng = np.random.default_rng(5)
    per = 4000 // int((topo.degrees > 0).sum()) + 1
    total = 0
    for v in np.nonzero(topo.degrees > 0)[0]:
        obs = LQ.random_obs(topo, int(v), per, rng)
        nodes = np.full(per, v, dtype=np.int32)
        qo, ao = o.mlp_q_batch(w, nodes, obs)
        qh, ah = host.mlp_q_batch(w, nodes, obs)
        assert np.array_equal(qo.view(np.uint32), qh.view(np.uint32)), (name, int(v))
        assert np.array_equal(ao, ah)
        assert host.mlp_action(w, int(v), obs[3]) == o.mlp_action(w, int(v), obs[3])
        assert np.array_equal(host.mlp_q(w, int(v), obs[4]).view(np.uint32), o.mlp_q(w, int(v), obs[4]).view(np.uint32))
        total += per
    assert total >= 4000
    o.close()
