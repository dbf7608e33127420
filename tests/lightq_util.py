"""Host restatement of the DQN-buffer family's fixed operation order for any widths (B, H, NH)
(DESIGN.md §2, §5c), the comparator of the reduced models' tests: the oracle restates the 64-wide
model only.

fp32 throughout.  LayerNorm: sequential fp32 sums in k order, population variance,
sqrt(var + 1e-3f), IEEE divisions.  One-hot row plus bias.  Every dense unit is one fmaf chain over
its inputs in input order starting at +0 (the concat: one-hot branch first, then the buffers
branch), the bias added last with a plain add; ELU is x > 0 ? x : det_expm1f(x) through the oracle
library's or_det_expm1f; the action is the first-minimum argmin over the node's deg outputs.

The multiply-add is an exactly rounded fmaf emulated in float64 (``fmaf32``): the product of two
floats is exact in float64, the sum is rounded to odd, and the cast to float32 then rounds once.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from prisma_amd import explore

# (B, H, NH) per kind, restated here from models.py:39-306 (the comparator keeps its own table)
DIMS = {"buffer": (32, 64, 2), "buffer_lite": (16, 32, 2), "buffer_lighter": (16, 32, 1),
        "buffer_lighter_2": (8, 16, 1), "buffer_lighter_3": (4, 8, 1)}

_HALF = np.int64(0x10000000)           # a float64 whose low 29 mantissa bits are this lies half-way
_LOW29 = np.int64(0x1FFFFFFF)          # between two normal floats
_TINY = 2.0 ** -120                    # below it fp32 results approach the subnormals: slow path
_MAG = np.int64(0x7FFFFFFFFFFFFFFF)
_TINY_BITS_1 = np.uint64(np.float64(_TINY).view(np.int64) - 1)


def _add_round_to_odd(p, c):
    """p + c in float64 rounded to odd (TwoSum for the error; an inexact sum with an even last
    mantissa bit moves one ulp towards the exact value)."""
    s = p + c
    with np.errstate(invalid="ignore", over="ignore"):
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
    if np.any(fix):
        # towards the exact value p + c = s + e
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s


def fmaf32(a, b, c):
    """fmaf(a, b, c) of float32 arrays (broadcast), exactly rounded: float32 result."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    b64 = np.asarray(b, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return _add_round_to_odd(a64 * b64, np.broadcast_to(c64, np.broadcast(a64 * b64, c64).shape).copy()
                                 ).astype(np.float32)


def _fma_step(h64, w64, acc64):
    """One step of a chain on float64 arrays that hold float32 values: float32(h * w + acc) back as
    float64.  The plain float64 sum is right unless it lands half-way between two floats (or near
    the subnormals), where the round-to-odd sum decides."""
    p = h64 * w64
    s = p + acc64
    bits = s.view(np.int64)
    # (0 < |s| < _TINY as one unsigned compare of the magnitude bits less one: zero wraps around)
    tiny = ((bits & _MAG) - 1).view(np.uint64) < _TINY_BITS_1
    if (((bits & _LOW29) == _HALF) | tiny).any():
        s = _add_round_to_odd(p, np.broadcast_to(acc64, p.shape).copy())
    return s.astype(np.float32).astype(np.float64)


def _fma_chain(h64, W64):
    """The fmaf chains of a dense layer before its bias: h64 [n, in] and W64 [in, out] (float64
    arrays that hold float32 values) -> [n, out], every unit's chain in input order from +0, each
    link as _fma_step.  The plain float64 sums of the whole chain first, tested for _fma_step's
    doubtful cases all at once afterwards: a chain without one is what _fma_step gives link by link
    (up to the first doubtful link both see the same sums), any other is redone link by link."""
    if h64.shape[0] > 256:                                 # (bounds the [n, in, out] temporaries)
        return np.concatenate([_fma_chain(h64[k:k + 256], W64) for k in range(0, h64.shape[0], 256)])
    prod = h64[:, :, None] * W64[None, :, :]               # exact: 24 + 24 mantissa bits
    sums = np.empty_like(prod)
    acc = np.zeros((h64.shape[0], W64.shape[1]), dtype=np.float64)
    for i in range(W64.shape[0]):
        s = sums[:, i]
        np.add(prod[:, i], acc, out=s)
        acc = s.astype(np.float32).astype(np.float64)
    bits = sums.view(np.int64)
    tiny = ((bits & _MAG) - 1).view(np.uint64) < _TINY_BITS_1
    if not (((bits & _LOW29) == _HALF) | tiny).any():
        return acc
    acc = np.zeros((h64.shape[0], W64.shape[1]), dtype=np.float64)
    for i in range(W64.shape[0]):
        acc = _fma_step(h64[:, i:i + 1], W64[i][None, :], acc)
    return acc


def random_obs(topo, v, n, rng):
    """n observations at node v: uniform buffer values, with all-equal rows, zero rows and rows at
    the largest buffer value mixed in."""
    deg = int(topo.degrees[v])
    obs = np.zeros((n, topo.obs_width), dtype=np.uint32)
    obs[:, 0] = rng.integers(0, topo.n_overlay, n)
    obs[:, 1:1 + deg] = rng.integers(0, 16261, (n, deg))
    obs[0::7, 1:1 + deg] = obs[0::7, 1:2]                  # all equal
    obs[1::11, 1:1 + deg] = 0                              # zeros
    obs[2::13, 1:1 + deg] = 16260
    return obs


class HostMLP:
    """The restatement for one topology and one kind; `checker` of parity_util.check_near_ties."""

    def __init__(self, oracle_mod, topo, kind):
        self.B, self.H, self.NH = DIMS[kind]
        self.kind = kind
        self.N, self.D = topo.n_nodes, topo.max_deg
        self.deg = topo.degrees.astype(np.int64)
        self._expm1f = oracle_mod.lib().or_det_expm1f
        self._cache = (None, None)

    # -- packed layout ------------------------------------------------------
    def offsets(self):
        """{name: (offset, shape)} of the packed layout (StackedQNet.pack())."""
        N, D, B, H = self.N, self.D, self.B, self.H
        shapes = [("W1", (N, N, B)), ("b1", (N, B)), ("Wb", (N, D, B)), ("bb", (N, B)), ("W2", (N, 2 * B, H)),
                  ("b2", (N, H))]
        if self.NH == 2:
            shapes += [("W3", (N, H, H)), ("b3", (N, H))]
        shapes += [("W4", (N, H, D)), ("b4", (N, D))]
        out, o = {}, 0
        for name, shp in shapes:
            out[name] = (o, shp)
            o += int(np.prod(shp))
        out["_total"] = (o, ())
        return out

    def _split(self, weights):
        w = np.asarray(weights)
        key = (w.__array_interface__["data"][0], w.size)
        if self._cache[0] != key or not np.array_equal(self._cache[1]["_raw"], w):
            w32 = np.ascontiguousarray(w, dtype=np.float32).copy()
            offs = self.offsets()
            assert w32.size == offs["_total"][0], (w32.size, offs["_total"][0])
            parts = {"_raw": w32}
            for name, (o, shp) in offs.items():
                if name != "_total":
                    parts[name] = w32[o:o + int(np.prod(shp))].reshape(shp).astype(np.float64)
            self._cache = (key, parts)
        return self._cache[1]

    def _elu(self, x64):
        """ELU on float64-held floats, the negative branch through or_det_expm1f."""
        out = x64.copy()
        flat = out.reshape(-1)
        for i in np.nonzero(~(flat > 0))[0]:
            flat[i] = float(self._expm1f(C.c_float(flat[i])))
        return out

    def _dense(self, h64, W64, b64):
        """h64 [n, in], W64 [in, out], b64 [out]: the fmaf chains in input order, bias last, ELU."""
        return self._elu((_fma_chain(h64, W64).astype(np.float32) + b64.astype(np.float32)[None, :]).astype(np.float64))

    def _q_node(self, P, v, obs):
        """Q [n, deg] of n observations (uint32 [n, >= 1 + deg]) at node v."""
        deg = int(self.deg[v])
        f32 = np.float32
        dst = obs[:, 0].astype(np.int64)
        x = obs[:, 1:1 + deg].astype(f32)
        s = np.zeros(len(obs), dtype=f32)
        for k in range(deg):
            s = s + x[:, k]
        mean = s / f32(deg)
        d = x - mean[:, None]
        var = np.zeros(len(obs), dtype=f32)
        for k in range(deg):
            var = var + d[:, k] * d[:, k]
        var = var / f32(deg)
        den = np.sqrt(var + f32(1e-3))
        xn = (d / den[:, None]).astype(np.float64)
        h1 = self._elu((P["W1"][v][dst].astype(f32) + P["b1"][v].astype(f32)[None, :]).astype(np.float64))
        hb = self._dense(xn, P["Wb"][v][:deg], P["bb"][v])
        h = self._dense(np.concatenate([h1, hb], axis=1), P["W2"][v], P["b2"][v])
        if self.NH == 2:
            h = self._dense(h, P["W3"][v], P["b3"][v])
        return self._dense(h, P["W4"][v][:, :deg], P["b4"][v][:deg]).astype(f32)

    # -- the oracle's interface ----------------------------------------------
    def mlp_q(self, weights, node, obs):
        o = np.asarray(obs).astype(np.uint32).reshape(1, -1)
        return self._q_node(self._split(weights), int(node), o)[0]

    def mlp_action(self, weights, node, obs) -> int:
        return first_argmin(self.mlp_q(weights, node, obs))

    def mlp_q_batch(self, weights, nodes, obs):
        """(Q [n, max_deg] with +inf past each node's degree, actions [n]), as OracleSim.mlp_q_batch."""
        P = self._split(weights)
        nodes = np.asarray(nodes).astype(np.int64)
        obs = np.asarray(obs).astype(np.uint32)
        q = np.full((len(nodes), max(self.D, 1)), np.inf, dtype=np.float32)
        a = np.zeros(len(nodes), dtype=np.int32)
        for v in np.unique(nodes):
            rows = np.nonzero(nodes == v)[0]
            qv = self._q_node(P, int(v), obs[rows])
            q[rows, :qv.shape[1]] = qv
            a[rows] = [first_argmin(r) for r in qv]
        return q, a


def first_argmin(q) -> int:
    """best = 0; for a in 1..n-1: if q[a] < q[best]: best = a (tf.argmin, learner.py:145)."""
    best = 0
    for i in range(1, len(q)):
        if q[i] < q[best]:
            best = i
    return best


class HostStepped:
    """One CPU oracle per replica, stepped decision by decision (OracleSim.step) with the host
    restatement's action, optionally through the epsilon-greedy rule (thr: uint32 [N] thresholds by
    underlay id, prisma_amd.explore).  `weights` is read at every decision, so a caller may swap
    it between launches.  base: global log index of this episode's first record."""

    def __init__(self, oracle_mod, topo, params, replica, host: HostMLP, weights, thr=None, episode=0, base=0):
        self.O, self.topo, self.params, self.host = oracle_mod, topo, params, host
        self.weights = weights
        self.gid, self.episode, self.base = int(replica), int(episode), int(base)
        self.thr = None if thr is None else np.asarray(thr, dtype=np.uint32)
        self.o = oracle_mod.OracleSim(topo, params, replica=replica, episode=episode)
        self.explored = self.changed = self.hops = 0
        self.explored_at = []                              # record indices (this episode's) of the explored decisions
        self._c = np.zeros((0, 4), dtype=np.uint32)
        self.obs = None                                    # the pending decision's observation, if any
        self._over = False

    def n_records(self) -> int:
        return int(self.O.lib().or_record_count(self.o.h))

    def _draw(self, k):
        if k >= len(self._c):
            n = max(4096, 2 * (k + 1))
            self._c = explore.explore_draw(self.params["seed"], self.gid, self.base + np.arange(n), self.episode)
        return self._c[k]

    def to_decision(self) -> bool:
        """Run to the next decision and leave it pending (prisma_step without actions); False once
        the episode is over."""
        if self.obs is None and not self._over:
            self.obs = self.o.step(-1)
            self._over = self.obs is None
        return not self._over

    def step(self) -> bool:
        """One hop: run to the next decision (unless one is pending) and apply the rule's action.
        The oracle stops right after applying it, where a fused launch that ran out of hops
        stops: the action goes in as a one-entry table run of one hop."""
        if not self.to_decision():
            return False
        v = self.o.pending_node()
        a = g = self.host.mlp_action(self.weights, v, self.obs)
        if self.thr is not None:
            c = self._draw(self.n_records() - 1)
            if (int(c[0]) >> 8) < int(self.thr[v]):
                a = (int(c[1]) * int(self.topo.degrees[v])) >> 32
                self.explored += 1
                self.explored_at.append(self.n_records() - 1)
                self.changed += int(a != g)
        self.hops += 1
        assert self.o.run_table(np.full((self.topo.n_nodes, self.topo.n_nodes), a, dtype=np.uint8), 1) == 1
        self.obs = None
        return True

    def advance(self, hops) -> int:
        """Up to `hops` more hops (fewer when the episode ends); the hops executed."""
        n = 0
        while n < hops and self.step():
            n += 1
        return n

    def over(self) -> bool:
        return self._over

    def records(self, first=0, count=None):
        r = self.o.records(first, count).copy()
        r["prev"] = np.where(r["prev"] >= 0, r["prev"] + self.base, r["prev"])
        return r

    def counters(self):
        return self.o.counters()

    def close(self):
        self.o.close()


def random_weights(net, seed, scale=1.0):
    """Overwrite every parameter of a StackedQNet in place with fresh uniform draws inside the
    rows / columns a node uses (padding stays zero): another policy of the same shape."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.where(p != 0, (torch.rand(p.shape, generator=g) * 2 - 1) * scale, p))
    return net
