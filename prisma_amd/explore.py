"""The epsilon-greedy draw rule of the fused rollouts (include/prisma.h prisma_run_explore),
restated on the host for callers and tests.

For the data decision with log index ``d`` (the numbering of the records' ``prev``, which carries
over episode ends), in episode ``e``, at node ``v`` of overlay degree ``deg``, with policy action
``g``, in the replica with global id ``gid = replica_base + r``:

    c = philox4x32_10(ctr = {d, 0, e, 2}, key = {seed & 0xffffffff, gid})
    a = ((c[0] >> 8) < thr[v]) ? (uint32)(((uint64)c[1] * deg) >> 32) : g
    thr[v] = floor(eps[v] * 2^24 + 0.5) clamped to [0, 2^24]

Integer only: thr = 0 never explores, thr = 2^24 always does, and the pick is uniform over the
node's valid actions.  Counter word 3 = 2 is the exploration domain (0: flow start offsets,
1: send delays).  numpy only; everything is vectorised over its arguments.

History-weighted ("smart") exploration (include/prisma.h prisma_run_explore_smart; the
reference's --smart_exploration) keeps the draw and the hit test and replaces the uniform pick:
with ``h_i`` the count of action ``i`` in the deciding node's row of the caller's per-replica
action history (uint32, ``h = hist[r][row[v] : row[v] + deg]``),

    nb = sum h_i;  w_i = nb - h_i;  W = (deg - 1) * nb
    pick = W == 0 ? (uint32)(((uint64)c[1] * deg) >> 32)
                  : min { i : w_0 + ... + w_i > u },  u = ((c[1] << 32 | c[2]) * W) >> 64
    a = hit ? pick : g;  then, if 0 <= a < deg:  h_a += 1

so action ``i`` is picked with probability ``w_i / W = (1 - h_i / nb) / (deg - 1)``, and every
data decision -- explored or greedy, thr = 0 included -- counts its action when it is valid.
``smart_pick`` and ``smart_explore_action`` restate it in exact integers: 64-bit sums, the
128-bit product in 32-bit limbs.
"""
from __future__ import annotations

import numpy as np

EXPLORE_DOMAIN = 2
THR_ONE = 1 << 24

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11) over arrays: ctr [..., 4], key [..., 2] (broadcast
    against each other) -> uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64) & _MASK
    key = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0 = np.uint64(_M0) * c0                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(_M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _MASK, n2, p0 & _MASK
        k0 = (k0 + np.uint64(_W0)) & _MASK
        k1 = (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def thresholds(eps) -> np.ndarray:
    """Epsilons (scalar or array) -> uint32 thresholds: floor(eps * 2^24 + 0.5) in [0, 2^24]."""
    e = np.nan_to_num(np.asarray(eps, dtype=np.float64), nan=0.0)
    return np.clip(np.floor(e * float(THR_ONE) + 0.5), 0.0, float(THR_ONE)).astype(np.uint32)


def explore_draw(seed, gid, d, episode) -> np.ndarray:
    """The decision's Philox words c [..., 4]."""
    d, episode, gid = np.broadcast_arrays(np.asarray(d, dtype=np.uint64), np.asarray(episode, dtype=np.uint64),
                                          np.asarray(gid, dtype=np.uint64))
    ctr = np.stack([d, np.zeros_like(d), episode, np.full_like(d, EXPLORE_DOMAIN)], axis=-1)
    key = np.stack([np.full_like(d, int(seed) & _MASK), gid], axis=-1)
    return philox4x32_10(ctr, key)


def explore_action(seed, gid, d, episode, thr_v, deg, greedy):
    """The action the exploring kernels take: ``greedy`` unless the draw falls below ``thr_v``
    (the deciding node's threshold), then a uniform pick in [0, deg).  Scalars give an int,
    arrays an int64 array."""
    c = explore_draw(seed, gid, d, episode).astype(np.uint64)
    pick = (c[..., 1] * np.asarray(deg, dtype=np.uint64)) >> np.uint64(32)
    hit = (c[..., 0] >> np.uint64(8)) < np.asarray(thr_v, dtype=np.uint64)
    a = np.where(hit, pick.astype(np.int64), np.asarray(greedy, dtype=np.int64))
    return int(a) if a.ndim == 0 else a


def _mulhi64(x, W) -> np.ndarray:
    """floor(x * W / 2^64) for uint64 arrays x and W < 2^38, in 32-bit limbs: no step overflows uint64
    (x1 * w0 <= (2^32 - 1)^2 leaves room for a 32-bit carry; w1 < 2^6)."""
    m, s = np.uint64(_MASK), np.uint64(32)
    x, W = np.asarray(x, dtype=np.uint64), np.asarray(W, dtype=np.uint64)
    x0, x1, w0, w1 = x & m, x >> s, W & m, W >> s
    mid = x1 * w0 + ((x0 * w0) >> s)
    mid2 = x0 * w1 + (mid & m)
    return x1 * w1 + (mid >> s) + (mid2 >> s)


def smart_pick(c, h):
    """The history-weighted pick of an exploring decision.  c: the decision's Philox words
    [..., 4]; h: the node's row of counts [..., deg] (uint32 values; one degree per call).
    Scalars (c [4], h [deg]) give an int, batches an int64 array."""
    c = np.asarray(c, dtype=np.uint64)
    h = np.asarray(h, dtype=np.uint64)
    deg = h.shape[-1]
    nb = h.sum(axis=-1, dtype=np.uint64)              # <= 55 * 2^32
    W = np.uint64(deg - 1) * nb
    uniform = (c[..., 1] * np.uint64(deg)) >> np.uint64(32)
    u = _mulhi64((c[..., 1] << np.uint64(32)) | c[..., 2], W)
    prefix = np.cumsum(nb[..., None] - h, axis=-1, dtype=np.uint64)
    weighted = (prefix <= u[..., None]).sum(axis=-1)  # the first i with prefix_i > u (prefix is non-decreasing)
    a = np.where(W == 0, uniform, weighted.astype(np.uint64)).astype(np.int64)
    return int(a) if a.ndim == 0 else a


def smart_explore_action(seed, gid, d, episode, thr_v, h, greedy):
    """The action the smart-exploring kernels take at a node whose row of counts is ``h``
    (before the decision): ``greedy`` unless the draw falls below ``thr_v``, then ``smart_pick``.
    The caller then counts the action: ``h[a] += 1`` if ``0 <= a < deg``.  Scalars give an int."""
    c = explore_draw(seed, gid, d, episode)
    hit = (c[..., 0].astype(np.uint64) >> np.uint64(8)) < np.asarray(thr_v, dtype=np.uint64)
    a = np.where(hit, smart_pick(c, h), np.asarray(greedy, dtype=np.int64))
    return int(a) if a.ndim == 0 else a
