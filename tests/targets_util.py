"""Host restatement of prisma_replay_targets' rule (include/prisma.h), the comparator of
tests/test_replay_targets.py and tests/test_gpu_replay_targets.py.

The Q values come from lightq_util.HostMLP for the DQN-buffer kinds; the routing model is the same
operation order with the one-hot branch alone feeding layer 2 (HostRouting below: HostMLP's dense
layers, i.e. lightq_util._fma_chain and the oracle's or_det_expm1f, over the routing layout).  The
rule itself -- slot, gather, not evaluable, done, the filtered first-listed minimum in which a NaN
never wins, fadd_rn(rew, fmul_rn(gamma, best)) -- is restated in plain numpy float32 operations.
"""
from __future__ import annotations

import numpy as np

from lightq_util import DIMS, HostMLP

STATUS_EVAL, STATUS_DONE, STATUS_NOT_EVALUABLE = 0, 1, 2


class HostRouting(HostMLP):
    """DQN_routing_model in the DQN-buffer family's fixed order: one_hot row + bias, then every
    dense unit one fmaf chain in input order from +0, bias last, ELU on every layer."""

    def __init__(self, oracle_mod, topo):
        HostMLP.__init__(self, oracle_mod, topo, "buffer")
        self.kind = "routing"

    def offsets(self):
        N, D = self.N, self.D
        shapes = [("W1", (N, N, 32)), ("b1", (N, 32)), ("W2", (N, 32, 64)), ("b2", (N, 64)), ("W3", (N, 64, 64)),
                  ("b3", (N, 64)), ("W4", (N, 64, D)), ("b4", (N, D))]
        out, o = {}, 0
        for name, shp in shapes:
            out[name] = (o, shp)
            o += int(np.prod(shp))
        out["_total"] = (o, ())
        return out

    def _q_node(self, P, v, obs):
        deg = int(self.deg[v])
        f32 = np.float32
        dst = obs[:, 0].astype(np.int64)
        h = self._elu((P["W1"][v][dst].astype(f32) + P["b1"][v].astype(f32)[None, :]).astype(np.float64))
        h = self._dense(h, P["W2"][v], P["b2"][v])
        h = self._dense(h, P["W3"][v], P["b3"][v])
        return self._dense(h, P["W4"][v][:, :deg], P["b4"][v][:deg]).astype(f32)


def host_model(oracle_mod, topo, kind):
    return HostRouting(oracle_mod, topo) if kind == "routing" else HostMLP(oracle_mod, topo, kind)


def topology_tables(topo):
    """(row [N + 1], nxt [T], back [T]): the action-history layout, the next node of every (u, a) and
    the next node's action leading back to u (-1: none)."""
    N = topo.n_nodes
    row = np.concatenate([[0], np.cumsum(topo.degrees.astype(np.int64))]).astype(np.int64)
    nxt = np.zeros(int(row[-1]), dtype=np.int64)
    back = np.full(int(row[-1]), -1, dtype=np.int64)
    for u in range(N):
        for a, v in enumerate(topo.neighbors(u)):
            nv = list(topo.neighbors(v))
            nxt[row[u] + a] = v
            back[row[u] + a] = nv.index(u) if u in nv else -1
    return row, nxt, back


def filtered_min(q, bk):
    """best = +inf; for j: if j != bk and q[j] < best: best = q[j] (a NaN never wins)."""
    best = np.float32(np.inf)
    for j in range(len(q)):
        if j != bk and q[j] < best:
            best = q[j]
    return np.float32(best)


def host_targets(host, topo, rings, idx, weights, gamma, n_replicas, gen_of=None):
    """The rule for rings (dict of numpy arrays obs / next_obs [N, size, W], action, reward, done,
    replica [N, size]), idx int64 [N, batch], weights a list of packed float32 arrays, gen_of int32
    [R, T] or None.  Returns dict(obs, action, target, status) with row i = u * batch + b."""
    N, size, W = rings["obs"].shape
    idx = np.asarray(idx, dtype=np.int64)
    batch = idx.shape[1]
    row, nxt, back = topology_tables(topo)
    deg = topo.degrees.astype(np.int64)
    rows = N * batch
    out = {"obs": np.zeros((rows, W), dtype=np.int32), "action": np.zeros(rows, dtype=np.int64),
           "target": np.zeros(rows, dtype=np.float32), "status": np.zeros(rows, dtype=np.uint8)}
    gamma32 = np.float32(gamma)
    todo = {}                                              # (generation, next node) -> [(row, back action)]
    for u in range(N):
        for b in range(batch):
            i, s = u * batch + b, int(idx[u, b])
            if s < 0 or s >= size:
                out["status"][i] = STATUS_NOT_EVALUABLE    # zeros, action 0, target +0
                continue
            a, rew = int(rings["action"][u, s]), np.float32(rings["reward"][u, s])
            done, r = bool(rings["done"][u, s]), int(rings["replica"][u, s])
            out["obs"][i] = rings["obs"][u, s]
            out["action"][i] = a
            out["target"][i] = rew
            g = -1
            if 0 <= a < deg[u] and 0 <= r < n_replicas:
                g = 0 if gen_of is None else int(gen_of[r, row[u] + a])
            dst = int(np.uint32(rings["next_obs"][u, s, 0]))
            if g < 0 or g >= len(weights) or (not done and dst >= N):
                out["status"][i] = STATUS_NOT_EVALUABLE
            elif done:
                out["status"][i] = STATUS_DONE
            else:
                out["status"][i] = STATUS_EVAL
                t = int(row[u] + a)
                todo.setdefault((g, int(nxt[t])), []).append((i, int(back[t]), u, s))
    with np.errstate(invalid="ignore", over="ignore"):
        for (g, v) in sorted(todo):
            items = todo[(g, v)]
            nobs = np.stack([rings["next_obs"][u, s] for _, _, u, s in items]).astype(np.uint32)
            q = host._q_node(host._split(weights[g]), v, nobs)          # [n, deg(v)] float32
            for (i, bk, _, _), qi in zip(items, q):
                best = filtered_min(qi, bk)
                out["target"][i] = np.float32(out["target"][i] + np.float32(gamma32 * best))
    return out


def kind_dims(kind):
    """(B, H, NH, buffers branch) of a kind."""
    return (32, 64, 2, False) if kind == "routing" else DIMS[kind] + (True,)


def constructed_rings(topo, size, n_replicas, seed):
    """Rings as numpy arrays in which every class of the rule is present by construction: for every
    (u, a < deg(u)) done and not-done items (size >= 2 * max_deg), next observations from
    lightq_util.random_obs at the next node (all-equal rows, zero rows and rows at 16 260 mixed in),
    random fp32 rewards everywhere (also in the rings of nodes without an agent, which otherwise
    stay empty: action 0, replica 0) and random replicas in [0, n_replicas)."""
    from lightq_util import random_obs
    assert size >= 2 * topo.max_deg
    rng = np.random.default_rng(seed)
    N, W = topo.n_nodes, topo.obs_width
    rings = {"obs": np.zeros((N, size, W), dtype=np.int32), "next_obs": np.zeros((N, size, W), dtype=np.int32),
             "action": np.zeros((N, size), dtype=np.int64),
             "reward": rng.uniform(0.001, 2.0, (N, size)).astype(np.float32),
             "done": np.zeros((N, size), dtype=bool), "replica": np.zeros((N, size), dtype=np.int64)}
    for u in range(N):
        deg = int(topo.degrees[u])
        if deg == 0:
            continue
        nb = topo.neighbors(u)
        rings["obs"][u] = random_obs(topo, u, size, rng).astype(np.int32)
        pools = [random_obs(topo, v, 14, rng).astype(np.int32) for v in nb]
        for s in range(size):
            a = s % deg
            rings["action"][u, s] = a
            rings["done"][u, s] = (s // deg) % 2 == 1
            rings["next_obs"][u, s] = pools[a][(s // deg) % 14]
        rings["replica"][u] = rng.integers(0, n_replicas, size)
    return rings


def gather_rows(rings, key, idx):
    """rings[key][u, idx[u, b]] as rows i = u * batch + b (torch.gather's result, in numpy)."""
    t = rings[key]
    sel = np.take_along_axis(t, idx.reshape(idx.shape + (1,) * (t.ndim - 2)), axis=1)
    return sel.reshape((-1,) + t.shape[2:])
