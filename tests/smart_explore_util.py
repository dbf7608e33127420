"""The comparator of the smart-exploration tests: one CPU oracle per replica driven decision by
decision (OracleSim.step) under the rule of prisma_run_explore_smart as prisma_amd.explore restates
it, with a host action history of its own (one replica's row of the [R, T] layout).  Nothing is
read from the GPU."""
from __future__ import annotations

import numpy as np

from prisma_amd import explore


def history_rows(topo) -> np.ndarray:
    """row [n_nodes + 1]: node v's actions are columns row[v] .. row[v + 1], by underlay id (the
    overlay CSR: empty rows for nodes outside the overlay)."""
    return np.concatenate([[0], np.cumsum(topo.degrees.astype(np.int64))])


def big_pick(c, h) -> int:
    """The pick in plain Python integers (the statement of include/prisma.h, word for word)."""
    c = [int(x) for x in c]
    h = [int(x) for x in h]
    deg, nb = len(h), sum(h)
    W = (deg - 1) * nb
    if W == 0:
        return (c[1] * deg) >> 32
    u = ((((c[1] << 32) | c[2]) * W) >> 64)
    acc = 0
    for i in range(deg):
        acc += nb - h[i]
        if acc > u:
            return i
    raise AssertionError("u < W: some prefix exceeds it")


def histogram(topo, records) -> np.ndarray:
    """Counts [T] of (node, action) over the non-destination records with a valid action."""
    row = history_rows(topo)
    out = np.zeros(int(row[-1]), dtype=np.int64)
    rec = records[records["status"] != 3]
    deg = topo.degrees[rec["node"]]
    ok = (rec["action"] >= 0) & (rec["action"] < deg)
    np.add.at(out, row[rec["node"][ok]] + rec["action"][ok], 1)
    return out


class SmartSteppedOracle:
    """policy: ("table", uint8 [N, N]), ("mlp", packed fp32 DQN-buffer weights: the oracle's
    restatement of the argmin) or ("host", (lightq_util.HostMLP, packed fp32): a reduced model's
    host restatement).  thr: uint32 [N] by underlay id.  hist: the replica's counts
    [T] at the start (copied; ones by default).  base: global log index of this episode's first
    record (episodes after the first)."""

    def __init__(self, oracle_mod, topo, params, replica, thr, policy, hist=None, episode=0, base=0, scalar_check=True):
        self.O, self.topo, self.params = oracle_mod, topo, params
        self.scalar_check = scalar_check                   # smart_explore_action per decision beside the pick
        self.gid, self.episode, self.base = int(replica), int(episode), int(base)
        self.thr = np.asarray(thr, dtype=np.uint32)
        self.kind, self.pol = policy
        self.row = history_rows(topo)
        self.hist = (np.ones(int(self.row[-1]), dtype=np.uint32) if hist is None
                     else np.array(hist, dtype=np.uint32, copy=True))
        assert self.hist.shape == (int(self.row[-1]),)
        self.o = oracle_mod.OracleSim(topo, params, replica=replica, episode=episode)
        self.explored = self.changed = self.decisions = self.differing = 0
        self.min_W = None                                  # the smallest W over the explored decisions
        self.taken = []                                    # (node, action, explored) per decision
        self._c = np.zeros((0, 4), dtype=np.uint32)
        self.obs = self.o.step(-1)

    def n_records(self) -> int:
        return int(self.O.lib().or_record_count(self.o.h))

    def _draw(self, k):
        if k >= len(self._c):
            n = max(4096, 2 * (k + 1))
            self._c = explore.explore_draw(self.params["seed"], self.gid, self.base + np.arange(n), self.episode)
        return self._c[k]

    def _greedy(self, v):
        if self.kind == "table":
            return int(self.pol[v, int(self.topo.overlay_nodes[int(self.obs[0])])])
        if self.kind == "mlp":
            return self.o.mlp_action(self.pol, v, self.obs)
        host, w = self.pol
        return host.mlp_action(w, v, self.obs)

    def step(self) -> bool:
        """Answer the pending decision by the rule and count it; False once the episode is over."""
        if self.obs is None:
            return False
        v = self.o.pending_node()
        k = self.n_records() - 1                           # the pending decision's record
        deg = int(self.topo.degrees[v])
        g = self._greedy(v)
        c = self._draw(k)
        h = self.hist[self.row[v]: self.row[v] + deg]
        hit = (int(c[0]) >> 8) < int(self.thr[v])
        a = g
        if hit:
            a = explore.smart_pick(c, h)
            assert a == big_pick(c, h) and 0 <= a < deg
            W = (deg - 1) * int(h.astype(np.uint64).sum())
            self.min_W = W if self.min_W is None else min(self.min_W, W)
            self.differing += int(a != (int(c[1]) * deg) >> 32)
        if self.scalar_check:
            assert a == explore.smart_explore_action(self.params["seed"], self.gid, self.base + k, self.episode,
                                                     int(self.thr[v]), h, g)
        self.decisions += 1
        self.explored += int(hit)
        self.changed += int(hit and a != g)
        self.taken.append((v, a, hit))
        if 0 <= a < deg:
            h[a] += 1                                      # (a view of self.hist)
        self.obs = self.o.step(a)
        return True

    def run(self, until_records=None):
        """To the episode end, or until the first `until_records` records are final."""
        while self.obs is not None and (until_records is None or self.n_records() - 1 < until_records):
            self.step()
        return self

    def records(self, first=0, count=None):
        r = self.o.records(first, count).copy()
        r["prev"] = np.where(r["prev"] >= 0, r["prev"] + self.base, r["prev"])
        return r

    def counters(self):
        return self.o.counters()
