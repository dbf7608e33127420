"""The comparator of the exploration tests: one CPU oracle per replica driven decision by decision
(OracleSim.step) with the action prisma_amd.explore.explore_action gives over the oracle's own
greedy action -- the table entry, or the oracle's restatement of the DQN-buffer argmin.  Nothing
is read from the GPU."""
from __future__ import annotations

import numpy as np

from prisma_amd import explore


class SteppedOracle:
    """policy: ("table", uint8 [N, N]) or ("mlp", packed fp32).  thr: uint32 [N] by underlay id.
    base: global log index of this episode's first record (episodes after the first)."""

    def __init__(self, oracle_mod, topo, params, replica, thr, policy, episode=0, base=0, scalar_check=True):
        self.O, self.topo, self.params = oracle_mod, topo, params
        self.scalar_check = scalar_check                   # explore_action per decision beside the vectorised draw
        self.gid, self.episode, self.base = int(replica), int(episode), int(base)
        self.thr = np.asarray(thr, dtype=np.uint32)
        self.kind, self.pol = policy
        self.o = oracle_mod.OracleSim(topo, params, replica=replica, episode=episode)
        self.explored = self.changed = self.decisions = 0
        self._c = np.zeros((0, 4), dtype=np.uint32)        # the draws of decisions base .. base + len
        self.obs = self.o.step(-1)

    def n_records(self) -> int:
        return int(self.O.lib().or_record_count(self.o.h))

    def _draw(self, k):
        if k >= len(self._c):
            n = max(4096, 2 * (k + 1))
            self._c = explore.explore_draw(self.params["seed"], self.gid, self.base + np.arange(n), self.episode)
        return self._c[k]

    def step(self) -> bool:
        """Answer the pending decision by the rule; False once the episode is over."""
        if self.obs is None:
            return False
        v = self.o.pending_node()
        k = self.n_records() - 1                           # the pending decision's record
        deg = int(self.topo.degrees[v])
        if self.kind == "table":
            g = int(self.pol[v, int(self.topo.overlay_nodes[int(self.obs[0])])])
        else:
            g = self.o.mlp_action(self.pol, v, self.obs)
        c = self._draw(k)
        hit = (int(c[0]) >> 8) < int(self.thr[v])
        a = ((int(c[1]) * deg) >> 32) if hit else g
        if self.scalar_check:                              # the scalar rule says the same as the vectorised draw
            assert a == explore.explore_action(self.params["seed"], self.gid, self.base + k, self.episode,
                                               int(self.thr[v]), deg, g)
        assert 0 <= a < deg or not hit
        self.decisions += 1
        self.explored += int(hit)
        self.changed += int(hit and a != g)
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
