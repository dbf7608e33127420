"""The comparator of the stochastic-routing ("opt") tests: one CPU oracle per replica driven
decision by decision (OracleSim.step) under the rule of prisma_run_stochastic as
prisma_amd.optrouting restates it.  A packet's source and its previous (node, action) come from
the oracle's own records through their `prev` chain.  Nothing is read from the GPU.

Also here: the plain-Python statement of the pick, and a literal restatement of the reference's
optimal_routing_decision that carries an explicit per-packet tag and takes its draws injected."""
from __future__ import annotations

import numpy as np

from prisma_amd import optrouting


def big_pick(c1, wt) -> int:
    """The drawn action in plain Python integers (the statement of include/prisma.h, word for word)."""
    c1 = int(c1)
    wt = [int(x) for x in wt]
    deg, W = len(wt), sum(wt)
    if W == 0:
        return (c1 * deg) >> 32
    u = (c1 * W) >> 32
    acc = 0
    for i in range(deg):
        acc += wt[i]
        if acc > u:
            return i
    raise AssertionError("u < W: some prefix exceeds it")


def literal_decision(prob_to_neighbors, tag, injected_choice):
    """utils.py:161-199 optimal_routing_decision after its lookups, word for word, with the index
    np.random.choice would have drawn given as `injected_choice`: returns (action, tag, followed).
    prob_to_neighbors: float64 routing[src][dst][the deciding node's edges]."""
    if tag:
        if tag in prob_to_neighbors and tag < 1:
            return list(prob_to_neighbors).index(tag), tag, True
    choice = int(injected_choice)
    tag = prob_to_neighbors[choice]
    return choice, tag, False


class OptSteppedOracle:
    """routing: float64 [NO, NO, T] in the reference's edge order (packed here).  base: global log
    index of this episode's first record (episodes after the first)."""

    def __init__(self, oracle_mod, topo, params, replica, routing, episode=0, base=0):
        self.O, self.topo, self.params = oracle_mod, topo, params
        self.gid, self.episode, self.base = int(replica), int(episode), int(base)
        self.routing = np.asarray(routing, dtype=np.float64)
        self.tab = optrouting.pack_routing(topo, self.routing)
        self.row = optrouting.edge_rows(topo)
        self.col = optrouting.reference_edges(topo)[1]     # reference edge -> table column
        self.o = oracle_mod.OracleSim(topo, params, replica=replica, episode=episode)
        self.src = {}                                      # record index -> the packet's source (underlay id)
        self.dec = {}                                      # record index -> (node, action) of that decision
        self.follows = self.draws = self.follows_nonzero = self.decisions = 0
        self.trace = []                                    # one dict per decision (the CPU tests replay it)
        self._c = np.zeros((0, 4), dtype=np.uint32)
        self.obs = self.o.step(-1)

    def n_records(self) -> int:
        return int(self.O.lib().or_record_count(self.o.h))

    def _draw(self, k):
        if k >= len(self._c):
            n = max(4096, 2 * (k + 1))
            self._c = optrouting.stoch_draw(self.params["seed"], self.gid, self.base + np.arange(n), self.episode)
        return self._c[k]

    def step(self) -> bool:
        """Answer the pending decision by the rule; False once the episode is over."""
        if self.obs is None:
            return False
        k = self.n_records() - 1                           # the pending decision's record
        rec = self.o.records(k, 1)[0]
        v, p = int(rec["node"]), int(rec["prev"])
        assert v == self.o.pending_node()
        src = v if p < 0 else self.src[p]
        prev = None if p < 0 else self.dec[p]
        s, t = int(self.topo.overlay_index[src]), int(self.topo.overlay_index[int(rec["dst"])])
        assert t == int(self.obs[0])
        deg = int(self.topo.degrees[v])
        # the rule on the cached draws; every 16th decision also through the scalar restatement
        st = self.tab[s, t]
        e = st[self.row[v]: self.row[v] + deg]
        wt = e & np.uint32(0xFFFFFF)
        c_prev = 0
        if prev is not None and 0 <= prev[1] < int(self.topo.degrees[prev[0]]):
            c_prev = int(st[self.row[prev[0]] + prev[1]]) >> 24
        m = np.flatnonzero((e >> np.uint32(24)) == c_prev) if c_prev else np.zeros(0, dtype=np.int64)
        followed = bool(m.size)
        c = self._draw(k)
        a = int(m[0]) if followed else big_pick(c[1], wt)
        if k % 16 == 0:
            assert (a, followed) == optrouting.stoch_action(self.tab, self.row, s, t, v, prev, self.params["seed"],
                                                            self.gid, self.base + k, self.episode, with_branch=True)
            assert followed or a == optrouting.stoch_pick(int(c[1]), wt)
        assert 0 <= a < deg
        self.decisions += 1
        self.follows += int(followed)
        self.follows_nonzero += int(followed and a != 0)
        self.draws += int(not followed)
        self.trace.append(dict(k=k, uid=int(rec["uid"]), s=s, t=t, v=v, prev=prev, action=a, followed=followed,
                               W=int(wt.astype(np.uint64).sum())))
        self.src[k], self.dec[k] = src, (v, a)
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

    def node_probs(self, s, t, v):
        """float64 routing[s][t][node v's edges], in action order (the reference's prob_to_neighbors)."""
        q = np.zeros(int(self.row[-1]), dtype=np.float64)
        q[self.col] = self.routing[s, t]
        return q[self.row[v]: self.row[v + 1]]
