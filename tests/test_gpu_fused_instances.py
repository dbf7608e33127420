"""The seams between the fused-only table step kernels (prisma_step_kernel_fused_t: what run()
with a table launches on an identity-overlay env without the ctrl paths whose table sits in LDS)
and the general ones (what step() launches, and run() on every other env), bit-exact against the
CPU oracle after every launch: the two kernels alternating on one env, an episode end inside a fused launch with the
restart loop copy, a budget of one hop, an env whose table stays in HBM, and the dispatch itself.

The existing table parity tests exercise the fused instances; here the general lite instance runs
between fused launches, on the same state."""
import numpy as np
import pytest
import torch

import synth_topology as S
from prisma_amd.config import engine_params
from prisma_amd.engine import PrismaEngine
from prisma_amd.topology import Topology, sp_next_hop_table

from parity_util import OracleChain, assert_counters_equal, compare_steady, first_difference, random_table

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

R_BASE = 7


class Pair:
    """One engine and its replicas' oracles, driven in lockstep and compared after every launch."""

    def __init__(self, oracle_mod, topo, params, R, table, label):
        self.topo, self.R, self.table, self.label = topo, R, table, label
        self.eng = PrismaEngine(topo, params, R)
        self.orcs = [oracle_mod.OracleSim(topo, params, replica=params["replica_base"] + r) for r in range(R)]
        self.dev = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        self.rng = np.random.default_rng(3)
        self.eng.reset(0)
        self.pending = False
        self.obs = self.mask = self.node = self.ref_obs = None

    def close(self):
        self.eng.close()
        for o in self.orcs:
            o.close()

    def compare(self, where):
        """Every record written so far and the counters of every replica, byte for byte."""
        torch.cuda.synchronize()
        cnt = self.eng.counters()
        log = self.eng.log_tensor().cpu().numpy()
        for r, o in enumerate(self.orcs):
            ref = o.records()
            assert int(cnt[r]["error"]) == 0, (self.label, where, r, int(cnt[r]["error"]))
            assert int(cnt[r]["dec_count"]) == len(ref) <= self.eng.log_capacity, (self.label, where, r)
            got = self.eng.records(r, 0, len(ref), log_host=log)
            bad = first_difference(got, ref)
            assert bad is None, (f"{self.label} {where} replica {r}: record {bad} differs\n engine {got[bad]}\n "
                                 f"oracle {ref[bad]}")
            assert_counters_equal(cnt[r], o.counters(), r, f" ({self.label}, {where})")

    def _check_pending(self, where):
        g, m, nd = self.obs.cpu().numpy(), self.mask.cpu().numpy(), self.node.cpu().numpy()
        for r in range(self.R):
            assert self.ref_obs[r] is not None and m[r] == 1, (self.label, where, r)
            assert np.array_equal(self.ref_obs[r], g[r]), (self.label, where, r, g[r], self.ref_obs[r])
            assert nd[r] == self.orcs[r].pending_node(), (self.label, where, r)
        return nd

    def steps(self, n, where):
        """n prisma_step launches with random valid actions (the first with none, when nothing is
        pending); a decision is left pending.  Observation, mask and node compared every launch."""
        if not self.pending:
            self.ref_obs = [o.step(-1) for o in self.orcs]
            self.obs, self.mask, self.node = self.eng.step(None)
            self.pending = True
        for s in range(n):
            nd = self._check_pending(f"{where} step {s}")
            acts = np.array([self.rng.integers(0, self.topo.degrees[nd[r]]) for r in range(self.R)], dtype=np.int32)
            self.ref_obs = [self.orcs[r].step(int(acts[r])) for r in range(self.R)]
            self.obs, self.mask, self.node = self.eng.step(torch.from_numpy(acts).cuda())
        self._check_pending(f"{where} last step")

    def run(self, hops, where):
        """One fused launch of `hops` hops: it opens with the pending decision, if one is."""
        self.eng.run(self.dev, hops)
        for o in self.orcs:
            assert o.run_table(self.table, hops) == hops, (self.label, where)
        self.pending = False
        self.compare(where)


def _alternate(oracle_mod, topo, params, table, label, fused):
    p = Pair(oracle_mod, topo, params, 3, table, label)
    try:
        assert p.eng.kernel_name_step.startswith("prisma_step_kernel_t<")
        assert p.eng.kernel_name.startswith("prisma_step_kernel_fused_t<") == fused, p.eng.kernel_name
        p.steps(40, "first external")
        for hops in (1, 7, 300):
            p.run(hops, f"fused {hops}")             # opens with the decision the step left pending
            p.steps(25, f"external after fused {hops}")   # and the external kernel picks up after it
        p.run(300, "last fused")
        p.run(300, "fused after fused")              # (nothing pending at its start)
    finally:
        p.close()


@pytest.mark.parametrize("ping", [0, 1])
def test_alternating_kernels_abilene(oracle_mod, ping):
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=ping, replica_base=R_BASE, log_capacity=8192)
    _alternate(oracle_mod, topo, params, sp_next_hop_table(topo), f"abilene ping {ping}", fused=True)


def test_alternating_kernels_tunnelled(oracle_mod):
    """A tunnelled overlay (table in LDS, no ctrl paths): no fused instance, the general one on both sides."""
    topo = Topology.example("overlay_full_mesh_3n_abilene", 0, 10.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=8192)
    _alternate(oracle_mod, topo, params, random_table(topo, 11), "mesh3 lf 10", fused=False)


def test_alternating_kernels_table_in_hbm(oracle_mod):
    """l100_f128: with the table in LDS one replica fewer would fit a CU, so it stays in HBM, and
    fused runs stay on the general instance (no fused instance reads the table from HBM)."""
    name = "l100_f128"
    assert S.CASES[name]["table_in_lds"][0] == 0
    topo = S.build(name)
    _alternate(oracle_mod, topo, S.case_params(name), sp_next_hop_table(topo), name, fused=False)


def _episode_hops(oracle_mod, topo, params, table, R):
    """Hops of episodes 0 and 1 of every replica (oracle, CPU)."""
    out = []
    for r in range(R):
        ch = OracleChain(oracle_mod, topo, params, params["replica_base"] + r, ("table", table))
        e = []
        for _ in range(2):
            e.append(ch._run(1 << 30))
            ch._next_episode()
        out.append(e)
    return np.array(out)


@pytest.mark.parametrize("ends", [1, 2])
def test_episode_end_inside_fused_launch(oracle_mod, ends):
    """sim_time_s 0.75 with auto_reset: a budget that crosses the episode's end once continues in
    the restart loop copy and spends the rest in episode 1; one that would cross a second end
    stops the replica there (the launch executes fewer hops than asked), and the reset kernel
    starts episode 2."""
    topo = Topology.example("abilene", 0, 1.0)
    table = sp_next_hop_table(topo)
    R = 2
    params = engine_params(topo, sim_time_s=0.75, ping_as_obs=1, auto_reset=1, replica_base=R_BASE, log_capacity=32768)
    e = _episode_hops(oracle_mod, topo, params, table, R)
    assert e.min() > 100
    if ends == 1:
        budget = int(e[:, 0].max() + e[:, 1].min() // 2)
        assert e[:, 0].max() < budget < e.sum(axis=1).min()
    else:
        budget = int(e.sum(axis=1).max() + 100)
    eng = PrismaEngine(topo, params, R)
    try:
        assert eng.kernel_name.startswith("prisma_step_kernel_fused_t<")
        eng.reset(0)
        out = compare_steady(oracle_mod, eng, topo, params, ("table", table), t_target_s=0.0,
                             hops_per_launch=budget, label=f"episode end x{ends}")
        assert out["launches"] == 1 and out["episodes"] == [ends] * R
        assert out["short_launches"] == (R if ends == 2 else 0)
        assert out["hops"] == (int(e.sum()) if ends == 2 else budget * R)
    finally:
        eng.close()


def test_budget_of_one_hop(oracle_mod):
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=8192)
    p = Pair(oracle_mod, topo, params, 3, sp_next_hop_table(topo), "one hop")
    try:
        assert p.eng.kernel_name.startswith("prisma_step_kernel_fused_t<")
        p.run(200, "warm")
        for k in range(5):
            p.run(1, f"one hop {k}")
    finally:
        p.close()


def test_dispatch_names():
    topo = Topology.example("abilene", 0, 1.0)
    for train, fused in ((0, True), (1, False)):
        eng = PrismaEngine(topo, engine_params(topo, sim_time_s=30.0, ping_as_obs=1, train=train), 2)
        try:
            ctrl = "true" if train else "false"
            assert eng.kernel_info()["ctrl"] == train
            assert eng.kernel_name_step == f"prisma_step_kernel_t<2, 1, false, false, {ctrl}>"
            assert eng.kernel_name_mlp == f"prisma_step_kernel_t<2, 1, true, false, {ctrl}>"
            assert eng.kernel_name == ("prisma_step_kernel_fused_t<2, 1, false, false>" if fused else eng.kernel_name_step)
        finally:
            eng.close()
