"""Epsilon-greedy exploration of the fused rollouts, the parts that need no GPU: the host
restatement of the draw rule (prisma_amd/explore.py), the new C-ABI entry, the trainer's epsilons,
and the rule driving the CPU oracle."""
import os
import re
import subprocess

import numpy as np
import torch

from prisma_amd import engine, explore
from prisma_amd.config import engine_params
from prisma_amd.topology import Topology, sp_next_hop_table
from prisma_amd.trainer import LinearSchedule, QRoutingTrainer

from explore_util import SteppedOracle


def test_philox_matches_the_oracle(oracle_mod):
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(1000, 2), dtype=np.uint64)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    got = explore.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (1000, 4)
    for i in range(1000):
        assert got[i].tolist() == oracle_mod.philox(ctr[i].tolist(), key[i].tolist()), i
    # the published known-answer vector of Philox4x32-10 (Random123 kat_vectors)
    assert explore.philox4x32_10([0, 0, 0, 0], [0, 0]).tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # a broadcast key gives the rows the full call gives
    assert np.array_equal(explore.philox4x32_10(ctr[:5], key[3]), explore.philox4x32_10(ctr[:5], np.tile(key[3], (5, 1))))


def test_thresholds_and_picks():
    assert explore.thresholds(0.0) == 0 and explore.thresholds(1.0) == 1 << 24
    assert explore.thresholds(-0.5) == 0 and explore.thresholds(7.0) == 1 << 24
    eps = np.linspace(0.0, 1.0, 4097)
    thr = explore.thresholds(eps)
    assert thr.dtype == np.uint32 and np.all(np.diff(thr.astype(np.int64)) >= 0)
    assert explore.thresholds(0.1) == int(np.floor(0.1 * (1 << 24) + 0.5))
    d = np.arange(20000)
    for deg in (1, 2, 3, 5, 127):
        a = explore.explore_action(100, 3, d, 0, 1 << 24, deg, -7)       # always explores
        assert a.min() >= 0 and a.max() < deg
        if deg > 1:
            assert len(np.unique(a)) == deg
    g = np.full(d.shape, 2)
    assert np.array_equal(explore.explore_action(100, 3, d, 0, 0, 4, g), g)          # never explores
    a = explore.explore_action(100, 3, d, 0, explore.thresholds(0.25), 4, np.full(d.shape, 9))
    frac = np.mean(a != 9)
    assert abs(frac - 0.25) < 4 * np.sqrt(0.25 * 0.75 / d.size)          # 4 sigma of the binomial
    # scalars in, int out; the draw is keyed on every argument
    one = explore.explore_action(100, 3, 17, 0, 1 << 24, 1000, 0)
    assert isinstance(one, int) and one == int(explore.explore_action(100, 3, d, 0, 1 << 24, 1000, 0)[17])
    base = explore.explore_draw(100, 3, 17, 0)
    for other in (explore.explore_draw(101, 3, 17, 0), explore.explore_draw(100, 4, 17, 0),
                  explore.explore_draw(100, 3, 18, 0), explore.explore_draw(100, 3, 17, 1)):
        assert not np.array_equal(base, other)
    # counter word 3 = 2: apart from the flow start offsets (0) and the send delays (1)
    assert np.array_equal(base, explore.philox4x32_10([17, 0, 0, 2], [100, 3]))


def test_library_exports_prisma_run_explore():
    assert "prisma_run_explore" in engine.EXPORTS
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_engine()
    lib = engine.load_library()
    assert hasattr(lib, "prisma_run_explore")
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert "prisma_run_explore" in set(re.findall(r" T (prisma_\w+)", out))
    assert lib.prisma_run_explore(None, 1, None, 1, None, None) == -5                # PRISMA_ERR_ARG, no exit
    assert lib.prisma_abi_version() == 10


def test_explore_eps_is_the_linear_schedule_of_transitions_seen():
    topo = Topology.example("overlay_full_mesh_3n_abilene")
    tr = QRoutingTrainer(topo, "routing", seed=1, device="cpu", iteration_num=3000)
    assert (topo.degrees == 0).any()                       # underlay-only nodes decide nothing
    eps = tr.explore_eps()
    assert eps.shape == (topo.n_nodes,)
    assert torch.all(eps[torch.from_numpy(topo.degrees > 0)] == 1.0) and torch.all(eps[torch.from_numpy(topo.degrees == 0)] == 0.0)
    seen = torch.arange(topo.n_nodes, dtype=torch.int64) * 700
    tr.transitions_seen = seen.clone()
    want = LinearSchedule(3000, 1.0, 0.1).value(seen)
    want[torch.from_numpy(topo.degrees == 0)] = 0.0
    assert torch.equal(tr.explore_eps(), want)
    # past the schedule's end: its final value (1.0 + 1.0 * (0.1 - 1.0) in float64)
    tr.transitions_seen = torch.full_like(seen, 10 ** 6)
    assert torch.all(tr.explore_eps()[torch.from_numpy(topo.degrees > 0)] == 1.0 + (0.1 - 1.0))


def test_oracle_under_the_rule(oracle_mod):
    """The rule drives the oracle by step(): Abilene TM0, load 1.0, 2 s, eps 0.3 everywhere."""
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=2.0)
    table = sp_next_hop_table(topo)
    thr = np.full(topo.n_nodes, explore.thresholds(0.3), dtype=np.uint32)
    for r in range(3):
        s = SteppedOracle(oracle_mod, topo, params, r, thr, ("table", table)).run()
        c = s.counters()
        print(f"replica {r}: {s.decisions} decisions, {s.explored} explored, {s.changed} changed, error {int(c['error'])}")
        assert int(c["error"]) == 0 and int(c["episode_over"]) == 1
        assert s.explored > 500 and s.changed > 200
        rec = s.records()
        hops = rec[rec["status"] != 3]
        assert np.all((hops["action"] >= 0) & (hops["action"] < topo.degrees[hops["node"]]))
    # threshold 0: the stepped oracle is run_table, every counter included
    z = SteppedOracle(oracle_mod, topo, params, 1, np.zeros(topo.n_nodes, dtype=np.uint32), ("table", table)).run()
    o = oracle_mod.OracleSim(topo, params, replica=1)
    o.run_table(table, 10 ** 9)
    assert z.explored == 0 and z.records().tobytes() == o.records().tobytes()
    assert z.counters().tobytes() == o.counters().tobytes()
