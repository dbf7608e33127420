"""History-weighted ("smart") exploration of the fused rollouts, the parts that need no GPU: the
host restatements of the pick (prisma_amd/explore.py) against a big-integer loop and against the
probabilities, the rule driving the CPU oracle, the C-ABI entries, the flag and the trainer's
external path."""
import os
import re
import subprocess

import numpy as np
import torch

from prisma_amd import engine, explore
from prisma_amd.config import DEFAULTS, engine_params, parse_arguments
from prisma_amd.topology import Topology, sp_next_hop_table
from prisma_amd.trainer import QRoutingTrainer

from smart_explore_util import SmartSteppedOracle, big_pick, histogram, history_rows


def _rows(rng, deg, n):
    """n random rows of one degree: small counts, counts up to 2^31, zero rows, one-hot rows."""
    h = np.where(rng.random((n, 1)) < 0.5, rng.integers(0, 60, size=(n, deg)),
                 rng.integers(0, (1 << 31) + 1, size=(n, deg))).astype(np.uint32)
    h[rng.random(n) < 0.1] = 0
    one = rng.random(n) < 0.1                              # every count but one zero: W > 0, zero weights
    h[one] = 0
    h[one, rng.integers(0, deg, size=int(one.sum()))] = rng.integers(1, 1 << 31, size=int(one.sum()))
    return h


def test_restatements_agree_with_big_integers():
    rng = np.random.default_rng(11)
    seen_fallback = seen_big = 0
    for deg in range(1, 56):
        n = 40
        h = _rows(rng, deg, n)
        c = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
        c[0, 1], c[0, 2] = 0xFFFFFFFF, 0xFFFFFFFF          # the largest u
        c[1, 1], c[1, 2] = 0, 0                            # the smallest
        want = np.array([big_pick(c[i], h[i]) for i in range(n)])
        got = explore.smart_pick(c, h)
        assert got.dtype == np.int64 and np.array_equal(got, want), deg
        for i in range(n):
            one = explore.smart_pick(c[i], h[i])
            assert isinstance(one, int) and one == want[i], (deg, i)
        assert want.min() >= 0 and want.max() < deg
        W = (deg - 1) * h.astype(np.uint64).sum(axis=1)
        seen_fallback += int((W == 0).sum())
        seen_big += int((W >= np.uint64(1 << 32)).sum())
        # a weighted pick never lands on an action with weight 0 (the only one taken so far)
        for i in np.nonzero(W > 0)[0]:
            nb = int(h[i].astype(np.uint64).sum())
            assert int(h[i, want[i]]) < nb
    assert seen_fallback > 100 and seen_big > 500


def test_zero_weight_fallback_is_the_uniform_pick():
    d = np.arange(5000)
    c = explore.explore_draw(100, 3, d, 0)
    for deg in (1, 2, 7, 55):
        uni = explore.explore_action(100, 3, d, 0, 1 << 24, deg, -1)
        zero = np.zeros((len(d), deg), dtype=np.uint32)
        assert np.array_equal(explore.smart_pick(c, zero), uni)
        assert np.array_equal(explore.smart_explore_action(100, 3, d, 0, 1 << 24, zero, -1), uni)
    # degree 1 with any count: W = 0 as well
    assert np.all(explore.smart_pick(c, np.full((len(d), 1), 9, dtype=np.uint32)) == 0)
    # below the threshold: the greedy action, whatever the history
    g = np.full(d.shape, 4)
    assert np.array_equal(explore.smart_explore_action(100, 3, d, 0, 0, np.ones((len(d), 5), dtype=np.uint32), g), g)
    one = explore.smart_explore_action(100, 3, 17, 0, 1 << 24, np.array([5, 1, 1], dtype=np.uint32), 0)
    assert isinstance(one, int) and one == big_pick(c[17], [5, 1, 1])


def test_frequencies_follow_the_weights():
    n = 1 << 16
    c = explore.explore_draw(100, 9, np.arange(n), 0)
    rows = [[1, 1, 1], [1000, 1, 1, 1], [3, 0, 5, 7, 2], [1 << 31, 1 << 30, 5, 1 << 29],
            [(i + 1) << 21 for i in range(33)], list(range(1, 56)), [0, 0, 4]]
    for h in rows:
        deg, nb = len(h), sum(h)
        p = np.array([(nb - x) / ((deg - 1) * nb) for x in h])
        assert abs(p.sum() - 1.0) < 1e-12
        a = explore.smart_pick(c, np.tile(np.array(h, dtype=np.uint32), (n, 1)))
        freq = np.bincount(a, minlength=deg) / n
        sigma = np.sqrt(p * (1 - p) / n)
        worst = np.max(np.abs(freq - p) - 5 * sigma)
        print(f"deg {deg}: largest |freq - p| - 5 sigma = {worst:.3e}")
        assert np.all(np.abs(freq - p) <= 5 * sigma), (h[:6], freq, p)


def test_oracle_under_the_rule(oracle_mod):
    """The rule drives the oracle by step(): Abilene TM0, load 1.0, 2 s, eps 0.3 everywhere."""
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=2.0)
    table = sp_next_hop_table(topo)
    thr = np.full(topo.n_nodes, explore.thresholds(0.3), dtype=np.uint32)
    T = int(history_rows(topo)[-1])
    for r in range(2):
        s = SmartSteppedOracle(oracle_mod, topo, params, r, thr, ("table", table)).run()
        c = s.counters()
        print(f"replica {r}: {s.decisions} decisions, {s.explored} explored, {s.changed} changed, "
              f"{s.differing} differ from the uniform pick, error {int(c['error'])}")
        assert int(c["error"]) == 0 and int(c["episode_over"]) == 1
        assert s.explored > 500 and s.changed > 200 and s.differing > 100
        assert np.array_equal(s.hist.astype(np.int64), 1 + histogram(topo, s.records()))
        assert int(s.hist.sum()) == T + s.decisions
    # threshold 0: the greedy run, and the history is still its histogram
    z = SmartSteppedOracle(oracle_mod, topo, params, 1, np.zeros(topo.n_nodes, dtype=np.uint32), ("table", table)).run()
    o = oracle_mod.OracleSim(topo, params, replica=1)
    o.run_table(table, 10 ** 9)
    assert z.explored == 0 and z.records().tobytes() == o.records().tobytes()
    assert np.array_equal(z.hist.astype(np.int64), 1 + histogram(topo, o.records()))


def test_library_exports_the_smart_entries():
    assert {"prisma_run_explore_smart", "prisma_action_history_layout"} <= set(engine.EXPORTS)
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_engine()
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    defined = set(re.findall(r" T (prisma_\w+)", out))
    assert {"prisma_run_explore_smart", "prisma_action_history_layout"} <= defined
    assert lib.prisma_run_explore_smart(None, 1, None, 1, None, None, 0, None) == -5     # PRISMA_ERR_ARG, no exit
    assert lib.prisma_action_history_layout(None, None, None) == -5
    assert lib.prisma_abi_version() == 10


def test_flag_parses():
    assert DEFAULTS["smart_exploration"] == 0
    assert parse_arguments([])["smart_exploration"] == 0
    assert parse_arguments(["--smart_exploration", "1"])["smart_exploration"] == 1


def test_trainer_act_counts_what_it_returns():
    topo = Topology.example("abilene", 0, 1.0)
    R = 64
    tr = QRoutingTrainer(topo, "routing", seed=3, device="cpu", n_replicas=R, smart_exploration=True)
    row = history_rows(topo)
    T = int(row[-1])
    assert tr.action_history.shape == (R, T) and tr.action_history.dtype == torch.int32
    assert torch.all(tr.action_history == 1) and tr.stats()["action_history_total"] == R * T
    assert QRoutingTrainer(topo, "routing", device="cpu").action_history is None
    g = torch.Generator().manual_seed(5)
    want = np.ones((R, T), dtype=np.int64)
    counted = 0
    for it in range(40):
        node = torch.randint(0, topo.n_nodes, (R,), generator=g, dtype=torch.int32)
        node[it % R] = -1                                  # no notification: nothing counted
        obs = torch.zeros((R, topo.obs_width), dtype=torch.int32)
        obs[:, 0] = torch.randint(0, topo.n_nodes, (R,), generator=g, dtype=torch.int32)
        obs[(it + 7) % R, 0] = 1000                        # a control notification: nothing counted
        a = tr.act(obs, node, explore=(it % 4 != 3))       # eps 1 at the start: every pick explores
        for r in range(R):
            if int(node[r]) >= 0 and int(obs[r, 0]) != 1000:
                v, x = int(node[r]), int(a[r])
                assert 0 <= x < int(topo.degrees[v])
                want[r, row[v] + x] += 1
                counted += 1
    assert np.array_equal(tr.action_history.numpy().astype(np.int64), want)
    assert tr.stats()["action_history_total"] == R * T + counted and counted > 2000
    # the weights bite: an action taken 10^6 times more often than the others is all but avoided
    tr.action_history[:] = 1
    tr.action_history[:, torch.from_numpy(row[:-1])] = 1000000
    node = torch.full((R,), 1, dtype=torch.int32)
    obs = torch.zeros((R, topo.obs_width), dtype=torch.int32)
    picks = torch.cat([tr.act(obs, node) for _ in range(20)])
    assert int(topo.degrees[1]) > 1 and float((picks == 0).double().mean()) < 0.02
