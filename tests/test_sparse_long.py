"""The sparse, full-length cases of tests/sparse_cases.py on the CPU oracle alone: the conditions
that keep the GPU parity runs (tests/test_gpu_sparse_long.py) from passing vacuously.  Each case's
episode ends inside its hop budget at t > 4080 s without an error flag; packets start after 2048 s
(the 12-bit start second's top bit) and rewards are taken from microsecond states above 2^31; the
idle cases have event gaps of 2^32 - 1 ns and more (every 32-bit offset of the event selection
saturates) and gaps in [2^31, 2^32 - 1) ns; records fall on py_micros' tie (t mod 1000 = 500); and
the DQN-buffer weights of sparse_cases.sp_equivalent_net decide as the shortest-path table does.

These thresholds are conditions, not measurements: each sits well inside what the oracle gives
(the ledger in sparse_cases.py).  A case that misses one is changed, not the threshold."""
import numpy as np
import pytest
import torch

import sparse_cases as S
from parity_util import check_near_ties, decisions_of


@pytest.mark.parametrize("name", list(S.CASES))
def test_oracle_run_reaches_both_regimes(name):
    c = S.CASES[name]
    ties = 0
    for r, (got, recs, cnt, trace) in enumerate(S.oracle_runs(name)):
        where = (name, S.REPLICA_BASE + r)
        s = S.summary(recs, trace)
        print(f"{name} replica {S.REPLICA_BASE + r}: hops {got} events {int(cnt['events'])} idle gaps {s['idle']} "
              f"half gaps {s['half']} record gaps {s['record_gaps']} records {s['records']} late {s['late']} "
              f"prev late {s['prev_late']} ties {s['ties']} ping rounds {int(cnt['ping_rounds'])} "
              f"end {int(cnt['now_ns']) / 1e9:.3f} s")
        assert int(cnt["error"]) == 0, where
        assert int(cnt["episode_over"]) == 1 and got == int(cnt["hops"]) < c["hops"], where
        assert len(recs) == int(cnt["dec_count"]) <= S.LOG, where
        assert int(cnt["now_ns"]) >= 4080 * 10**9, where
        assert s["max_start_s"] >= 4000, where
        assert s["late"] >= 1000, where
        assert s["prev_late"] >= 500, where
        assert s["idle"] >= c["idle"] and s["half"] >= c["half"], where
        assert len(trace) == int(cnt["events"]), where
        ties += s["ties"]
    assert ties >= 1, name


def test_idle_gap_thresholds_are_the_stated_ones():
    assert {n: (S.CASES[n]["idle"], S.CASES[n]["half"]) for n in S.IDLE_CASES} == {
        "idle": (100, 1), "idle_geant": (100, 1), "idle_ns3": (100, 1), "ctrl": (10, 1), "tunnelled": (10, 0)}
    assert S.CASES["pings"]["over"]["ping_interval_s"] == 1.0


def test_plan_takes_every_gpu_run():
    """prisma_plan accepts each case at sim_time_s = 4095 on the register-resident engine, at the
    shape the GPU runs assert, and the memory-resident engine's runs (`ctrl` among them) on that
    one; the identity cases without the ctrl paths keep their table in LDS (the fused instances)."""
    from prisma_amd import engine
    for name, c in S.CASES.items():
        p = engine.plan(S.case_topo(name), S.case_params(name, engine=engine.PRISMA_ENGINE_REGISTER))
        assert (p["engine"], p["flow_slots"], p["link_slots"]) == (engine.PRISMA_ENGINE_REGISTER, *S.SHAPES[c["topo"]])
        assert p["lds_bytes"] > p["lds_state_bytes"]
        assert engine.plan(S.case_topo(name), S.case_params(name))["engine"] == engine.PRISMA_ENGINE_REGISTER
    for name in {n for n, _ in S.MEMORY_RUNS}:
        p = engine.plan(S.case_topo(name), S.case_params(name, engine=engine.PRISMA_ENGINE_MEMORY))
        assert p["engine"] == engine.PRISMA_ENGINE_MEMORY
    assert (S.case_topo("idle_geant").n_flows + 63) // 64 == 8          # 506 flows: 8 blocks of 64


def test_pings_case_runs_every_round_of_the_episode():
    """A round per second from 0.0032 s on: k up to 4094, and no idle gap."""
    for _, _, cnt, trace in S.oracle_runs("pings"):
        assert int(cnt["ping_rounds"]) >= 4094
        assert S.gaps(trace[:, 0]) == (0, 0)


@pytest.mark.parametrize("name", S.MLP_CASES)
def test_sp_equivalent_weights_decide_as_the_table(name):
    """run_mlp under the hand-built weights writes the SP table's records byte for byte; torch's
    fp32 argmin agrees on every decision (no near-tie: the margin is 0.5), and the buffers branch
    really moves the Q values (but by less than 0.1)."""
    topo = S.case_topo(name)
    net, w = S.net(name)
    sp = S.table(name)
    import oracle as O
    checker = O.OracleSim(topo, S.case_params(name), replica=S.REPLICA_BASE)
    for (got_t, rec_t, cnt_t, _), (got_m, rec_m, cnt_m, _) in zip(S.oracle_runs(name), S.oracle_runs(name, "mlp")):
        assert got_m == got_t and rec_m.tobytes() == rec_t.tobytes()
        assert cnt_m.tobytes() == cnt_t.tobytes()
        n, differ, dq, gap = check_near_ties(net, w, checker, rec_m)
        assert n == got_m and differ == 0 and gap == 0.0 and dq < 1e-5
        dec = decisions_of(rec_m)
        node = torch.from_numpy(dec["node"].astype(np.int64))
        obs = torch.from_numpy(dec["obs"].astype(np.int64)).to(torch.int32)
        act = net.act(obs, node).numpy()
        assert np.array_equal(act, sp[dec["node"], topo.overlay_nodes[dec["obs"][:, 0]]])
        with torch.no_grad():
            q = net.q_values(obs, node).numpy()
        rows = np.arange(len(dec))
        q_sp = q[rows, act]
        q[rows, act] = np.inf
        others = q[np.isfinite(q)]
        assert q_sp.max() < np.expm1(-0.9) and others.min() > np.expm1(-0.1) and others.max() < 0.1
    checker.close()


@pytest.mark.parametrize("tname", ["abilene", "geant"])
def test_sp_equivalent_weights_at_any_buffer_occupancy(tname):
    """An idle network's FIFOs are empty at nearly every decision, so the runs above see the
    buffers branch at zero input.  At random occupancies (0 to 16 260 B per link, and a single
    full FIFO) it moves every Q, by less than 0.1, and the argmin stays the SP action at every
    (node, destination): the weights are SP-equivalent whatever the run observes."""
    topo = S.case_topo({"abilene": "idle", "geant": "idle_geant"}[tname])
    net, _ = S.sp_equivalent_net(topo)
    sp = S.table({"abilene": "idle", "geant": "idle_geant"}[tname])
    on = topo.overlay_nodes
    pairs = [(u, i) for u in on for i, d in enumerate(on) if d != u]
    node = torch.tensor([u for u, _ in pairs], dtype=torch.int64).repeat(8)
    rng = np.random.default_rng(2)
    obs = np.zeros((len(node), topo.obs_width), dtype=np.int64)
    obs[:, 0] = np.tile([i for _, i in pairs], 8)
    D = topo.max_deg
    obs[:len(node) // 2, 1:1 + D] = rng.integers(0, 16261, (len(node) // 2, D))
    rows = np.arange(len(node) // 2, len(node))
    obs[rows, 1 + rng.integers(0, topo.degrees[node.numpy()[rows]])] = 16260
    with torch.no_grad():
        q = net.q_values(torch.from_numpy(obs).to(torch.int32), node).numpy()
    want = sp[node.numpy(), on[obs[:, 0]]]
    assert np.array_equal(np.argmin(q, axis=1), want)
    r = np.arange(len(node))
    q_sp = q[r, want].copy()
    q[r, want] = np.inf
    others = q[np.isfinite(q)]
    assert q_sp.max() < np.expm1(-0.9) and q_sp.min() >= -1.0
    assert np.expm1(-0.1) < others.min() and others.max() < 0.1
    moved = np.abs(q_sp - np.float32(np.expm1(-1.0)))
    assert moved.max() > 1e-3 and (moved > 1e-5).mean() > 0.5 and np.abs(others).max() > 1e-3
