"""The parameter matrix of tests/param_cases.py, checked without a GPU: prisma_plan picks the
expected engine for every case and topology, the plain-Python sizing() gives the sizing classes
the matrix states and, on identity overlays, prisma_plan's ring_entries; the oracle's own run of
each case meets the conditions that make it worth a GPU parity run
(tests/test_gpu_param_matrix.py): wires fuller than the default 4 (and than 8, 16) slots, FIFOs
that hold no or one data packet, a moving-average window that wraps, an episode that ends; and
prisma_plan refuses what lies beyond the engines' limits."""
import functools

import numpy as np
import pytest

import param_cases as P
from prisma_amd import engine
from prisma_amd.records import ST_DROPPED, ST_ENQUEUED

ALL_PAIRS = [(n, t) for n in P.CASES for t in P.TOPOS if not (t == P.TUNNELLED and n in P.IDENTITY_ONLY)]
PAIRS = [p for p in ALL_PAIRS if p not in P.NO_ENGINE]


@pytest.mark.parametrize("name,tname", PAIRS)
def test_plan_and_sizing(name, tname):
    c, tp, params = P.CASES[name], P.case_topo(name, tname), P.case_params(name, tname)
    p = engine.plan(tp, params)
    assert p["engine"] == engine.PRISMA_ENGINE_REGISTER
    s = P.sizing(params, tp)
    assert (s["WCAP"], s["data_max"]) == (c["wcap"], c["data_max"])
    if tp.identity:
        assert (s["PBK"], s["qs"]) == (c["pbk"], c["qs"])
        assert s["qs"] % s["WCAP"] == 0
        assert s["ring_entries"] == p["ring_entries"]
        if name in P.MEMORY_CASES:
            m = engine.plan(tp, dict(params, engine=engine.PRISMA_ENGINE_MEMORY))
            assert m["engine"] == engine.PRISMA_ENGINE_MEMORY and m["ring_entries"] == s["ring_entries"]
    else:
        assert s["ring_multiple"] == max(c["wcap"], 4) and p["ring_entries"] % s["ring_multiple"] == 0


def test_gpu_runs_cover_the_sizing_classes():
    """What tests/test_gpu_param_matrix.py runs on each engine: every wire capacity the engine
    accepts, the ping-back rings of 2 to 64 slots, data_max 0, 1 and 300, windows of 1 and 64."""
    reg = {n for n, _, _ in P.REGISTER_RUNS}
    mem = {n for n, _, _ in P.MEMORY_RUNS}
    assert reg == set(P.CASES)
    assert {P.CASES[n]["wcap"] for n in reg} == {2, 4, 8, 16, 32, 64}
    assert {P.CASES[n]["wcap"] for n in mem} == {2, 4, 8, 16}
    for runs in (reg, mem):
        assert {P.CASES[n]["pbk"] for n in runs} == {2, 4, 16, 32, 64}
        assert {0, 1, 10, 30, 172, 300} <= {P.CASES[n]["data_max"] for n in runs}
        assert {1, 5, 64} <= {P.case_params(n, "abilene")["ma_size"] for n in runs}
    for n in P.TUNNELLED_RUNS + [n for n, _ in P.EXPLORE_RUNS] + [n for n, _, _ in P.STEP_RUNS]:
        assert n in P.CASES and n not in P.IDENTITY_ONLY
    assert all(n in P.MEMORY_CASES for n, _, e in P.STEP_RUNS if e == "memory")
    total = len(P.REGISTER_RUNS) + len(P.MEMORY_RUNS) + len(P.TUNNELLED_RUNS) + len(P.EXPLORE_RUNS) + len(P.STEP_RUNS)
    assert total <= 110


@functools.lru_cache(maxsize=None)
def _oracle_runs(name, tname, kind="table"):
    """The case's R replicas on the oracle alone: (hops run, records, counters, diagnostics) each."""
    import oracle as O
    O.build()
    tp, params = P.case_topo(name, tname), P.case_params(name, tname)
    _, pol = P.policy(tname, kind)
    out = []
    for r in range(P.R):
        o = O.OracleSim(tp, params, replica=P.REPLICA_BASE + r)
        H = P.CASES[name]["hops"]
        got = o.run_table(pol, H) if kind == "table" else o.run_mlp(pol, H)
        out.append((got, o.records(), o.counters(), o.diag()))
        o.close()
    return out


@pytest.mark.parametrize("name,tname", ALL_PAIRS)
def test_oracle_run_meets_the_premises(name, tname):
    c, tp = P.CASES[name], P.case_topo(name, tname)
    H = c["hops"]
    for r, (got, recs, cnt, d) in enumerate(_oracle_runs(name, tname)):
        where = (name, tname, r)
        drops = int((recs["status"] == ST_DROPPED).sum())
        hops = int(((recs["status"] == ST_DROPPED) | (recs["status"] == ST_ENQUEUED)).sum())
        print(f"{name} {tname} replica {P.REPLICA_BASE + r}: hops {got} max_wire {d['max_wire']} max_queue "
              f"{d['max_queue']} peak_ring {d['peak_ring']} drops {drops} relay_drops {d['relay_drops']} "
              f"ping_rounds {int(cnt['ping_rounds'])} ctrl_dropped {int(cnt['ctrl_dropped'])}")
        assert int(cnt["error"]) == 0 and got == int(cnt["hops"]) == hops, where
        assert len(recs) <= P.LOG or H > P.H, where
        assert d["max_wire"] <= c["wcap"], where
        if tp.identity:                            # the sizing promise: a ring holds its FIFO and its wire
            assert d["max_queue"] + d["max_wire"] <= c["qs"] and d["peak_ring"] <= c["qs"], where
        if name == "sim750ms":
            assert int(cnt["episode_over"]) == 1 and got < H, where
        else:
            assert int(cnt["episode_over"]) == 0 and got == H, where
        if name == "delay6_pkt64_train":           # more than the default 4 slots; than a WCAP of 8
            assert d["max_wire"] >= (9 if tp.identity else 5), where
        if name in P.WCAP64:
            assert d["max_wire"] >= 17, where
        if H == P.H_PKT64:                         # pings run; where the load fills the FIFOs, they drop
            assert int(cnt["ping_rounds"]) >= 2, where
            assert tname == "geant" or drops > 0, where
        if name == "delay0":
            assert d["max_wire"] <= 2, where
        if name == "buf541":
            assert drops == got == H and d["max_queue"] == 0, where
        if name == "buf542":
            assert drops > 0 and d["max_queue"] == 1, where
            assert tp.identity or d["relay_drops"] > 0, where
        if name == "buf162600":
            assert drops == 0, where
            assert tname != "abilene" or d["max_queue"] > 100, where
        if name == "cap5M":
            assert tname != "abilene" or drops > 0, where
        if name.startswith("ping10ms"):
            assert int(cnt["ping_rounds"]) >= 64 and int(cnt["ctrl_dropped"]) > 0, where
        if name == "ping100s":
            assert int(cnt["ping_rounds"]) == 0, where
        if name.startswith("penalty"):
            assert tname != "abilene" or drops > 300, where


@pytest.mark.parametrize("name", ["delay6_pkt64_train", "delay35_pkt64", "delay28_pkt64_train"])
def test_deep_wires_under_the_mlp_policy(name):
    """The DQN-buffer runs of the deep-wire cases on Abilene end without an error flag (9 000 hops
    stay inside the log).  With --train the 30-B echoes fill more than half the wire slots; without,
    a wire holds back-to-back data packets: one per 94-B transmission of the propagation delay."""
    params = P.case_params(name, "abilene")
    want = P.CASES[name]["wcap"] // 2 + 1 if params["train"] else params["link_delay_ns"] // (94 * 8 * 2000)
    for got, _, cnt, d in _oracle_runs(name, "abilene", "mlp"):
        print(f"{name} abilene mlp: max_wire {d['max_wire']} peak_ring {d['peak_ring']}")
        assert got == P.H_PKT64 and int(cnt["error"]) == 0
        assert want <= d["max_wire"] <= P.CASES[name]["wcap"]
        assert d["peak_ring"] <= P.CASES[name]["qs"]


def test_moving_average_window_changes_the_mlp_decisions():
    """A 64-word and a 1-word window give the DQN-buffer model other ping observations, and it
    decides differently: the window is live in the parity runs."""
    a = _oracle_runs("ping10ms_ma64", "abilene", "mlp")
    b = _oracle_runs("ping10ms_ma1", "abilene", "mlp")
    for (_, ra, _, _), (_, rb, _, _) in zip(a, b):
        n = min(len(ra), len(rb))
        assert not np.array_equal(ra["obs"][:n], rb["obs"][:n])
        assert not np.array_equal(ra["action"][:n], rb["action"][:n])


def test_penalty_cases_differ_only_in_the_loss_sums():
    """Under the table policy the penalty changes no event: the two cases' records are equal, and
    their reward and cost sums differ by the penalty per dropped packet."""
    for (_, r0, c0, _), (_, r1, c1, _) in zip(_oracle_runs("penalty0", "abilene"), _oracle_runs("penalty12_5", "abilene")):
        assert r0.tobytes() == r1.tobytes()
        drops = int((r0["status"] == ST_DROPPED).sum())
        assert drops > 300 and int(c0["ov_lost"]) == int(c1["ov_lost"]) >= drops
        assert abs(float(c1["reward_sum"]) - float(c0["reward_sum"]) - 12.5 * drops) < 1e-6
        # (cost_sum is an fp32 running sum of a few thousand terms of up to 12.5)
        assert abs(float(c1["cost_sum"]) - float(c0["cost_sum"]) - 12.5 * int(c1["ov_lost"])) < 1e-3 * 12.5 * int(c1["ov_lost"])


def _refused(tp, params, msg):
    with pytest.raises(engine.PrismaError, match=r"prisma error -1: .*" + msg):
        engine.plan(tp, params)


@pytest.mark.parametrize("tname", list(P.TOPOS))
def test_plan_refuses_beyond_the_limits(tname):
    """Each PRISMA_ERR_CONFIG (-1) with its message."""
    from prisma_amd.config import engine_params
    tp = P.topo(tname)
    base = engine_params(tp, sim_time_s=P.SIM_TIME_S, seed=P.SEED)
    _refused(tp, engine_params(tp, link_delay_ms=40), "propagation delay too long")
    for ma in (0, 65):
        _refused(tp, dict(base, ma_size=ma), "bad link / ping parameters")
    for key in ("max_buffer_bytes", "packet_size", "link_bps"):
        _refused(tp, dict(base, **{key: 0}), "bad link / ping parameters")
    _refused(tp, dict(base, ping_interval_s=0.0), "bad link / ping parameters")
    _refused(tp, dict(base, link_delay_ns=-1), "bad link / ping parameters")
    for t in (0.0, 4096.0):
        _refused(tp, dict(base, sim_time_s=t), "sim_time_s must be in")
    engine.plan(tp, dict(base, sim_time_s=4095.0, ma_size=64))
    engine.plan(tp, dict(base, ma_size=1))


@pytest.mark.parametrize("tname", P.IDENTITY)
@pytest.mark.parametrize("name", P.MEMORY_REFUSED)
def test_memory_engine_refuses_more_than_16_wire_slots(name, tname):
    assert P.CASES[name]["wcap"] in (32, 64)
    _refused(P.case_topo(name, tname), P.case_params(name, tname, engine=engine.PRISMA_ENGINE_MEMORY),
             "more than 16 packets on a wire")


@pytest.mark.parametrize("name,tname", P.NO_ENGINE)
def test_widest_wire_with_echo_rings_fits_neither_engine_on_geant(name, tname):
    tp = P.case_topo(name, tname)
    s = P.sizing(P.case_params(name, tname), tp)
    # the register-resident engine's LDS image: wire slots (2 words each), rings, windows, ...
    assert 4 * (tp.n_links + tp.n_nodes) * s["WCAP"] * 2 + 4 * s["ring_entries"] > 160 * 1024
    _refused(tp, P.case_params(name, tname, engine=engine.PRISMA_ENGINE_REGISTER), "exceeds the register-resident engine")
    _refused(tp, P.case_params(name, tname), "more than 16 packets on a wire")


def test_nn_echoes_are_refused_on_unequal_overlay_degrees():
    for name in P.IDENTITY_ONLY:
        _refused(P.topo(P.TUNNELLED), P.case_params(name, P.TUNNELLED), "equal overlay")
