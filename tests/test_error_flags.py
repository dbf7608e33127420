"""The engine's defined failures (include/prisma.h PRISMA_EBIT_LOGWRAP and _PINGIDX), without a
GPU: the premises the GPU tests of tests/test_gpu_error_flags.py stand on, computed from the
oracle's own runs, the oracle's restatement of the two failures, and the log_capacity range of
both validators.  Every number is computed; nothing here is a recorded figure."""
import functools

import numpy as np
import pytest

import parity_util as P
import synth_topology as S
from prisma_amd import engine
from prisma_amd.config import engine_params
from prisma_amd.records import EBIT_LOGWRAP, EBIT_PINGIDX, ST_DROPPED, ST_ENQUEUED
from prisma_amd.topology import Topology, sp_next_hop_table

ALL = {**P.WRAP_SCENARIOS, **P.WRAP_CONTROLS}


@functools.lru_cache(maxsize=None)
def _runs(name, cap):
    """The scenario's table run of `hops` hops on replicas 5, 6, 7 at a log capacity:
    (hops executed, records, counters) each."""
    import oracle as O
    O.build()
    sc = ALL[name]
    topo, params, table = P.wrap_case(sc, cap)
    out = []
    for r in range(P.WRAP_R):
        o = O.OracleSim(topo, params, replica=P.WRAP_BASE + r)
        got = o.run_table(table, sc["hops"])
        rec, cnt = o.records(), o.counters()
        if int(cnt["error"]):                                  # a failed oracle stays stopped
            assert o.run_table(table, 100) == 0
            assert o.records().tobytes() == rec.tobytes() and o.counters().tobytes() == cnt.tobytes()
        out.append((got, rec, cnt))
        o.close()
    return out


@pytest.mark.parametrize("name", list(P.WRAP_SCENARIOS))
def test_age_premises(name):
    sc = P.WRAP_SCENARIOS[name]
    stars = []
    for got, rec, cnt in _runs(name, P.BIG_LOG):
        assert got == sc["hops"] and int(cnt["error"]) == 0 and len(rec) <= P.BIG_LOG
        d = P.first_wrap(rec, P.WRAP_CAP)
        assert d is not None and d < 0.75 * len(rec), (name, d, len(rec))
        if sc["clean"]:
            assert int(P.record_ages(rec).max()) < P.CLEAN_CAP, name
        else:
            assert P.first_wrap(rec, P.CLEAN_CAP) is not None
        stars.append(d)
    assert len(set(stars)) == P.WRAP_R, (name, stars)          # three replicas, three failure points
    # the GPU run: 1.5 x the hops to the failure, within WRAP_MAX_HOPS per replica
    assert 1.5 * max(got for got, _, _ in _runs(name, P.WRAP_CAP)) <= P.WRAP_MAX_HOPS


@pytest.mark.parametrize("name", list(P.WRAP_CONTROLS))
def test_controls_never_reach_the_capacity(name):
    for cap in (P.BIG_LOG, P.WRAP_CAP):
        for got, rec, cnt in _runs(name, cap):
            assert got == ALL[name]["hops"] and int(cnt["error"]) == 0 and int(cnt["episode_over"]) == 0
            assert int(P.record_ages(rec).max()) < P.WRAP_CAP and P.first_wrap(rec, P.WRAP_CAP) is None
    assert all(a[1].tobytes() == b[1].tobytes() for a, b in zip(_runs(name, P.BIG_LOG), _runs(name, P.WRAP_CAP)))


def test_a_first_offending_age_equals_the_capacity():
    """The check is `age >= log_capacity`: a scenario whose first offending age is log_capacity
    itself tells it from `>` (an identity one, and one with the --train paths)."""
    exact = [(name, r) for name in P.WRAP_SCENARIOS for r, (_, rec, _) in enumerate(_runs(name, P.BIG_LOG))
             if P.record_ages(rec)[P.first_wrap(rec, P.WRAP_CAP)] == P.WRAP_CAP]
    assert ("abilene_lf3", 2) in exact and ("abilene_lf3_train", 1) in exact, exact


@pytest.mark.parametrize("name,want", [("abilene_on_geant_lf3_s129", [0, 2]),
                                       ("abilene_on_geant_lf3_s130_train", [0])])
def test_the_check_inside_a_tunnel_fires_first_somewhere(name, want):
    """Without the check at the switches inside a tunnel the same run would stop later, at the
    tunnel's end: a scenario where the oracle stops before d* and before that record's time tells
    an engine without it from one with it -- one for the instances without the ctrl paths (18-bit
    relay entries), one with --train for those with them (22-bit)."""
    early = [r for r, ((_, big, _), (_, rec, cnt)) in enumerate(zip(_runs(name, P.BIG_LOG), _runs(name, P.WRAP_CAP)))
             if len(rec) < P.first_wrap(big, P.WRAP_CAP)
             and int(cnt["now_ns"]) < int(big[P.first_wrap(big, P.WRAP_CAP)]["t_ns"])]
    assert early == want, early


def _same_but_later_drops(short, long):
    """Byte equality, but for records the longer run has marked DROPPED since: inside a tunnel a
    packet is dropped after its decision, which the run that stopped earlier may not have seen."""
    later = (short["status"] == ST_ENQUEUED) & (long["status"] == ST_DROPPED)
    fixed = short.copy()
    fixed["status"][later] = ST_DROPPED
    return fixed.tobytes() == long.tobytes()


@pytest.mark.parametrize("name", list(P.WRAP_SCENARIOS))
def test_oracle_flags_the_wrap(name):
    sc = P.WRAP_SCENARIOS[name]
    identity = Topology.example(sc["topo"], 0, sc["lf"]).identity
    for (_, big, _), (got, rec, cnt), (got2, rec2, cnt2) in zip(_runs(name, P.BIG_LOG), _runs(name, P.WRAP_CAP),
                                                                 _runs(name, P.CLEAN_CAP)):
        d = P.first_wrap(big, P.WRAP_CAP)
        assert int(cnt["error"]) == EBIT_LOGWRAP and int(cnt["episode_over"]) == 1, (name, cnt)
        n = int(cnt["dec_count"])
        assert n == len(rec) and got == int(cnt["hops"]) == int(cnt["hops_total"]) < sc["hops"]
        assert P.first_wrap(rec, P.WRAP_CAP) is None               # the refused record is not written
        if identity:
            assert n == d, (name, n, d)
            assert rec.tobytes() == big[:n].tobytes()
        else:
            # (the check inside a tunnel can fire before the packet arrives -- or is dropped)
            # (at or before d* + 1 is what the run needs; d* itself follows from the records: every
            # record before the stop has an age below the capacity, so d* cannot lie before it)
            assert n <= d, (name, n, d)
            assert _same_but_later_drops(rec, big[:n]), name
        if sc["clean"]:
            assert int(cnt2["error"]) == 0 and int(cnt2["episode_over"]) == 0 and got2 == sc["hops"]
            assert rec2.tobytes() == big.tobytes()
        else:
            assert int(cnt2["error"]) == EBIT_LOGWRAP and len(rec2) == P.first_wrap(big, P.CLEAN_CAP)


def test_dqn_buffer_scenario_premises():
    import oracle as O
    O.build()
    topo, params, w = P.wrap_mlp_case(P.BIG_LOG)
    _, small, _ = P.wrap_mlp_case(P.WRAP_CAP)
    stars = []
    for r in range(P.WRAP_R):
        o = O.OracleSim(topo, params, replica=P.WRAP_BASE + r)
        o.run_mlp(w, P.WRAP_MLP_HOPS)
        rec = o.records()
        d = P.first_wrap(rec, P.WRAP_CAP)
        assert d is not None and d < 0.75 * len(rec) and int(P.record_ages(rec).max()) < P.CLEAN_CAP
        f = O.OracleSim(topo, small, replica=P.WRAP_BASE + r)
        got = f.run_mlp(w, P.WRAP_MLP_HOPS)
        c = f.counters()
        assert int(c["error"]) == EBIT_LOGWRAP and int(c["dec_count"]) == d and 1.5 * got <= P.WRAP_MAX_HOPS
        assert f.records().tobytes() == rec[:d].tobytes()
        stars.append(d)
    assert len(set(stars)) == P.WRAP_R


# ---- PRISMA_EBIT_PINGIDX ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inner_runs(name):
    import oracle as O
    O.build()
    topo = S.build_error(name)
    params = S.error_params(name, ping_as_obs=1)
    out = []
    for r in range(S.R):
        o = O.OracleSim(topo, params, replica=S.REPLICA_BASE + r)
        got = o.run_table(sp_next_hop_table(topo), S.H)
        out.append((got, o.records(), o.counters()))
        o.close()
    return out


@pytest.mark.parametrize("name", list(S.ERROR_CASES))
def test_oracle_flags_the_ping_index(name):
    topo = S.build_error(name)
    assert not topo.identity
    for got, rec, cnt in _inner_runs(name):
        assert int(cnt["error"]) == EBIT_PINGIDX and int(cnt["episode_over"]) == 1, (name, cnt)
        assert got < S.H and 0 < len(rec) == int(cnt["dec_count"]) < 100
        # within the second ping round (pings every 0.2 s)
        assert 0.2e9 <= int(cnt["now_ns"]) < 0.4e9 and int(cnt["ping_rounds"]) >= 1


def test_memory_engine_cannot_meet_the_ping_index():
    """The memory-resident engine refuses tunnelled overlays, and on an identity overlay a
    ping-back's tunnel is the link it acknowledges: its PINGIDX branch has no input."""
    for name in S.ERROR_CASES:
        with pytest.raises(engine.PrismaError, match="identity overlays only"):
            engine.plan(S.build_error(name), S.error_params(name, engine=engine.PRISMA_ENGINE_MEMORY))
        assert engine.plan(S.build_error(name), S.error_params(name))["engine"] == engine.PRISMA_ENGINE_REGISTER


def test_leaf_first_cases_never_flag_the_ping_index():
    from test_instance_matrix import _oracle_runs
    for name in S.TUNNELLED:
        for train in (0, 1):
            for got, _, cnt in _oracle_runs(name, train):
                assert int(cnt["error"]) == 0 and got == S.H
    # and the builder's default is the leaf-first order
    for name, (args, seed, rate) in S.ERROR_CASES.items():
        leaf = S.tunnelled(*args, seed, rate)
        inner = S.build_error(name)
        assert not np.array_equal(leaf.overlay_nodes, inner.overlay_nodes)


# ---- log_capacity: [1024, 2^21] in both validators ---------------------------------------------
def test_log_capacity_range():
    ab = Topology.example("abilene")
    with pytest.raises(ValueError, match=r"2\^21"):
        engine_params(ab, log_capacity=1 << 22)
    with pytest.raises(engine.PrismaError, match=r"log_capacity.*2\^21"):
        engine.plan(ab, dict(engine_params(ab), log_capacity=1 << 22))
    for topo in (ab, Topology.example("overlay_full_mesh_3n_abilene")):
        p = engine.plan(topo, engine_params(topo, log_capacity=1 << 21))
        assert p["engine"] == engine.PRISMA_ENGINE_REGISTER
