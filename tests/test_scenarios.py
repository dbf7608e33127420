"""Traffic scenarios on the CPU: ScenarioSet's structural check over the shipped data sets, the
refusals of prisma_plan_scenarios, the replica assignment under sharding, the host restatement of
prisma_scenario_stats' f64 order, and the oracle precondition of tests/test_gpu_scenarios.py."""
import math

import numpy as np
import pytest

from prisma_amd import dist, engine
from prisma_amd.config import engine_params
from prisma_amd.scenarios import (STATS_DTYPE, ScenarioSet, derived_stats, stats_host, stats_sum)
from prisma_amd.records import COUNTERS_DTYPE
from prisma_amd.topology import Topology, sp_next_hop_table

from scenario_util import ABILENE_4, example, scenario_set


@pytest.mark.parametrize("name,flows", [("abilene", 110), ("geant", 506), ("abilene_on_geant", 110)])
def test_shipped_data_sets_share_their_flow_list(name, flows):
    sc = ScenarioSet.grid(name, range(4), (0.5, 1.0, 2.0))
    assert len(sc) == sc.n_scenarios == 12 and sc.rates.shape == (12, flows) and sc.rates.dtype == np.uint64
    assert np.all(sc.rates > 0)
    # TM-major grid; the load factor scales the rates, the TM changes them
    assert [(t.load_factor) for t in sc.topos[:3]] == [0.5, 1.0, 2.0]
    assert np.array_equal(sc.rates[1], example(name, 0, 1.0).flow_rate_bps)
    assert not np.array_equal(sc.rates[1], sc.rates[4]) and np.all(sc.rates[2] >= sc.rates[1])
    assert len(set(sc.labels)) == 3                       # (name and load factor; the TM index is not in a Topology)


def test_set_refuses_other_flow_lists_and_topologies():
    a = example("abilene", 0, 1.0)
    tm = a.tm_strings.copy()
    i, j = int(a.flow_src[7]), int(a.flow_dst[7])
    tm[i, j] = "0"
    b = Topology.from_matrices(a.adjacency, tm, load_factor=1.0, name="abilene")
    assert b.n_flows == a.n_flows - 1
    with pytest.raises(ValueError, match="flow_src"):
        ScenarioSet([a, b])
    with pytest.raises(ValueError, match="n_nodes"):
        ScenarioSet([a, example("geant", 0, 1.0)])
    with pytest.raises(ValueError, match="flow_src"):
        ScenarioSet([example("geant", 0, 1.0), example("abilene_on_geant", 0, 1.0)])
    with pytest.raises(ValueError):
        ScenarioSet([])
    assert len(ScenarioSet([a, a])) == 2


def test_plan_scenarios_validates_and_equals_plan():
    sc = scenario_set("abilene", ABILENE_4)
    topo = sc.topos[0]
    params = engine_params(topo)
    one = engine.plan(topo, params)
    # S = 1 on the topology's own rates: what prisma_plan says, and one image
    p1 = engine.plan(topo, params, scenarios=ScenarioSet([topo]), n_replicas=3)
    assert {k: p1[k] for k in one} == one
    assert p1["n_scenarios"] == 1 and p1["topo_bytes"] == p1["image_bytes"] > 0
    # S = 4: the same per-replica footprint, four images (each rounded up to 256 B)
    p4 = engine.plan(topo, params, scenarios=sc, scenario_of=[0, 1, 2, 3, 1, 0], n_replicas=6)
    assert {k: p4[k] for k in one} == one
    assert p4["n_scenarios"] == 4 and p4["image_bytes"] == p1["image_bytes"]
    assert p4["topo_bytes"] == 4 * ((p1["image_bytes"] + 255) // 256 * 256)
    # ... on the memory-resident engine too
    pm = engine.plan(topo, dict(params, engine=engine.PRISMA_ENGINE_MEMORY), scenarios=sc, n_replicas=4)
    assert pm["engine"] == engine.PRISMA_ENGINE_MEMORY and pm["topo_bytes"] >= 4 * pm["image_bytes"]
    # the default assignment at this layer is round robin by global id too
    sc_d, keep_d = engine._scenarios_struct(sc, None, 3, topo.n_flows, replica_base=5)
    assert keep_d[1].tolist() == sc.assign(3, replica_base=5).tolist() == [1, 2, 3]
    # refusals, naming the argument
    rates = sc.rates.copy()
    rates[2, 17] = 0
    with pytest.raises(engine.PrismaError, match=r"error -1: flow_rate_bps: zero rate of flow 17 in scenario 2"):
        engine.plan(topo, params, scenarios=rates, n_replicas=4)
    with pytest.raises(engine.PrismaError, match=r"error -1: scenario_of\[2\] = 4 "):
        engine.plan(topo, params, scenarios=sc, scenario_of=[0, 1, 4], n_replicas=3)
    with pytest.raises(engine.PrismaError, match=r"error -1: scenario_of\[0\] = -1 "):
        engine.plan(topo, params, scenarios=sc, scenario_of=[-1, 1, 2], n_replicas=3)
    with pytest.raises(engine.PrismaError, match=r"error -5: .*n_scenarios"):
        engine.plan(topo, params, scenarios=np.zeros((0, topo.n_flows), dtype=np.uint64), scenario_of=[0], n_replicas=1)
    # null pointers straight at the C entry point
    import ctypes as C
    lib = engine.load_library()
    t, keep = engine._topo_struct(topo)
    p = engine._params_struct(params)
    out = engine._Plan()
    assert lib.prisma_plan_scenarios(C.byref(t), C.byref(p), None, 1, C.byref(out)) == -5
    assert b"scenarios" in lib.prisma_last_error()
    so = np.zeros(1, dtype=np.int32)
    s = engine._Scenarios(1, None, so.ctypes.data)
    assert lib.prisma_plan_scenarios(C.byref(t), C.byref(p), C.byref(s), 1, C.byref(out)) == -5
    s = engine._Scenarios(1, sc.rates.ctypes.data, None)
    assert lib.prisma_plan_scenarios(C.byref(t), C.byref(p), C.byref(s), 1, C.byref(out)) == -5
    assert b"scenario_of" in lib.prisma_last_error()
    s = engine._Scenarios(65536, sc.rates.ctypes.data, so.ctypes.data)
    assert lib.prisma_plan_scenarios(C.byref(t), C.byref(p), C.byref(s), 1, C.byref(out)) == -1
    assert b"PRISMA_MAX_SCENARIOS" in lib.prisma_last_error()
    # with a set the topology's own rates are not read, but must be there
    t.flow_rate_bps = None
    s = engine._Scenarios(4, sc.rates.ctypes.data, so.ctypes.data)
    assert lib.prisma_plan_scenarios(C.byref(t), C.byref(p), C.byref(s), 1, C.byref(out)) == -5
    import dataclasses                                               # all-zero topology rates: not read
    t2, keep2 = engine._topo_struct(dataclasses.replace(topo, flow_rate_bps=np.zeros_like(topo.flow_rate_bps)))
    assert lib.prisma_plan_scenarios(C.byref(t2), C.byref(p), C.byref(s), 1, C.byref(out)) == 0
    assert lib.prisma_plan(C.byref(t2), C.byref(p), C.byref(out)) == -1


def test_assign_is_a_function_of_the_global_id():
    sc = scenario_set("abilene", ABILENE_4)
    for how, kw in (("round_robin", {}), ("blocks", {"n_total": 6})):
        whole = sc.assign(6, how=how, **kw)
        assert whole.dtype == np.int32 and whole.shape == (6,)
        assert whole.min() == 0 and whole.max() <= 3
        for k in range(2):
            base, n = dist.shard(6, k, 2)
            assert np.array_equal(sc.assign(n, how=how, replica_base=base, **kw), whole[base:base + n]), (how, k)
    assert sc.assign(6).tolist() == [0, 1, 2, 3, 0, 1]
    assert sc.assign(8, how="blocks").tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert sc.assign(3, replica_base=5).tolist() == [1, 2, 3]
    with pytest.raises(ValueError):
        sc.assign(4, how="random")


def _plain(x):
    a = 0.0
    for v in x:
        a = a + float(v)
    return a


def test_stats_order_on_adversarial_doubles():
    # one lane's column: 1e16, 1, -1e16 at positions 0, 64, 128 -- the lane adds them in turn, so the
    # 1 is absorbed; plain ascending summation over the whole array sees other values in between
    x = np.zeros(130)
    x[0], x[64], x[128] = 1e16, 1.0, -1e16
    x[1] = 3.0
    assert stats_sum(x) == 3.0                         # lane 0: (1e16 + 1) - 1e16 = 0; lane 1: 3
    assert _plain(x) == 4.0 and math.fsum(x) == 4.0    # ascending: 1e16 + 3 = 1e16 + 4 (tie to even), + 1 absorbed ...
    assert stats_sum(x) != _plain(x)
    # the fold pairs lane l with l + 32, then 16, ...: 1e16 in lane 0 and -1e16 in lane 32 cancel first
    y = np.zeros(64)
    y[0], y[32], y[1] = 1e16, -1e16, 1.0
    assert stats_sum(y) == 1.0 and _plain(y) == 0.0
    # reproducible, and a permutation within the order changes it
    rng = np.random.default_rng(3)
    z = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 9, 1000)
    assert stats_sum(z) == stats_sum(z.copy()) == stats_sum(list(z))
    assert stats_sum([]) == 0.0 and stats_sum([2.5]) == 2.5 and stats_sum(np.arange(65.0)) == 2080.0
    # counter-like data: within 1e-12 relative of the exact sum
    for n in (1, 63, 64, 65, 130, 4096):
        c = rng.random(n) * 50.0 + rng.integers(0, 2000, n)
        assert abs(stats_sum(c) - math.fsum(c)) <= 1e-12 * abs(math.fsum(c)), n
        f = (rng.random(n) * 3.0).astype(np.float32)
        assert abs(stats_sum(f) - math.fsum(f.astype(np.float64))) <= 1e-12 * math.fsum(f.astype(np.float64)), n


def test_stats_host_and_derived():
    rng = np.random.default_rng(8)
    cnt = np.zeros(10, dtype=COUNTERS_DTYPE)
    for k in ("events", "hops", "now_ns", "ov_injected", "ov_lost", "e2e_n", "cost_n", "dec_count"):
        cnt[k] = rng.integers(1, 1000, 10)
    cnt["reward_sum"] = rng.random(10)
    cnt["e2e_sum"] = rng.random(10).astype(np.float32)
    cnt["cost_sum"] = rng.random(10).astype(np.float32)
    cnt["error"][3] = 16
    cnt["episode_over"][[3, 4]] = 1
    so = np.array([0, 1, 1, 1, 0, 1, 1, 1, 1, 1])
    st = stats_host(cnt, so, 3)
    assert st.dtype == STATS_DTYPE and st["n_replicas"].tolist() == [2, 8, 0]
    assert st["n_error"].tolist() == [0, 1, 0] and st["n_over"].tolist() == [1, 1, 0]
    assert int(st["hops"][1]) == int(cnt["hops"][so == 1].sum()) and int(st["now_ns"][0]) == int(cnt["now_ns"][[0, 4]].sum())
    assert st["reward_sum"][0] == cnt["reward_sum"][0] + cnt["reward_sum"][4]
    d = derived_stats(st)
    assert d["avg_e2e_delay"][0] == st["e2e_sum"][0] / st["e2e_n"][0]
    assert d["loss_ratio"][1] == st["ov_lost"][1] / st["ov_injected"][1]
    assert np.isnan(d["avg_cost"][2])


def test_gpu_case_scenarios_differ_from_record_0(oracle_mod):
    """The precondition of tests/test_gpu_scenarios.py: under the SP table, replica 5 of each of the
    Abilene scenarios (tm1, 0.5), (tm2, 2.0), (tm3, 1.5) differs from scenario (tm0, 1.0) already in
    decision record 0, and none carries an error bit after 3 000 hops -- so a kernel that ignores
    scenario_of (or binds another scenario's image) cannot pass."""
    sc = scenario_set("abilene", ABILENE_4)
    params = engine_params(sc.topos[0], replica_base=5)
    table = sp_next_hop_table(sc.topos[0])
    recs, cnts = [], []
    for t in sc.topos:
        o = oracle_mod.OracleSim(t, params, replica=5)
        assert o.run_table(table, 3000) == 3000
        recs.append(o.records().copy())
        cnts.append(o.counters().copy())
        o.close()
    assert all(int(c["error"]) == 0 and int(c["episode_over"]) == 0 for c in cnts)
    for s in (1, 2, 3):
        assert recs[s][0].tobytes() != recs[0][0].tobytes(), s
    # the loads show: (tm1, 0.5) loses nothing and runs longest, (tm2, 2.0) loses most in the shortest time
    lost = [int(c["ov_lost"]) for c in cnts]
    now = [int(c["now_ns"]) for c in cnts]
    assert lost == [22, 0, 206, 115]
    assert [round(t / 1e9, 2) for t in now] == [2.03, 3.82, 1.34, 1.60]
    assert lost[1] == 0 < lost[0] < lost[3] < lost[2] and now[2] < now[3] < now[0] < now[1]
