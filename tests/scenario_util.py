"""Shared machinery of the scenario tests (tests/test_scenarios.py, tests/test_gpu_scenarios.py) and
of scripts/scenario_bench.py: an env whose replicas run different traffic scenarios against one CPU
oracle per replica ON ITS OWN SCENARIO'S TOPOLOGY -- parity_util.run_fused_both / compare_steady with
a topology per replica, built on OracleSim, OracleChain and explore_util.SteppedOracle.  The oracle
is unchanged: replica r is OracleSim(topology of scenario_of[r], params, global replica id)."""
from __future__ import annotations

import functools

import numpy as np

from parity_util import OracleChain, assert_counters_equal, check_near_ties, first_difference


@functools.lru_cache(maxsize=None)
def example(name, tm, lf):
    from prisma_amd.topology import Topology
    return Topology.example(name, tm, lf)


def scenario_set(name, pairs):
    """ScenarioSet of (tm index, load factor) pairs of a shipped data set."""
    from prisma_amd.scenarios import ScenarioSet
    return ScenarioSet([example(name, tm, lf) for tm, lf in pairs])


# the four Abilene scenarios of the GPU cases (precondition: tests/test_scenarios.py)
ABILENE_4 = ((0, 1.0), (1, 0.5), (2, 2.0), (3, 1.5))


def compare_launch(eng, chains, checked, prev_hops, hops, *, label="", launch=0, net_cpu=None, pol=None):
    """After one fused launch of `hops` hops: every new record and the counters of every replica in
    `chains` ({local replica: OracleChain}) byte for byte.  checked / prev_hops: per-replica progress,
    updated in place.  Returns the counters."""
    import torch
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    for r, ch in chains.items():
        c = cnt[r]
        assert int(c["error"]) == 0, (label, launch, r, int(c["error"]))
        delta = int(c["hops_total"]) - prev_hops[r]
        prev_hops[r] = int(c["hops_total"])
        assert 0 <= delta <= hops, (label, launch, r, delta)
        got = ch.advance(delta)
        assert got == delta, (label, launch, r, got, delta)
        ch.sync_episode(int(c["episode"]))
        total = int(c["dec_count"])
        first, new = checked[r], total - checked[r]
        assert new <= eng.log_capacity, (label, "a launch wrote more records than the log holds")
        ref = ch.records(first, new)
        assert len(ref) == new, (label, launch, r, len(ref), new)
        got_rec = eng.records(r, first, new, log_host=log)
        bad = first_difference(got_rec, ref)
        assert bad is None, (f"{label} replica {r} launch {launch}: record {first + bad} differs\n engine "
                             f"{got_rec[bad]}\n oracle {ref[bad]}")
        if net_cpu is not None:
            check_near_ties(net_cpu, pol, ch.o, got_rec)
        checked[r] = total
        assert_counters_equal(c, ch.counters(), r, f" ({label}, launch {launch})")
        assert int(c["hops_total"]) == ch.hops_total, (label, launch, r)
        assert int(c["events_total"]) == ch.events_done + int(ch.o.counters()["events"]), (label, launch, r)
    return cnt


def run_scenarios_both(oracle_mod, scen, scenario_of, params, H, policy, *, launches=1, net_cpu=None, label="",
                       kernel=None, kernel_name=None, replicas=None, eng=None):
    """R = len(scenario_of) replicas, `launches` fused launches of H hops each of a policy ("table",
    uint8 [N, N]) or ("mlp", packed fp32 numpy) on an engine with the scenario set `scen`; after EVERY
    launch every new record and the counters of each checked replica equal an OracleChain on that
    replica's own scenario topology (auto_reset: across episode ends).  kernel / kernel_name as
    parity_util.run_fused_both.  eng: an engine already made and reset (else one is made here and
    closed).  Returns (last counters, chains)."""
    import torch
    from prisma_amd.engine import PrismaEngine
    kind, pol = policy
    scenario_of = np.asarray(scenario_of, dtype=np.int32)
    R = len(scenario_of)
    own = eng is None
    if own:
        eng = PrismaEngine(scen.topos[0], params, R, scenarios=scen, scenario_of=scenario_of)
    try:
        assert eng.n_scenarios == len(scen) and np.array_equal(eng.scenario_of_host, scenario_of)
        if kernel is not None:
            ki = eng.kernel_info()
            assert {k: ki[k] for k in kernel} == kernel, (label, ki)
        if kernel_name is not None:
            name = eng.kernel_name if kind == "table" else eng.kernel_name_mlp
            assert name.startswith(kernel_name), (label, name)
        if own:
            eng.reset(0)
        picks = list(range(R)) if replicas is None else list(replicas)
        chains = {r: OracleChain(oracle_mod, scen.topos[int(scenario_of[r])], params, params["replica_base"] + r,
                                 policy) for r in picks}
        checked = {r: 0 for r in picks}
        prev_hops = {r: 0 for r in picks}
        dev = torch.from_numpy(np.ascontiguousarray(pol)).cuda()
        cnt = None
        for launch in range(launches):
            eng.run(dev, H)
            cnt = compare_launch(eng, chains, checked, prev_hops, H, label=label, launch=launch,
                                 net_cpu=net_cpu if kind == "mlp" else None, pol=pol)
    finally:
        if own:
            eng.close()
    return cnt, chains


def run_explore_both(oracle_mod, scen, scenario_of, params, H, launches, eps, table, label=""):
    """Exploring fused launches (prisma_run_explore) on a scenario env against one
    explore_util.SteppedOracle per replica on its own scenario's topology.  A stepped oracle stops at
    pending decisions, not at a hop count, so after every launch the comparison is: the engine made
    exactly launch * H hops, and every record it has written equals the oracle's record of that index
    once the oracle has decided that many (all of them final on both sides)."""
    import torch
    from explore_util import SteppedOracle
    from prisma_amd import explore
    from prisma_amd.engine import PrismaEngine
    scenario_of = np.asarray(scenario_of, dtype=np.int32)
    R = len(scenario_of)
    thr = explore.thresholds(np.full(scen.topos[0].n_nodes, eps))
    refs = [SteppedOracle(oracle_mod, scen.topos[int(scenario_of[r])], params, params["replica_base"] + r, thr,
                          ("table", table)) for r in range(R)]
    eng = PrismaEngine(scen.topos[0], params, R, scenarios=scen, scenario_of=scenario_of)
    try:
        eng.reset(0)
        dev = torch.from_numpy(table).cuda()
        for launch in range(launches):
            eng.run(dev, H, explore=eps)
            torch.cuda.synchronize()
            cnt = eng.counters()
            log = eng.log_tensor().cpu().numpy()
            for r, ref in enumerate(refs):
                c = cnt[r]
                assert int(c["error"]) == 0 and int(c["episode_over"]) == 0, (label, launch, r)
                assert int(c["hops_total"]) == (launch + 1) * H, (label, launch, r, int(c["hops_total"]))
                n = int(c["dec_count"])
                ref.run(until_records=n)
                want = ref.records(0, n)
                got = eng.records(r, 0, n, log_host=log)
                bad = first_difference(got, want)
                assert bad is None, (f"{label} replica {r} launch {launch}: record {bad} differs\n engine "
                                     f"{got[bad]}\n oracle {want[bad]}")
        assert all(ref.explored > 10 and ref.changed > 3 for ref in refs), [(f.explored, f.changed) for f in refs]
    finally:
        eng.close()
    return refs
