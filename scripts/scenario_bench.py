"""Mixed-load run: BASELINE config 4's shape per GPU -- GEANT, the in-kernel DQN-buffer model, 2 048
replicas, 8 192 hops per launch -- with its seven load factors round-robin in ONE env (a scenario
set, prisma_create_scenarios) against the same seven as single-scenario envs of 2 048 replicas each.
Reports total hops / total time for both, checks two replicas of the mixed env against the CPU
oracle on their own scenarios' topologies, and times prisma_scenario_stats at R = 4 096, S = 28
against reading counters() to the host.  One JSON line per measurement.  Reads nothing outside the
repository.

Usage: python scripts/scenario_bench.py [--replicas 2048] [--hops 8192] [--steps 5] [--warmup 2]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prisma_amd.config import engine_params  # noqa: E402
from prisma_amd.engine import PrismaEngine  # noqa: E402
from prisma_amd.policies import StackedQNet  # noqa: E402
from prisma_amd.scenarios import ScenarioSet  # noqa: E402
from prisma_amd.topology import Topology, sp_next_hop_table  # noqa: E402

LOAD_FACTORS = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0)


def timed_launches(eng, weights, hops, steps, warmup):
    """Seconds of `steps` launches (a host clock around work that ends in a device synchronise) and
    the hops they executed."""
    for _ in range(warmup):
        eng.run(weights, hops)
    torch.cuda.synchronize()
    h0 = int(eng.counters()["hops_total"].sum())
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.run(weights, hops)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cnt = eng.counters()
    assert np.all(cnt["error"] == 0), "a replica stopped on an error bit"
    return dt, int(cnt["hops_total"].sum()) - h0, cnt


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=2048)
    ap.add_argument("--hops", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-hops", type=int, default=2000, help="hops of the oracle check (0: skip)")
    a = ap.parse_args(argv)
    R, H = a.replicas, a.hops
    sc = ScenarioSet.grid("geant", [0], LOAD_FACTORS)
    topo = sc.topos[0]
    kw = dict(sim_time_s=60.0, ping_as_obs=0, log_capacity=8192)
    weights = StackedQNet(topo, "buffer", seed=0).pack()

    # ---- the seven load factors in one env, round robin
    params = engine_params(topo, **kw)
    so = sc.assign(R)
    eng = PrismaEngine(topo, params, R, scenarios=sc, scenario_of=so)
    eng.reset(0)
    dt_mixed, hops_mixed, cnt = timed_launches(eng, weights, H, a.steps, a.warmup)
    per = {f"{lf:g}": int(cnt["hops_total"][so == s].sum()) for s, lf in enumerate(LOAD_FACTORS)}
    eng.close()
    print(json.dumps(dict(metric="mixed_env_hops_per_s", value=hops_mixed / dt_mixed, seconds=dt_mixed, hops=hops_mixed,
                          replicas=R, hops_per_launch=H, steps=a.steps, scenarios=len(sc),
                          hops_total_by_load_factor=per)), flush=True)

    # ---- the same seven as single-scenario envs of R replicas each
    dt_single = hops_single = 0
    lines = {}
    for s, lf in enumerate(LOAD_FACTORS):
        t = sc.topos[s]
        e1 = PrismaEngine(t, engine_params(t, **kw), R)
        e1.reset(0)
        dt, hp, _ = timed_launches(e1, weights, H, a.steps, a.warmup)
        e1.close()
        dt_single += dt
        hops_single += hp
        lines[f"{lf:g}"] = hp / dt
    print(json.dumps(dict(metric="single_envs_hops_per_s", value=hops_single / dt_single, seconds=dt_single,
                          hops=hops_single, replicas=R, envs=len(LOAD_FACTORS), hops_per_s_by_load_factor=lines)),
          flush=True)
    print(json.dumps(dict(metric="mixed_over_single", value=(hops_mixed / dt_mixed) / (hops_single / dt_single))),
          flush=True)

    # ---- two replicas of a mixed env against the oracle on their own scenario's topology
    if a.check_hops:
        import oracle as O
        from scenario_util import run_scenarios_both
        O.build()
        p2 = engine_params(topo, replica_base=3, **kw)
        so2 = sc.assign(16, replica_base=3)
        picks = [1, 6]                               # two scenarios: load factors 1.5 and 1.0
        run_scenarios_both(O, sc, so2, p2, a.check_hops, ("mlp", weights.cpu().numpy()), launches=2,
                           label="scenario_bench", replicas=picks)
        print(json.dumps(dict(metric="oracle_check", value=1, replicas=picks,
                              load_factors=[LOAD_FACTORS[int(so2[r])] for r in picks], hops=2 * a.check_hops)),
              flush=True)

    # ---- prisma_scenario_stats against counters() read to the host, R = 4 096, S = 28
    ab = ScenarioSet.grid("abilene", range(4), LOAD_FACTORS)
    t0_ = ab.topos[0]
    eng = PrismaEngine(t0_, engine_params(t0_), 4096, scenarios=ab, scenario_of=ab.assign(4096))
    eng.reset(0)
    eng.run(torch.from_numpy(sp_next_hop_table(t0_)).cuda(), 500)
    eng.scenario_stats()
    torch.cuda.synchronize()
    n = 200
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        eng.scenario_stats()
    ev1.record()
    torch.cuda.synchronize()
    stats_us = ev0.elapsed_time(ev1) * 1e3 / n
    t0 = time.perf_counter()
    for _ in range(n):
        eng.counters()
    read_us = (time.perf_counter() - t0) * 1e6 / n
    t0 = time.perf_counter()
    for _ in range(n):
        st = eng.scenario_stats().cpu()
    stats_read_us = (time.perf_counter() - t0) * 1e6 / n
    eng.close()
    print(json.dumps(dict(metric="scenario_stats_us", value=stats_us, replicas=4096, scenarios=len(ab),
                          stats_to_host_us=stats_read_us, counters_to_host_us=read_us,
                          bytes_stats=int(st.numel()), bytes_counters=4096 * 152)), flush=True)


if __name__ == "__main__":
    main()
