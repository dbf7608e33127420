#!/usr/bin/env python
"""Fused-run throughput of in-kernel stochastic multipath routing (prisma_run_stochastic, the
reference's "opt" agent) beside the SP-table run() at the headline shape: 4 096 Abilene replicas,
pingAsObs 1, 60-s episodes with auto-reset, a log of 8 192 records, 32 768 hops per launch, the
equal split over shortest-path next hops (optrouting.ecmp_routing) as the routing matrix.

One JSON line per measurement, measured like bench.py: --warmup untimed launches, then --steps
timed ones between device synchronisations; hops/s from the hops_total counters.  The order is
sp, opt, sp, opt, sp in one session, so the SP lines' spread shows the run-to-run noise the ratio
carries.  The two policies route differently, so their traffic differs: events_per_hop is printed
to show by how much.  bench.py stays the yardstick of the headline.

    python scripts/opt_bench.py [--out profiles/opt_policy/opt_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prisma_amd import optrouting  # noqa: E402
from prisma_amd.config import engine_params  # noqa: E402
from prisma_amd.engine import PrismaEngine, build_id  # noqa: E402
from prisma_amd.topology import Topology, sp_next_hop_table  # noqa: E402


def measure(policy, args):
    topo = Topology.example(args.topology, 0, 1.0)
    params = engine_params(topo, sim_time_s=60.0, ping_as_obs=1, auto_reset=1, seed=100, log_capacity=8192)
    eng = PrismaEngine(topo, params, args.replicas)
    if policy == "sp":
        data = torch.from_numpy(sp_next_hop_table(topo)).cuda()
        launch = lambda: eng.run(data, args.hops)
        kernel = eng.kernel_name
    else:
        data = eng.stochastic_table(optrouting.ecmp_routing(topo))
        launch = lambda: eng.run_stochastic(data, args.hops)
        ki = eng.kernel_info()
        kernel = (f"prisma_step_kernel_stoch_t<{ki['flow_slots']}, {ki['link_slots']}, "
                  f"{'true' if ki['tunnels'] else 'false'}, false>")
    eng.reset(0)
    for _ in range(args.warmup):
        launch()
    torch.cuda.synchronize()
    c0 = eng.counters()
    h0, e0 = int(c0["hops_total"].sum()), int(c0["events_total"].sum())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        launch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cnt = eng.counters()
    hops = int(cnt["hops_total"].sum()) - h0
    events = int(cnt["events_total"].sum()) - e0
    out = {"policy": policy, "routing": None if policy == "sp" else "ecmp", "topology": args.topology,
           "replicas": args.replicas, "hops_per_launch": args.hops, "steps": args.steps, "warmup": args.warmup,
           "wall_s": round(dt, 4), "hops_per_s": round(hops / dt, 1), "events_per_hop": round(events / max(hops, 1), 4),
           "events_per_s": round(events / dt, 1), "errors": int(cnt["error"].max()), "build_id": build_id(),
           "kernel": kernel, "device": torch.cuda.get_device_name(0)}
    eng.close()
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--topology", default="abilene")
    p.add_argument("--replicas", type=int, default=4096)
    p.add_argument("--hops", type=int, default=32768, help="hops per replica per launch")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--order", default="sp,opt,sp,opt,sp")
    p.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = p.parse_args(argv)
    for policy in args.order.split(","):
        line = json.dumps(measure(policy, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
