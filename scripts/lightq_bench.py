#!/usr/bin/env python
"""Fused-run throughput of the in-kernel DQN-buffer family: the 64-wide model against the reduced
ones (buffer_lite, buffer_lighter, buffer_lighter_2, buffer_lighter_3) at bench.py's config 3 and
config 4 shapes (abilene_on_geant, 4 096 replicas, pingAsObs 1; geant, 2 048 replicas, pingAsObs
0, load factor 1.0; 8 192 hops per launch, a log of 8 192 records, 60-s episodes with auto-reset).

One JSON line per (shape, model), measured like bench.py: --warmup untimed launches, then --steps
timed ones between device synchronisations; hops/s from the hops_total counters.  "buffer" is
measured three times per shape (first, in the middle, last), so its spread shows the run-to-run
noise the other figures carry.  bench.py stays the yardstick of the headline; this script only
compares the models with each other.

The models are different policies, so their greedy runs are different workloads (path lengths,
drops, events per hop).  Each model is therefore measured a second time under equal traffic:
prisma_run_explore with epsilon 1 at every node ("traffic": "uniform") -- the kernel still
evaluates the model at every decision, the uniform pick replaces its action, and every model then
simulates the same packets, event for event (events_per_hop is printed to show it).

    python scripts/lightq_bench.py [--shapes config3,config4] [--models buffer,buffer_lite,...]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prisma_amd.config import engine_params  # noqa: E402
from prisma_amd.engine import PrismaEngine, build_id  # noqa: E402
from prisma_amd.policies import BUFFER_DIMS, StackedQNet  # noqa: E402
from prisma_amd.topology import Topology  # noqa: E402

SHAPES = {
    "config3": dict(topology="abilene_on_geant", replicas=4096, ping_as_obs=1, lf=1.0),
    "config4": dict(topology="geant", replicas=2048, ping_as_obs=0, lf=1.0),
}
DEFAULT_ORDER = ["buffer", "buffer_lite", "buffer_lighter", "buffer", "buffer_lighter_2", "buffer_lighter_3", "buffer"]


def measure(shape, model, args, explore=None):
    s = SHAPES[shape]
    topo = Topology.example(s["topology"], 0, s["lf"])
    params = engine_params(topo, sim_time_s=60.0, ping_as_obs=s["ping_as_obs"], auto_reset=1, seed=100,
                           log_capacity=8192)
    eng = PrismaEngine(topo, params, s["replicas"])
    w = StackedQNet(topo, model, seed=1234, device="cuda").pack()
    eng.reset(0)
    for _ in range(args.warmup):
        eng.run(w, args.hops, model=model, explore=explore)
    torch.cuda.synchronize()
    c0 = eng.counters()
    h0, e0 = int(c0["hops_total"].sum()), int(c0["events_total"].sum())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.run(w, args.hops, model=model, explore=explore)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cnt = eng.counters()
    hops = int(cnt["hops_total"].sum()) - h0
    out = {"shape": shape, "topology": s["topology"], "replicas": s["replicas"], "ping_as_obs": s["ping_as_obs"],
           "load_factor": s["lf"], "model": model, "traffic": "greedy" if explore is None else "uniform",
           "dims_B_H_NH": list(BUFFER_DIMS[model]), "weights_floats": int(w.numel()),
           "hops_per_launch": args.hops, "steps": args.steps, "warmup": args.warmup, "wall_s": round(dt, 4),
           "hops_per_s": round(hops / dt, 1),
           # the policies differ, and with them the traffic: the events a hop costs (injections, pings,
           # completions, arrivals inside tunnels) say how much of a rate difference is the workload's
           "events_per_hop": round((int(cnt["events_total"].sum()) - e0) / max(hops, 1), 4),
           "events_per_s": round((int(cnt["events_total"].sum()) - e0) / dt, 1),
           "errors": int(cnt["error"].max()), "build_id": build_id(),
           "kernel": eng.kernel_info(), "device": torch.cuda.get_device_name(0)}
    eng.close()
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", default="config4,config3")
    p.add_argument("--models", default=",".join(DEFAULT_ORDER), help="measured in this order, repeats included")
    p.add_argument("--hops", type=int, default=8192, help="hops per replica per launch")
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    args = p.parse_args(argv)
    for shape in args.shapes.split(","):
        for explore in (None, 1.0):
            for model in args.models.split(","):
                print(json.dumps(measure(shape, model, args, explore)), flush=True)


if __name__ == "__main__":
    main()
