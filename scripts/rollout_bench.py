#!/usr/bin/env python
"""Throughput of the training rollouts: the external path against the fused exploring kernels.

4 096 Abilene replicas, DQ-routing agents, eps 0.1 at every node.  One JSON line per part:

  a  trainer.train(): one decision per replica per launch (VecRoutingEnv.step, the torch policy,
     gather_records and the counters every step) -- decisions/s and transitions/s into the buffers
  b  trainer.train_fused(): one fused epsilon-greedy launch of --hops hops per replica, then the
     launch's transitions into the buffers -- the same two figures
  c  PrismaEngine.run(..., explore=0.1) alone against run() alone, hops/s (the cost of the draw)
  d  PrismaEngine.run(..., explore=0.1, action_history=...) alone against run(..., explore=0.1)
     alone, hops/s (the cost of the action counts and the history-weighted pick)
  e  what follows a fused launch: buffers.add(env.transitions()) (the torch chain) against
     env.ingest_transitions(buffers) (prisma_ingest_transitions) on the same log, wall time and peak
     allocated memory of each, and train_fused() with fused_ingest off and on, transitions/s; run it
     with --hops 256 and --hops 8192
  f  the targets of a training step, for --kinds routing,buffer: (i) QRoutingTrainer.targets() alone and
     train_step() on the torch path, with one stored generation, with the generations a
     --gen-steps train() run leaves and with --forced-gens made-up ones (replica r reading
     generation r mod G, the state of a long run); (ii) PrismaEngine.replay_targets
     (prisma_replay_targets) and train_step(engine=) on the same batch; (iii) train_fused()
     iterations at --hops-list hops with fused_targets off and on

    python scripts/rollout_bench.py --part a        # or b, c, d, e, f; --repeat 2 prints each line twice

Every part warms up first and is timed between device synchronisations.  bench.py stays the
headline's yardstick; this script only compares the rollout paths with each other."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prisma_amd import engine  # noqa: E402
from prisma_amd.env import VecRoutingEnv  # noqa: E402
from prisma_amd.trainer import QRoutingTrainer, train, train_fused  # noqa: E402


def pow2_at_least(n: int) -> int:
    p = 1024
    while p < n:
        p *= 2
    return p


def make(args, log_capacity, kind="routing"):
    env = VecRoutingEnv(args.topology, n_replicas=args.replicas, sim_time_s=60.0, auto_reset=1,
                        log_capacity=log_capacity)
    tr = QRoutingTrainer(env.topo, kind, n_replicas=args.replicas, seed=0, batch_size=args.batch,
                         eps_initial=args.eps, eps_final=args.eps)
    return env, tr


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def common(args, part):
    return {"part": part, "topology": args.topology, "replicas": args.replicas, "agent": "dq_routing",
            "eps": args.eps, "batch_size": args.batch, "build_id": engine.build_id(),
            "device": torch.cuda.get_device_name(0)}


def part_a(args):
    env, tr = make(args, 8192)
    train(env, tr, args.warmup_steps)
    for _ in range(args.repeat):
        seen0 = int(tr.buffers.total.sum())
        dt, losses = wall(lambda: train(env, tr, args.steps))
        out = common(args, "a")
        out.update(path="train (external actions)", steps=args.steps, wall_s=round(dt, 4),
                   decisions_per_s=round(args.replicas * args.steps / dt, 1),
                   transitions_per_s=round((int(tr.buffers.total.sum()) - seen0) / dt, 1),
                   train_steps=len(losses))
        print(json.dumps(out), flush=True)
    env.close()


def part_b(args):
    # a launch writes a record per hop and per destination arrival: twice the hops holds them
    env, tr = make(args, pow2_at_least(2 * args.hops))
    train_fused(env, tr, args.warmup_launches, args.hops)
    for _ in range(args.repeat):
        seen0 = int(tr.buffers.total.sum())
        dt, losses = wall(lambda: train_fused(env, tr, args.launches, args.hops))
        # (train_fused resets the env, and the hop totals restart with it: these are this call's)
        hops = int(env.counters()["hops_total"].sum())
        out = common(args, "b")
        out.update(path="train_fused (in-kernel exploration)", launches=args.launches, hops_per_launch=args.hops,
                   log_capacity=env.engine.log_capacity, wall_s=round(dt, 4),
                   decisions_per_s=round(hops / dt, 1),
                   transitions_per_s=round((int(tr.buffers.total.sum()) - seen0) / dt, 1),
                   train_steps=len(losses))
        print(json.dumps(out), flush=True)
    env.close()


def part_c(args):
    env, tr = make(args, 8192)
    table = tr.q.argmin_table()
    eps = torch.full((env.topo.n_nodes,), args.eps, dtype=torch.float64, device=env.device)
    for _ in range(args.repeat):
        res = {}
        for name, kw in (("greedy", {}), ("explore", {"explore": eps})):
            env.engine.reset(0)
            for _ in range(args.warmup_launches):
                env.run(table, args.hops, **kw)
            torch.cuda.synchronize()
            h0 = int(env.counters()["hops_total"].sum())
            dt, _ = wall(lambda: [env.run(table, args.hops, **kw) for _ in range(args.launches)])
            cnt = env.counters()
            assert int(cnt["error"].max()) == 0
            res[name] = (int(cnt["hops_total"].sum()) - h0) / dt
        out = common(args, "c")
        out.update(path="run alone", launches=args.launches, hops_per_launch=args.hops,
                   greedy_hops_per_s=round(res["greedy"], 1), explore_hops_per_s=round(res["explore"], 1),
                   explore_over_greedy=round(res["explore"] / res["greedy"], 4))
        print(json.dumps(out), flush=True)
    env.close()


def part_d(args):
    env, tr = make(args, 8192)
    table = tr.q.argmin_table()
    eps = torch.full((env.topo.n_nodes,), args.eps, dtype=torch.float64, device=env.device)
    for _ in range(args.repeat):
        res = {}
        for name in ("explore", "smart"):
            kw = {"explore": eps}
            if name == "smart":
                kw["action_history"] = env.engine.new_action_history()
            env.engine.reset(0)
            for _ in range(args.warmup_launches):
                env.run(table, args.hops, **kw)
            torch.cuda.synchronize()
            h0 = int(env.counters()["hops_total"].sum())
            dt, _ = wall(lambda: [env.run(table, args.hops, **kw) for _ in range(args.launches)])
            cnt = env.counters()
            assert int(cnt["error"].max()) == 0
            res[name] = (int(cnt["hops_total"].sum()) - h0) / dt
        out = common(args, "d")
        out.update(path="run alone", launches=args.launches, hops_per_launch=args.hops,
                   explore_hops_per_s=round(res["explore"], 1), smart_hops_per_s=round(res["smart"], 1),
                   smart_over_explore=round(res["smart"] / res["explore"], 4))
        print(json.dumps(out), flush=True)
    env.close()


def part_e(args):
    from prisma_amd.trainer import ReplayBuffers
    env, tr = make(args, pow2_at_least(2 * args.hops))
    twin = ReplayBuffers(tr.buffers.N, tr.buffers.size, tr.buffers.W, tr.buffers.device)
    table = tr.q.argmin_table()
    eps = torch.full((env.topo.n_nodes,), args.eps, dtype=torch.float64, device=env.device)
    fields = ("obs", "next_obs", "action", "reward", "done", "replica", "next_idx", "count", "total")

    def launch():
        env.run(table, args.hops, explore=eps)
        torch.cuda.synchronize()
        return env._consumed.clone()

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        dt, _ = wall(fn)
        return dt, torch.cuda.max_memory_allocated() - base

    env.reset()
    for _ in range(args.warmup_launches):                     # both paths once, on the same log
        c0 = launch()
        tr.buffers.add(env.transitions())
        env._consumed = c0
        env.ingest_transitions(twin)
    train_fused(env, tr, args.warmup_launches, args.hops, fused_ingest=True)
    for _ in range(args.repeat):
        env.reset()
        for _ in range(args.warmup_launches):
            launch()
            env.ingest_transitions(twin)
        c0 = launch()
        for f in fields:                                      # the twin starts where the torch path's buffers do
            getattr(twin, f).copy_(getattr(tr.buffers, f))
        before = int(tr.buffers.total.sum())
        t_torch, m_torch = peak(lambda: tr.buffers.add(env.transitions()))
        n = int(tr.buffers.total.sum()) - before
        c1 = env._consumed
        env._consumed = c0
        t_kernel, m_kernel = peak(lambda: env.ingest_transitions(twin))
        assert torch.equal(env._consumed, c1) and all(torch.equal(getattr(twin, f), getattr(tr.buffers, f))
                                                      for f in fields)
        res = {}
        for name, fused in (("torch", False), ("kernel", True)):
            seen0 = int(tr.buffers.total.sum())
            dt, losses = wall(lambda: train_fused(env, tr, args.launches, args.hops, fused_ingest=fused))
            res[name] = ((int(tr.buffers.total.sum()) - seen0) / dt, dt, len(losses))
        out = common(args, "e")
        out.update(path="after a fused launch: torch chain vs prisma_ingest_transitions", hops_per_launch=args.hops,
                   log_capacity=env.engine.log_capacity, transitions=n,
                   torch_add_transitions_s=round(t_torch, 6), ingest_s=round(t_kernel, 6),
                   torch_over_ingest=round(t_torch / t_kernel, 2),
                   torch_peak_bytes=int(m_torch), ingest_peak_bytes=int(m_kernel),
                   launches=args.launches,
                   train_fused_torch_transitions_per_s=round(res["torch"][0], 1),
                   train_fused_ingest_transitions_per_s=round(res["kernel"][0], 1),
                   train_fused_torch_wall_s=round(res["torch"][1], 4),
                   train_fused_ingest_wall_s=round(res["kernel"][1], 4), train_steps=res["kernel"][2])
        print(json.dumps(out), flush=True)
    env.close()


def part_f(args):
    import statistics

    def med(fn, n=args.timed):
        fn()                                                  # (warm: allocator, first-call tables)
        return statistics.median(wall(fn)[0] for _ in range(n))

    for kind in args.kinds.split(","):
        # (i), (ii): the targets of one sampled batch, torch path against prisma_replay_targets
        env, tr = make(args, 8192, kind)
        train_fused(env, tr, 4, 256, fused_ingest=True)       # fills the rings past the batch size
        N, B = tr.N, tr.batch_size
        node = torch.arange(N, device=tr.device).repeat_interleave(B)
        for stage in ("one generation", f"after a {args.gen_steps}-step train()",
                      f"{args.forced_gens} generations, replicas assigned in turn"):
            if stage == "one generation":
                tr.sync()
                tr.sync()                                     # every copy refers to the newest generation
            elif stage.startswith("after"):
                train(env, tr, args.gen_steps)
            else:
                # what a long run's drifting replica clocks leave (29 at the
                # peak), made here: a new version of perturbed weights per step, read by every G-th replica
                for g in range(args.forced_gens):
                    with torch.no_grad():
                        for p in tr.params:
                            p.mul_(1.0 + 1e-3 * (g + 1))
                    tr.version += 1
                    tr._snap_gen[tr.version] = tr._capture()
                    tr.tgt_ver[g::args.forced_gens] = tr.version
            gens = len({tr._snap_gen[int(k)] for k in set(tr.tgt_ver.ravel().tolist())})
            idx = tr.buffers.sample_idx(B, tr.gen)

            def torch_targets():
                s = tr.buffers.sample_full(B, idx=idx)
                with torch.no_grad():
                    return tr.targets(node, s["action"].reshape(-1), s["reward"].reshape(-1),
                                      s["next_obs"].reshape(N * B, -1), s["done"].reshape(-1), s["replica"].reshape(-1))

            def only_targets(s):
                with torch.no_grad():
                    return tr.targets(node, s["action"].reshape(-1), s["reward"].reshape(-1),
                                      s["next_obs"].reshape(N * B, -1), s["done"].reshape(-1), s["replica"].reshape(-1))

            s0 = tr.buffers.sample_full(B, idx=idx)
            weights, gen_of = tr._device_generations()
            ref = torch_targets()
            out = env.engine.replay_targets(tr.buffers, idx, weights, kind, tr.gamma, gen_of)
            fin = torch.isfinite(ref)
            err = float(((out["target"] - ref).abs() / ref.abs().clamp_min(1.0))[fin].max()) if bool(fin.any()) else 0.0
            t_targets = med(lambda: only_targets(s0))
            t_sample_targets = med(torch_targets)
            t_kernel = med(lambda: env.engine.replay_targets(tr.buffers, idx, weights, kind, tr.gamma, gen_of))
            # (the training steps last: they move the online weights, not the stored generations)
            t_step = med(lambda: tr.train_step())
            t_step_fused = med(lambda: tr.train_step(engine=env.engine))
            line = common(args, "f")
            line.update(agent=kind, path="targets of one batch: torch targets() vs prisma_replay_targets", stage=stage,
                        live_generations=gens, stored_generations=len(tr._gen_w), rows=N * B,
                        torch_targets_s=round(t_targets, 6), torch_sample_and_targets_s=round(t_sample_targets, 6),
                        replay_targets_s=round(t_kernel, 6), torch_over_kernel=round(t_sample_targets / t_kernel, 2),
                        train_step_torch_s=round(t_step, 6), train_step_fused_targets_s=round(t_step_fused, 6),
                        max_rel_diff_finite=err, timed=args.timed)
            print(json.dumps(line), flush=True)
        env.close()
        del env, tr
        torch.cuda.empty_cache()
        # (iii) train_fused iterations with and without fused_targets
        for hops in [int(h) for h in args.hops_list.split(",")]:
            env, tr = make(args, pow2_at_least(2 * hops), kind)
            train_fused(env, tr, args.warmup_launches, hops, fused_ingest=True, fused_targets=True)
            for _ in range(args.repeat):
                res = {}
                for name, fused in (("torch", False), ("kernel", True)):
                    dt, losses = wall(lambda: train_fused(env, tr, args.launches, hops, fused_ingest=True,
                                                          fused_targets=fused))
                    res[name] = (dt / args.launches, len(losses))
                line = common(args, "f")
                line.update(agent=kind, path="train_fused iteration: targets() vs fused_targets", hops_per_launch=hops,
                            log_capacity=env.engine.log_capacity, launches=args.launches,
                            stored_generations=len(tr._gen_w),
                            iteration_torch_targets_ms=round(1e3 * res["torch"][0], 3),
                            iteration_fused_targets_ms=round(1e3 * res["kernel"][0], 3), train_steps=res["kernel"][1])
                print(json.dumps(line), flush=True)
            env.close()
            del env, tr
            torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--part", choices=["a", "b", "c", "d", "e", "f"], required=True)
    p.add_argument("--kinds", default="routing,buffer", help="agent kinds (part f)")
    p.add_argument("--hops-list", default="256,8192", help="hops per launch of the train_fused iterations (part f)")
    p.add_argument("--gen-steps", type=int, default=600, help="train() steps that spread the generations (part f)")
    p.add_argument("--forced-gens", type=int, default=29, help="generations of the made-up spread (part f)")
    p.add_argument("--timed", type=int, default=7, help="timed calls per figure, the median is reported (part f)")
    p.add_argument("--topology", default="abilene")
    p.add_argument("--replicas", type=int, default=4096)
    p.add_argument("--eps", type=float, default=0.1)
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--hops", type=int, default=32768, help="hops per replica per fused launch (parts b, c, d, e)")
    p.add_argument("--launches", type=int, default=3, help="timed fused launches (parts b, c)")
    p.add_argument("--warmup-launches", type=int, default=1)
    p.add_argument("--steps", type=int, default=200, help="timed env steps (part a)")
    p.add_argument("--warmup-steps", type=int, default=20)
    p.add_argument("--repeat", type=int, default=2, help="timed repeats, one JSON line each (the spread)")
    args = p.parse_args(argv)
    {"a": part_a, "b": part_b, "c": part_c, "d": part_d, "e": part_e, "f": part_f}[args.part](args)


if __name__ == "__main__":
    main()
