"""Both engines against the CPU oracle, byte for byte, at sparse traffic over full-length episodes:
the cases of tests/sparse_cases.py (sim_time_s = 4095, load factors of 0.0002 to 0.002).  They reach
what no loaded, short run does: an idle network, where the next event lies 2^32 - 1 ns or more
ahead and the event selection's exact 64-bit path decides (engine_core.h select_event,
prisma_engine_mem.hip wave_min_key_exact), and a late clock, where the device-only forms of the
time code (numerics.h div_1e3, div_1e9, div_const, py_micros, py_reward; engine_core.h
ping_send_s) work on t up to 4.095e12 ns, microseconds above 2^31 and start seconds above 2^11.

Every run: 3 replicas from replica_base 7, the whole episode (a few thousand hops) in a log that
holds all of its records; tests/test_sparse_long.py checks on the CPU that each case's episode has
the idle gaps, the late records and the py_micros ties it is here for.  Through the fused table
instances (lite, ctrl, tunnelled), the MLP ones under weights that decide as the shortest-path
table does, the memory-resident engine, the external-policy step loop, the episode end at 4095 s
with auto_reset and the exploring set."""
import numpy as np
import pytest
import torch

import sparse_cases as S
from explore_util import SteppedOracle
from parity_util import assert_counters_equal, compare_steady, first_difference, run_fused_both
from prisma_amd import explore
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine
from test_gpu_prio_ladder import FOUR_WAVE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

ENGINES = {"register": PRISMA_ENGINE_REGISTER, "memory": PRISMA_ENGINE_MEMORY}


def _kernel(name, engine):
    """The prisma_kernel_info fields a case must report, and the start of the name of the instance
    its table runs launch: the fused table instances on identity overlays without the ctrl paths,
    the ctrl instances with --train, notify_dest or ns-3's streams (prisma_engine.hip ctrl_env),
    the tunnelled ones on Abilene over GEANT."""
    c, params = S.CASES[name], S.case_params(name)
    ctrl = int(bool(params["train"] or params["notify_dest"] or params["rng_mode"]))
    tun = int(c["topo"] == "abilene_on_geant")
    if engine == PRISMA_ENGINE_MEMORY:
        return dict(engine=engine, ctrl=ctrl), f"prisma_mem_step_kernel<false, {'true' if ctrl else 'false'}>"
    fs, ls = S.SHAPES[c["topo"]]
    ki = dict(engine=engine, flow_slots=fs, link_slots=ls, tunnels=tun, ctrl=ctrl)
    if ctrl or tun:
        return ki, f"prisma_step_kernel_t<{fs}, {ls}, false, {'true' if tun else 'false'}, {'true' if ctrl else 'false'}>"
    return ki, f"prisma_step_kernel_fused_t<{fs}, {ls}, "


def _both(oracle_mod, name, pol, engine, launches=3, hops=None):
    """The case's whole episode over `launches` launches of a third of its hop budget each: it ends
    inside a launch, and the later launches find it over."""
    ki, kname = _kernel(name, engine)
    if pol == "mlp":
        kname = kname.replace("<false", "<true") if engine == PRISMA_ENGINE_MEMORY else \
            f"prisma_step_kernel_t<{ki['flow_slots']}, {ki['link_slots']}, true, false, {'true' if ki['ctrl'] else 'false'}>"
    H = S.CASES[name]["hops"] if hops is None else hops
    cnt, refs = run_fused_both(oracle_mod, S.case_topo(name), S.case_params(name, engine=engine), S.R, H,
                               S.policy(name, pol), launches=launches, kernel=ki, kernel_name=kname,
                               net_cpu=S.net(name)[0] if pol == "mlp" else None,
                               label=f"{name} {pol} engine {engine}")
    for r in range(S.R):
        assert int(cnt[r]["episode_over"]) == 1 and int(cnt[r]["hops_total"]) < H
        assert int(cnt[r]["now_ns"]) >= 4080 * 10**9 and len(refs[r]) <= S.LOG
    return cnt, refs


@pytest.mark.parametrize("name", list(S.CASES))
def test_fused_table(oracle_mod, name):
    _both(oracle_mod, name, "table", PRISMA_ENGINE_REGISTER)


def test_headline_instance_in_one_launch(oracle_mod):
    """`idle` on the headline instance (2 flow slots, 1 link slot: 4 waves per SIMD) in one launch
    of the bench's 32 768 hops: the issue-priority ladder at its shipped chunk, with the episode end
    inside its first chunk."""
    ki, _ = _kernel("idle", PRISMA_ENGINE_REGISTER)
    assert ki == dict(FOUR_WAVE, tunnels=0)
    _both(oracle_mod, "idle", "table", PRISMA_ENGINE_REGISTER, launches=1, hops=32768)


@pytest.mark.parametrize("name", S.MLP_CASES)
def test_mlp_instances(oracle_mod, name):
    """The lite and ctrl MLP instances under the SP-equivalent weights; every decision also against
    torch's fp32 model (check_near_ties)."""
    _, refs = _both(oracle_mod, name, "mlp", PRISMA_ENGINE_REGISTER)
    for ref, (_, want, _, _) in zip(refs, S.oracle_runs(name)):
        assert ref.tobytes() == want.tobytes()                  # the SP table's own records


@pytest.mark.parametrize("name,pol", S.MEMORY_RUNS, ids=["-".join(r) for r in S.MEMORY_RUNS])
def test_memory_engine(oracle_mod, name, pol):
    """GEANT's 506 flows are 8 flow blocks and one group of the event tree: wave_min_key falls back
    to wave_min_key_exact in each when the network is idle."""
    _both(oracle_mod, name, pol, PRISMA_ENGINE_MEMORY)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_external_step_loop_through_the_episode(oracle_mod, engine):
    """prisma_step in lock-step with three oracles under the SP table's actions until every mask is
    0 (about 1.9 k steps): the observations, the mask and the pending node after every step -- the
    late-time reward, ping delays and finish_pending -- then every record and the counters."""
    name = "idle"
    topo, params = S.case_topo(name), S.case_params(name, engine=ENGINES[engine])
    table, on = S.table(name), S.case_topo(name).overlay_nodes
    eng = PrismaEngine(topo, params, S.R)
    try:
        assert eng.kernel_info()["engine"] == ENGINES[engine]
        eng.reset(0)
        orcs = [oracle_mod.OracleSim(topo, params, replica=S.REPLICA_BASE + r) for r in range(S.R)]
        ref_obs = [o.step(-1) for o in orcs]
        obs, mask, node = eng.step(None)
        steps = 0
        while True:
            g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
            acts = np.zeros(S.R, dtype=np.int32)
            for r in range(S.R):
                assert (ref_obs[r] is None) == (m[r] == 0), (steps, r)
                if ref_obs[r] is None:
                    continue
                assert np.array_equal(ref_obs[r], g[r]), (steps, r, g[r], ref_obs[r])
                assert nd[r] == orcs[r].pending_node(), (steps, r)
                acts[r] = table[nd[r], on[g[r][0]]]
            if not m.any():
                break
            assert steps < S.CASES[name]["hops"]
            ref_obs = [orcs[r].step(int(acts[r])) if ref_obs[r] is not None else None for r in range(S.R)]
            obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
            steps += 1
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r, (_, want, _, _) in zip(range(S.R), S.oracle_runs(name)):
            ref = orcs[r].records()
            assert ref.tobytes() == want.tobytes()              # the fused table run's episode
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["episode_over"]) == 1
            assert int(cnt[r]["dec_count"]) == len(ref) <= eng.log_capacity
            got = eng.records(r, 0, len(ref), log_host=log)
            bad = first_difference(got, ref)
            assert bad is None, f"{engine} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {ref[bad]}"
            assert_counters_equal(cnt[r], orcs[r].counters(), r, f" (idle step loop, {engine})")
        assert steps > 1700
    finally:
        eng.close()


STEADY_RUNS = [("idle", "register"), ("idle_geant", "register"), ("idle", "memory")]


@pytest.mark.parametrize("name,engine", STEADY_RUNS, ids=["-".join(r) for r in STEADY_RUNS])
def test_episode_end_at_4095_s_and_auto_reset(oracle_mod, name, engine):
    """auto_reset at about a fifth of an episode per launch, through the episode end at 4095 s and
    300 s of simulated time beyond: episode 1 starts with the clock, the microsecond state and the
    12-bit start second back at zero, and matches the oracle's episode 1 record for record."""
    topo = S.case_topo(name)
    params = S.case_params(name, engine=ENGINES[engine], auto_reset=1)
    eng = PrismaEngine(topo, params, S.R)
    try:
        assert eng.kernel_info()["engine"] == ENGINES[engine]
        eng.reset(0)
        out = compare_steady(oracle_mod, eng, topo, params, S.policy(name, "table"), t_target_s=S.SIM_TIME_S + 300,
                             hops_per_launch=max(h for h, _, _, _ in S.oracle_runs(name)) // 5, min_episode=1,
                             max_launches=40, label=f"{name} {engine} auto_reset")
        assert out["t_compared_s"] >= S.SIM_TIME_S + 300 and out["episodes"] == [1] * S.R
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r, (_, ep0, _, _) in zip(range(S.R), S.oracle_runs(name)):
            n = int(cnt[r]["dec_count"])
            recs = eng.records(r, 0, n, log_host=log)
            assert n <= eng.log_capacity and recs[:len(ep0)].tobytes() == ep0.tobytes()
            ep1 = recs[len(ep0):]
            assert len(ep1) > 20 and (ep1["episode"] == 1).all() and (recs[:len(ep0)]["episode"] == 0).all()
            assert ep0["t_ns"][-1] >= 4080 * 10**9 and ep1["t_ns"][0] < 100 * 10**9
            assert (ep1["start_s"] <= ep1["t_ns"] // 10**9).all() and ep1["start_s"][0] < 100
            assert (ep1["prev"][ep1["prev"] >= 0] >= len(ep0)).all()
            assert np.abs(ep1["reward"]).max() < 1.0            # a hop's delay, not one taken from 4095 s
    finally:
        eng.close()


def test_exploring_kernels_through_the_episode(oracle_mod):
    """`idle` under run(..., explore=0.1) to the episode's end, against an oracle stepped decision
    by decision under the same rule (SteppedOracle)."""
    name = "idle"
    topo, params, policy = S.case_topo(name), S.case_params(name), S.policy(name, "table")
    eps = np.full(topo.n_nodes, 0.1)
    thr = explore.thresholds(eps)
    H = S.CASES[name]["hops"]
    eng = PrismaEngine(topo, params, S.R)
    try:
        ki, _ = _kernel(name, PRISMA_ENGINE_REGISTER)
        got_ki = eng.kernel_info()
        assert {k: got_ki[k] for k in ki} == ki, got_ki
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(policy[1])).cuda()
        dev_eps = torch.from_numpy(eps).cuda()
        for _ in range(3):
            eng.run(dev, H // 3, explore=dev_eps)
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(S.R):
            ref = SteppedOracle(oracle_mod, topo, params, S.REPLICA_BASE + r, thr, policy, scalar_check=False).run()
            oc = ref.counters()
            assert int(oc["episode_over"]) == 1 and int(oc["error"]) == 0 and int(oc["now_ns"]) >= 4080 * 10**9
            assert ref.explored > 100 and ref.changed > 50 and ref.explored < ref.decisions < H
            want = ref.records()
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["episode_over"]) == 1
            assert int(cnt[r]["hops_total"]) == ref.decisions
            assert int(cnt[r]["dec_count"]) == len(want) <= eng.log_capacity
            got = eng.records(r, 0, len(want), log_host=log)
            bad = first_difference(got, want)
            assert bad is None, f"idle explore replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {want[bad]}"
            assert_counters_equal(cnt[r], oc, r, " (idle, explore)")
    finally:
        eng.close()
