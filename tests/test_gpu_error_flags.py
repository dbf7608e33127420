"""The engine's defined failures against the oracle's restatement of them (include/prisma.h
PRISMA_EBIT_LOGWRAP and _PINGIDX): every replica fails at the record, clock and counters its own
oracle run fails at, a failed replica stays as it is until reset, and the Python surface reports
the failure.  The scenarios and their premises: tests/parity_util.py, tests/test_error_flags.py.

A 1 024-record ring holds less than a launch writes, so after each launch the records the ring
still holds (the launch's last log_capacity at most) are compared; at the failure those are the
log_capacity records before the refused one."""
import functools

import numpy as np
import pytest
import torch

import parity_util as P
import synth_topology as S
from explore_util import SteppedOracle
from prisma_amd import explore
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine, PrismaError
from prisma_amd.records import EBIT_LOGWRAP, EBIT_PINGIDX
from prisma_amd.topology import sp_next_hop_table

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

R, BASE = P.WRAP_R, P.WRAP_BASE


class _Fused:
    """One replica's oracle advanced by hops under a fused policy."""

    def __init__(self, oracle_mod, topo, params, replica, policy):
        self.kind, self.pol = policy
        self.o = oracle_mod.OracleSim(topo, params, replica=replica)

    def advance(self, hops):
        return self.o.run_table(self.pol, hops) if self.kind == "table" else self.o.run_mlp(self.pol, hops)


def _budget(oracle_mod, topo, params, policy, bit):
    """Hops per replica: 1.5 x what the slowest replica's oracle needs to reach its failure (an
    even number, for two launches), and the failure points."""
    hops, decs = [], []
    for r in range(R):
        f = _Fused(oracle_mod, topo, params, params["replica_base"] + r, policy)
        hops.append(f.advance(10 ** 9))
        c = f.o.counters()
        assert int(c["error"]) == bit and int(c["episode_over"]) == 1, (r, c)
        decs.append(int(c["dec_count"]))
        f.o.close()
    H = 2 * int(np.ceil(0.75 * max(hops)))
    assert H <= P.WRAP_MAX_HOPS
    return H, decs


def _compare(eng, cnt, log, r, o, checked, label, bit=None):
    """Replica r after a launch against its oracle `o`: the counters, and the records since
    `checked` that the ring still holds.  Returns the new `checked`."""
    c, oc = cnt[r], o.counters()
    for k in ("error", "episode_over", "dec_count", "hops_total", "now_ns"):
        assert int(c[k]) == int(oc[k]), (label, r, k, int(c[k]), int(oc[k]))
    if bit is not None:
        assert int(c["error"]) == bit and int(c["episode_over"]) == 1, (label, r, int(c["error"]))
    total = int(c["dec_count"])
    first = max(checked, total - eng.log_capacity)
    got = eng.records(r, first, total - first, log_host=log)
    want = o.records(first, total - first)
    bad = P.first_difference(got, want)
    assert bad is None, f"{label} replica {r}: record {first + bad} differs\n engine {got[bad]}\n oracle {want[bad]}"
    P.assert_counters_equal(c, oc, r, f" ({label})")
    assert int(c["events_total"]) == int(oc["events"])
    return total


def _run_to_failure(oracle_mod, topo, params, policy, bit, label, *, launches=2, kernel=None):
    """R replicas for the budget's hops over `launches` launches; compared after every launch.
    Every replica must have failed with `bit` by the end, each at its own record."""
    H, decs = _budget(oracle_mod, topo, params, policy, bit)
    assert len(set(decs)) == R, (label, decs)
    eng = PrismaEngine(topo, params, R)
    try:
        if kernel is not None:
            ki = eng.kernel_info()
            assert {k: ki[k] for k in kernel} == kernel, (label, ki)
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(policy[1])).cuda()
        refs = [_Fused(oracle_mod, topo, params, params["replica_base"] + r, policy) for r in range(R)]
        checked = [0] * R
        failed_in = []
        for launch in range(launches):
            eng.run(dev, H // launches)
            torch.cuda.synchronize()
            cnt = eng.counters()
            log = eng.log_tensor().cpu().numpy()
            for r in range(R):
                refs[r].advance(H // launches)
                last = launch == launches - 1
                checked[r] = _compare(eng, cnt, log, r, refs[r].o, checked[r], f"{label}, launch {launch}",
                                      bit if last else None)
            failed_in.append(int((cnt["error"] != 0).sum()))
        assert [int(c) for c in cnt["dec_count"]] == decs, (label, decs)
        return eng, cnt, log, failed_in
    except BaseException:
        eng.close()
        raise


def _wrap(name, **kw):
    topo, params, table = P.wrap_case(P.WRAP_SCENARIOS[name], P.WRAP_CAP, **kw)
    return topo, params, ("table", table)


# ---- PRISMA_EBIT_LOGWRAP at log_capacity = 1024, one case per code path that carries the check ----
WRAP_GPU = {
    # register engine, identity overlay, the instances without / with the ctrl paths
    "lite": ("abilene_lf3", {}, dict(engine=PRISMA_ENGINE_REGISTER, ctrl=0, tunnels=0)),
    "ctrl": ("abilene_lf3_train", {}, dict(engine=PRISMA_ENGINE_REGISTER, ctrl=1, tunnels=0)),
    "memory": ("abilene_lf3", dict(engine=PRISMA_ENGINE_MEMORY), dict(engine=PRISMA_ENGINE_MEMORY)),
    # two link slots
    "geant": ("geant_lf2", {}, dict(engine=PRISMA_ENGINE_REGISTER, ctrl=0, link_slots=2)),
    # tunnelled, relay entries with an 18-bit index and the check inside the tunnel
    "tun_abilene_on_geant": ("abilene_on_geant_lf3", {}, dict(tunnels=1, relay_ip=1, relay_dec_bits=18)),
    # (two replicas stop at a switch inside a tunnel, before the packet reaches the tunnel's end)
    "tun_inside_first": ("abilene_on_geant_lf3_s129", {}, dict(tunnels=1, relay_ip=1, relay_dec_bits=18)),
    "tun_mesh3": ("mesh3_lf20", {}, dict(tunnels=1, relay_ip=1, relay_dec_bits=18)),
    # tunnelled with the ctrl paths: a 22-bit index, the previous record read at every switch
    "tun_mesh3_ctrl": ("mesh3_lf20_train", {}, dict(tunnels=1, relay_ip=0, ctrl=1, relay_dec_bits=22)),
    # (the same instances; replica 5 stops at a switch inside a tunnel)
    "tun_ctrl_inside_first": ("abilene_on_geant_lf3_s130_train", {},
                              dict(tunnels=1, relay_ip=0, ctrl=1, relay_dec_bits=22)),
}


@pytest.mark.parametrize("case", list(WRAP_GPU))
def test_logwrap_parity(oracle_mod, case):
    name, kw, kernel = WRAP_GPU[case]
    topo, params, policy = _wrap(name, **kw)
    eng, cnt, _, failed_in = _run_to_failure(oracle_mod, topo, params, policy, EBIT_LOGWRAP, case, kernel=kernel)
    eng.close()
    assert np.all(cnt["dec_count"] > P.WRAP_CAP)
    print(f"[{case}] failures after each launch: {failed_in}; records {cnt['dec_count'].tolist()}")


def test_logwrap_parity_dqn_buffer(oracle_mod):
    """The in-kernel DQN-buffer policy (the MLP instances' copy of the arrival path)."""
    topo, params, w = P.wrap_mlp_case(P.WRAP_CAP)
    big = P.wrap_mlp_case(P.BIG_LOG)[1]
    for r in range(R):                                     # the premise, on the CPU
        o = oracle_mod.OracleSim(topo, big, replica=BASE + r)
        o.run_mlp(w, P.WRAP_MLP_HOPS)
        rec = o.records()
        d = P.first_wrap(rec, P.WRAP_CAP)
        assert d is not None and d < 0.75 * len(rec) and int(P.record_ages(rec).max()) < P.CLEAN_CAP
        o.close()
    eng, cnt, _, _ = _run_to_failure(oracle_mod, topo, params, ("mlp", w), EBIT_LOGWRAP, "dqn-buffer")
    eng.close()


def test_logwrap_parity_explore(oracle_mod):
    """One run(..., explore=eps) launch (the exploring instances), the oracle stepped under the
    host's restatement of the draw rule."""
    topo, params, (_, table) = _wrap("abilene_lf3")
    eps = np.full(topo.n_nodes, 0.1)
    refs = [SteppedOracle(oracle_mod, topo, params, BASE + r, explore.thresholds(eps), ("table", table)).run()
            for r in range(R)]
    for ref in refs:                                       # the premise, on the CPU
        c = ref.counters()
        assert int(c["error"]) == EBIT_LOGWRAP and int(c["dec_count"]) > P.WRAP_CAP and ref.changed > 20
    assert len({int(ref.counters()["dec_count"]) for ref in refs}) == R
    H = int(np.ceil(1.5 * max(int(ref.counters()["hops"]) for ref in refs)))
    assert H <= P.WRAP_MAX_HOPS
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        eng.run(torch.from_numpy(table).cuda(), H, explore=eps)
        torch.cuda.synchronize()
        cnt, log = eng.counters(), eng.log_tensor().cpu().numpy()
        for r in range(R):
            _compare(eng, cnt, log, r, refs[r].o, 0, "explore", EBIT_LOGWRAP)
    finally:
        eng.close()


def test_logwrap_parity_external_steps(oracle_mod):
    """The external path: engine.step(actions) with the SP action of every pending (node, dst)
    until every replica has failed, the oracle stepped the same way."""
    topo, params, (_, table) = _wrap("abilene_lf3")
    H, decs = _budget(oracle_mod, topo, params, ("table", table), EBIT_LOGWRAP)
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        orcs = [oracle_mod.OracleSim(topo, params, replica=BASE + r) for r in range(R)]
        ref_obs = [o.step(-1) for o in orcs]
        obs, mask, node = eng.step(None)
        for s in range(H):
            g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
            if not m.any():
                break
            acts = np.zeros(R, dtype=np.int32)
            for r in range(R):
                assert (ref_obs[r] is None) == (m[r] == 0), (s, r)
                if ref_obs[r] is None:
                    continue
                assert np.array_equal(ref_obs[r], g[r]) and nd[r] == orcs[r].pending_node(), (s, r, g[r], ref_obs[r])
                acts[r] = table[nd[r], g[r][0]]
            ref_obs = [orcs[r].step(int(acts[r])) for r in range(R)]
            obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
        else:
            raise AssertionError(f"{H} steps did not stop every replica")
        assert all(o is None for o in ref_obs) and 1000 < s
        torch.cuda.synchronize()
        cnt, log = eng.counters(), eng.log_tensor().cpu().numpy()
        for r in range(R):
            _compare(eng, cnt, log, r, orcs[r], 0, "external", EBIT_LOGWRAP)
        assert [int(c) for c in cnt["dec_count"]] == decs           # where the fused run fails too
    finally:
        eng.close()


# ---- the clean twin: the same runs at log_capacity = 2048 (geant's ages exceed it) ----------------
# (run_fused_both compares the records the ring holds at the end, the run's last 2 048, and the
# counters, which cover the whole run; the exploring launch and the external steps follow below)
@pytest.mark.parametrize("case", [c for c in WRAP_GPU if c != "geant"] + ["dqn-buffer"])
def test_clean_twin_at_2048(oracle_mod, case):
    if case == "dqn-buffer":
        topo, small, w = P.wrap_mlp_case(P.WRAP_CAP)
        params, policy, kernel = P.wrap_mlp_case(P.CLEAN_CAP)[1], ("mlp", w), None
    else:
        name, kw, kernel = WRAP_GPU[case]
        topo, small, policy = _wrap(name, **kw)
        params = P.wrap_case(P.WRAP_SCENARIOS[name], P.CLEAN_CAP, **kw)[1]
    H, _ = _budget(oracle_mod, topo, small, policy, EBIT_LOGWRAP)
    cnt, _ = P.run_fused_both(oracle_mod, topo, params, R, H, policy, launches=2, kernel=kernel, label=case)
    assert np.all(cnt["error"] == 0) and np.all(cnt["episode_over"] == 0) and np.all(cnt["hops_total"] == H)


def test_clean_twin_explore_at_2048(oracle_mod):
    """run_fused_both drives neither the exploring launch nor the external steps: their twins
    through their own drivers.  The same budget as the failing run's; step(None) after the launch
    brings the engine to the next decision, where the stepped oracle stands."""
    topo, small, (_, table) = _wrap("abilene_lf3")
    params = P.wrap_case(P.WRAP_SCENARIOS["abilene_lf3"], P.CLEAN_CAP)[1]
    eps = np.full(topo.n_nodes, 0.1)
    thr = explore.thresholds(eps)
    fail_hops = [int(SteppedOracle(oracle_mod, topo, small, BASE + r, thr, ("table", table), scalar_check=False)
                     .run().counters()["hops"]) for r in range(R)]
    H = int(np.ceil(1.5 * max(fail_hops)))
    refs = [SteppedOracle(oracle_mod, topo, params, BASE + r, thr, ("table", table)) for r in range(R)]
    for ref in refs:
        while ref.obs is not None and int(ref.counters()["hops"]) < H:
            ref.step()
        assert ref.obs is not None and int(ref.counters()["hops"]) == H
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        eng.run(torch.from_numpy(table).cuda(), H, explore=eps)
        _, mask, _ = eng.step(None)
        assert bool(mask.all())
        torch.cuda.synchronize()
        cnt, log = eng.counters(), eng.log_tensor().cpu().numpy()
        assert np.all(cnt["error"] == 0) and np.all(cnt["episode_over"] == 0) and np.all(cnt["hops_total"] == H)
        for r in range(R):
            _compare(eng, cnt, log, r, refs[r].o, 0, "explore twin")
    finally:
        eng.close()


def test_clean_twin_external_steps_at_2048(oracle_mod):
    topo, small, (_, table) = _wrap("abilene_lf3")
    params = P.wrap_case(P.WRAP_SCENARIOS["abilene_lf3"], P.CLEAN_CAP)[1]
    H, _ = _budget(oracle_mod, topo, small, ("table", table), EBIT_LOGWRAP)
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        orcs = [oracle_mod.OracleSim(topo, params, replica=BASE + r) for r in range(R)]
        ref_obs = [o.step(-1) for o in orcs]
        obs, mask, node = eng.step(None)
        for s in range(H):
            g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
            acts = np.zeros(R, dtype=np.int32)
            for r in range(R):
                assert ref_obs[r] is not None and m[r] == 1, (s, r)
                assert np.array_equal(ref_obs[r], g[r]) and nd[r] == orcs[r].pending_node(), (s, r, g[r], ref_obs[r])
                acts[r] = table[nd[r], g[r][0]]
            ref_obs = [orcs[r].step(int(acts[r])) for r in range(R)]
            obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
        torch.cuda.synchronize()
        cnt, log = eng.counters(), eng.log_tensor().cpu().numpy()
        assert np.all(cnt["error"] == 0) and np.all(cnt["episode_over"] == 0) and np.all(cnt["hops_total"] == H)
        for r in range(R):
            _compare(eng, cnt, log, r, orcs[r], 0, "external twin")
    finally:
        eng.close()


# ---- a failed replica stays as it is ------------------------------------------------------------
def test_failure_is_sticky_until_reset(oracle_mod):
    topo, params, policy = _wrap("abilene_lf3")
    eng, cnt, log, _ = _run_to_failure(oracle_mod, topo, params, policy, EBIT_LOGWRAP, "sticky")
    try:
        dev = torch.from_numpy(policy[1]).cuda()
        for _ in range(2):
            eng.run(dev, 500)
        torch.cuda.synchronize()
        assert eng.counters().tobytes() == cnt.tobytes()
        assert eng.log_tensor().cpu().numpy().tobytes() == log.tobytes()
        _, mask, node = eng.step(None)                          # the external path neither
        assert not mask.any().item() and (node == -1).all().item()
        assert eng.counters().tobytes() == cnt.tobytes()
        # reset: the flag is gone and the same run reproduces the same failure
        eng.reset(0)
        torch.cuda.synchronize()
        c0 = eng.counters()
        assert np.all(c0["error"] == 0) and np.all(c0["episode_over"] == 0) and np.all(c0["dec_count"] == 0)
        H = int(cnt["hops_total"].max()) * 3 // 2
        eng.run(dev, H)
        torch.cuda.synchronize()
        again = eng.counters()
        assert np.all(again["error"] == EBIT_LOGWRAP)
        assert again.tobytes() == cnt.tobytes()
        for r in range(R):
            n = int(cnt[r]["dec_count"])
            assert (eng.records(r, n - P.WRAP_CAP, P.WRAP_CAP).tobytes()
                    == eng.records(r, n - P.WRAP_CAP, P.WRAP_CAP, log_host=log).tobytes())
    finally:
        eng.close()


def test_auto_reset_leaves_a_failed_replica_alone(oracle_mod):
    """With auto_reset a replica whose episode ends starts its next one, inside the launch (from
    its spare image) or in the reset after it: neither touches a failed replica."""
    topo, params, policy = _wrap("abilene_lf3", auto_reset=1)
    eng, cnt, log, failed_in = _run_to_failure(oracle_mod, topo, params, policy, EBIT_LOGWRAP, "auto_reset")
    try:
        assert np.all(cnt["episode"] == 0)
        dev = torch.from_numpy(policy[1]).cuda()
        for _ in range(2):
            eng.run(dev, 500)
        torch.cuda.synchronize()
        after = eng.counters()
        assert np.all(after["episode"] == 0) and np.all(after["error"] == EBIT_LOGWRAP)
        assert after.tobytes() == cnt.tobytes()
        assert eng.log_tensor().cpu().numpy().tobytes() == log.tobytes()
    finally:
        eng.close()


# ---- PRISMA_EBIT_PINGIDX -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.ERROR_CASES))
def test_pingidx_parity(oracle_mod, name):
    """(The register engine only: the memory-resident engine runs identity overlays, where a
    ping-back's tunnel is its own link; tests/test_error_flags.py asserts the refusal.)"""
    kind = PRISMA_ENGINE_REGISTER
    topo = S.build_error(name)
    params = S.error_params(name, ping_as_obs=1, engine=kind)
    policy = ("table", sp_next_hop_table(topo))
    # (the budget: S.H = 3 000 hops over two launches, far more than the 8 to 47 records need)
    eng = PrismaEngine(topo, params, S.R)
    try:
        assert eng.engine_kind == kind and eng.kernel_info()["tunnels"] == 1
        eng.reset(0)
        dev = torch.from_numpy(policy[1]).cuda()
        refs = [_Fused(oracle_mod, topo, params, S.REPLICA_BASE + r, policy) for r in range(S.R)]
        checked = [0] * S.R
        for launch in range(2):
            eng.run(dev, S.H // 2)
            torch.cuda.synchronize()
            cnt, log = eng.counters(), eng.log_tensor().cpu().numpy()
            for r in range(S.R):
                refs[r].advance(S.H // 2)
                checked[r] = _compare(eng, cnt, log, r, refs[r].o, checked[r], f"{name}, launch {launch}", EBIT_PINGIDX)
        assert np.all(cnt["hops_total"] < S.H // 2) and np.all(cnt["dec_count"] > 0)
    finally:
        eng.close()


# ---- the log's range ----------------------------------------------------------------------------
def test_log_capacity_of_2_22_is_refused():
    topo, params, _ = P.wrap_case(P.WRAP_SCENARIOS["mesh3_lf20"], P.WRAP_CAP)
    with pytest.raises(PrismaError, match=r"log_capacity.*2\^21"):
        PrismaEngine(topo, dict(params, log_capacity=1 << 22), 1)


# ---- the Python surface --------------------------------------------------------------------------
def test_env_reports_the_failure_and_train_fused_raises():
    from prisma_amd.env import VecRoutingEnv
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    sc = P.WRAP_SCENARIOS["abilene_lf3"]
    env = VecRoutingEnv(sc["topo"], 0, sc["lf"], n_replicas=R, sim_time_s=30.0, ping_as_obs=sc["ping"],
                        replica_base=BASE, log_capacity=P.WRAP_CAP)
    try:
        table = torch.from_numpy(sp_next_hop_table(env.topo)).to(env.device)
        obs, info = env.reset()
        assert info["error"].dtype == torch.int64 and info["error"].shape == (R,) and info["error"].is_cuda
        node = info["node"]
        for s in range(P.WRAP_MAX_HOPS):
            acts = table[node.clamp_min(0).long(), obs[:, 0].long()].to(torch.int32)
            obs, _, _, info = env.step(acts)
            node = info["node"]
            if bool((info["error"] != 0).any()):
                break
        else:
            raise AssertionError("no replica failed")
        err = info["error"].cpu().numpy()
        cnt = env.counters()
        assert np.array_equal(err, cnt["error"].astype(np.int64))
        failed = err != 0
        assert np.all(err[failed] == EBIT_LOGWRAP) and np.all(info["mask"].cpu().numpy()[failed] == 0)
        assert np.all(cnt["episode_over"][failed] == 1) and np.all(cnt["dec_count"][failed] > P.WRAP_CAP)
        # train_fused starts over (env.reset) and meets the same failure in its fused rollouts
        tr = QRoutingTrainer(env.topo, "routing", batch_size=32, buffer_size=1 << 12, seed=0, n_replicas=R)
        with pytest.raises(RuntimeError, match=r"LOGWRAP \(16\)") as ei:
            train_fused(env, tr, 40, 300)
        assert f"of {R} replicas" in str(ei.value)
        assert np.any(env.counters()["error"] == EBIT_LOGWRAP)
    finally:
        env.close()
