"""The reduced DQN-buffer models decided in-kernel (prisma_run / prisma_run_explore with
PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3; PrismaEngine.run(..., model=)) against one CPU oracle
per replica stepped with the host restatement's action (lightq_util: nothing is read from the
GPU): every decision record byte for byte and every counter, and each decision against torch
fp32 under the near-tie rule.

Unless a test says otherwise: 2 replicas, 1 500 hops per replica in launches of 769 and 731 hops
after a prisma_step that leaves a decision pending (so the first launch starts at the
pending-decision site), a log of 2 048 records, and a load at which packets are dropped."""
import functools

import numpy as np
import pytest
import torch

import lightq_util as LQ
import synth_topology as S
from parity_util import assert_counters_equal, check_near_ties, first_difference
from prisma_amd import explore
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaEngine, PrismaError, model_floats
from prisma_amd.policies import StackedQNet
from prisma_amd.topology import Topology

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

NEW_KINDS = ["buffer_lite", "buffer_lighter", "buffer_lighter_2", "buffer_lighter_3"]
LAUNCHES = (769, 731)
LOG = 2048


@functools.lru_cache(maxsize=None)
def _topo(name, lf):
    return Topology.example(name, 0, lf)


_nets = {}


def _net(topo, kind, seed=21):
    """The torch model of a case on the CPU and its packed weights (numpy), built once."""
    key = (id(topo), kind, seed)
    if key not in _nets:
        net = StackedQNet(topo, kind, seed=seed, device="cpu")
        _nets[key] = (topo, net, net.pack().numpy())
    return _nets[key][1:]


def _compare(eng, r, ref, cnt, log, net, w, host, label, first=0):
    """Replica r's records [first, dec_count) and counters against the stepped oracle `ref`."""
    want = ref.records()
    c = cnt[r]
    assert int(c["error"]) == 0, (label, r, int(c["error"]))
    assert int(c["dec_count"]) == first + len(want), (label, r, int(c["dec_count"]), first + len(want))
    n = min(len(want), eng.log_capacity)
    got = eng.records(r, first + len(want) - n, n, log_host=log)
    bad = first_difference(got, want[len(want) - n:])
    assert bad is None, (f"{label} replica {r}: record {first + len(want) - n + bad} differs\n engine {got[bad]}\n "
                         f"oracle {want[len(want) - n + bad]}")
    if net is not None:
        check_near_ties(net, w, host, got)
    return got


def _run_case(oracle_mod, topo, params, kind, *, label, kernel=None, R=2, launches=LAUNCHES, eps=None, seed=21):
    net, w = _net(topo, kind, seed)
    host = LQ.HostMLP(oracle_mod, topo, kind)
    thr = None if eps is None else explore.thresholds(eps)
    H = sum(launches)
    eng = PrismaEngine(topo, params, R)
    refs = []
    try:
        ki = eng.kernel_info()
        assert ki["ctrl"] == 0, ki
        if kernel is not None:
            assert {k: ki[k] for k in kernel} == kernel, (label, ki)
        eng.reset(0)
        _, mask, _ = eng.step(None)                       # a decision pending at the first launch's start
        assert bool(mask.all())
        dev = torch.from_numpy(w).cuda()
        for h in launches:
            eng.run(dev, h, model=kind, explore=eps)
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(R):
            ref = LQ.HostStepped(oracle_mod, topo, params, params["replica_base"] + r, host, w, thr=thr)
            assert ref.advance(H) == H
            assert int(cnt[r]["hops_total"]) == H, (label, r, int(cnt[r]["hops_total"]))
            got = _compare(eng, r, ref, cnt, log, None if eps is not None else net, w, host, label)
            if eps is not None:
                # the decisions the rule left to the policy (draw at or above the threshold) against torch
                greedy = np.ones(len(got), dtype=bool)
                greedy[ref.explored_at] = False
                assert len(got) == ref.n_records() and greedy.sum() > 100
                check_near_ties(net, w, host, got[greedy])
            assert_counters_equal(cnt[r], ref.counters(), r, f" ({label})")
            refs.append(ref)
    finally:
        eng.close()
    assert sum(int(ref.counters()["ov_lost"]) for ref in refs) > 0, (label, "no packet was dropped: raise the load")
    return refs


# ---- 1. Abilene: instance (2, 1), 4 waves per SIMD ---------------------------------------
@pytest.mark.parametrize("ping", [0, 1])
@pytest.mark.parametrize("kind", NEW_KINDS)
def test_abilene_every_kind(oracle_mod, kind, ping):
    topo = _topo("abilene", 3.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=ping, replica_base=4094, log_capacity=LOG)
    _run_case(oracle_mod, topo, params, kind, label=f"abilene {kind} ping {ping}",
              kernel=dict(flow_slots=2, link_slots=1, tunnels=0))


# ---- 2. GEANT: instance (8, 2), 2 waves per SIMD ---------------------------------------------
@pytest.mark.parametrize("kind", ["buffer_lite", "buffer_lighter_3"])
def test_geant(oracle_mod, kind):
    topo = _topo("geant", 2.0)
    params = engine_params(topo, sim_time_s=30.0, replica_base=5, log_capacity=LOG)
    _run_case(oracle_mod, topo, params, kind, label=f"geant {kind}", kernel=dict(flow_slots=8, link_slots=2, tunnels=0))


# ---- 3. stars: hub degrees off the chunk size, past 4 B, past four Wb chunks, the degree limit --
@pytest.mark.parametrize("d", [5, 17, 33, 55])
@pytest.mark.parametrize("kind", ["buffer_lighter_3", "buffer_lite"])
def test_stars(oracle_mod, kind, d):
    name = f"star{d}"
    topo = S.build(name)
    params = S.case_params(name, log_capacity=LOG)
    # (init seed 22: under it the hub's action varies with its buffers in all eight cases, so its
    # buffers branch decides; under seed 21 star5's buffer_lite hub always picks one action)
    refs = _run_case(oracle_mod, topo, params, kind, label=f"{name} {kind}", seed=22,
                     kernel=dict(flow_slots=S.CASES[name]["shape"][0], link_slots=S.CASES[name]["shape"][1]))
    hub = np.concatenate([r.records() for r in refs])
    hub = hub[(hub["node"] == 0) & (hub["status"] != 3)]
    assert len(hub) > 100 and len(np.unique(hub["action"])) > 2


# ---- 4. tunnelled overlays: the one-hot row is selected by overlay index ----------------------
@pytest.mark.parametrize("name,lf", [("overlay_full_mesh_3n_abilene", 20.0), ("abilene_on_geant", 3.0)])
def test_tunnelled_overlay(oracle_mod, name, lf):
    topo = _topo(name, lf)
    assert topo.n_overlay < topo.n_nodes
    params = engine_params(topo, sim_time_s=30.0, replica_base=5, log_capacity=LOG)
    _run_case(oracle_mod, topo, params, "buffer_lighter", label=f"{name} buffer_lighter", kernel=dict(tunnels=1))


# ---- 5. an episode end inside a launch: the restart loop's copy of the event loop decides ------
def test_episode_boundary_inside_a_launch(oracle_mod):
    """2-s episodes with auto_reset at a light load (a few hundred hops per second): the second
    launch crosses every replica's episode end and spends about 300 hops in episode 1.  Episode 0
    is stepped on the CPU first; its lengths size the launches."""
    kind = "buffer_lite"
    topo = _topo("abilene", 0.2)
    params = engine_params(topo, sim_time_s=2.0, auto_reset=1, log_capacity=8192)
    net, w = _net(topo, kind)
    host = LQ.HostMLP(oracle_mod, topo, kind)
    R = 2
    ep0 = [LQ.HostStepped(oracle_mod, topo, params, r, host, w) for r in range(R)]
    h0 = [e.advance(10 ** 9) for e in ep0]
    assert all(e.over() for e in ep0) and min(h0) > 200
    launches = (min(h0) // 2, max(h0) - min(h0) // 2 + 300)
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        dev = torch.from_numpy(w).cuda()
        for h in launches:
            eng.run(dev, h, model=kind)
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(R):
            c = cnt[r]
            assert int(c["error"]) == 0 and int(c["episode"]) == 1 and int(c["hops_total"]) == sum(launches), (r, c)
            assert launches[0] < h0[r] < sum(launches)                   # the end lies inside launch 2
            base = ep0[r].n_records()
            got0 = eng.records(r, 0, base, log_host=log)
            assert first_difference(got0, ep0[r].records()) is None, (r, "episode 0")
            e1 = LQ.HostStepped(oracle_mod, topo, params, r, host, w, episode=1, base=base)
            assert e1.advance(sum(launches) - h0[r]) == sum(launches) - h0[r] >= 300
            got1 = _compare(eng, r, e1, cnt, log, net, w, host, "episode 1", first=base)
            assert np.all(got1["episode"] == 1)
            check_near_ties(net, w, host, got0)
            c1 = e1.counters().copy()
            c1["dec_count"] += base
            assert_counters_equal(c, c1, r, " (episode 1)")
    finally:
        eng.close()


# ---- 6. weights overwritten in place between two launches --------------------------------------
def test_weights_overwritten_in_place(oracle_mod):
    kind = "buffer_lighter_2"
    topo = _topo("abilene", 3.0)
    params = engine_params(topo, sim_time_s=30.0, replica_base=3, log_capacity=LOG)
    net1, w1 = _net(topo, kind, 21)
    net2, w2 = _net(topo, kind, 22)
    host = LQ.HostMLP(oracle_mod, topo, kind)
    R = 2
    eng = PrismaEngine(topo, params, R)
    try:
        eng.reset(0)
        dev = torch.from_numpy(w1).cuda()
        ptr = dev.data_ptr()
        eng.run(dev, LAUNCHES[0], model=kind)
        torch.cuda.synchronize()
        mid = eng.counters()["dec_count"].copy()
        dev.copy_(torch.from_numpy(w2))
        assert dev.data_ptr() == ptr
        eng.run(dev, LAUNCHES[1], model=kind)
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        differ = 0
        for r in range(R):
            ref = LQ.HostStepped(oracle_mod, topo, params, 3 + r, host, w1)
            assert ref.advance(LAUNCHES[0]) == LAUNCHES[0] and ref.n_records() == int(mid[r])
            ref.weights = w2
            assert ref.advance(LAUNCHES[1]) == LAUNCHES[1]
            got = _compare(eng, r, ref, cnt, log, None, None, None, "overwritten weights")
            assert_counters_equal(cnt[r], ref.counters(), r, " (overwritten weights)")
            check_near_ties(net1, w1, host, got[:int(mid[r])])
            check_near_ties(net2, w2, host, got[int(mid[r]):])
            # the second launch's decisions are not the first policy's
            same = LQ.HostStepped(oracle_mod, topo, params, 3 + r, host, w1)
            same.advance(sum(LAUNCHES))
            differ += int(first_difference(got, same.records()) is not None)
        assert differ == R
    finally:
        eng.close()


# ---- 7. prisma_run_explore ---------------------------------------------------------------------
def test_explore(oracle_mod):
    topo = _topo("abilene", 3.0)
    params = engine_params(topo, sim_time_s=30.0, replica_base=9, log_capacity=LOG)
    eps = np.array([(0.0, 1.0, 0.3, 0.05)[i % 4] for i in range(topo.n_nodes)])
    refs = _run_case(oracle_mod, topo, params, "buffer_lighter_2", label="abilene explore", eps=eps)
    for ref in refs:
        assert ref.explored > 0 and ref.changed > 0 and ref.explored < ref.hops
        rec = ref.records()
        host = ref.host
        z = rec[(rec["node"] == 0) & ((rec["status"] == 1) | (rec["status"] == 2))]     # eps 0: the greedy action
        _, a = host.mlp_q_batch(ref.weights, z["node"].astype(np.int32), z["obs"])
        assert len(z) and np.array_equal(a, z["action"])


def test_explore_tunnelled_overlay(oracle_mod):
    """The exploring reduced-model instances of a tunnelled overlay (the explore_lightq slot with
    TUN): the small full-mesh overlay on Abilene, the overlay nodes exploring."""
    topo = _topo("overlay_full_mesh_3n_abilene", 20.0)
    params = engine_params(topo, sim_time_s=30.0, replica_base=5, log_capacity=LOG)
    eps = np.where(topo.degrees > 0, 0.3, 0.0)
    refs = _run_case(oracle_mod, topo, params, "buffer_lighter", label="overlay mesh explore", eps=eps,
                     kernel=dict(tunnels=1))
    for ref in refs:
        assert ref.explored > 0 and ref.changed > 0 and ref.explored < ref.hops


# ---- 8. train_fused ------------------------------------------------------------------------------
def test_train_fused():
    from prisma_amd.env import VecRoutingEnv
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    kind = "buffer_lite"
    env = VecRoutingEnv("abilene", n_replicas=64, sim_time_s=30.0)
    tr = QRoutingTrainer(env.topo, kind, batch_size=32, buffer_size=1 << 15, seed=0, n_replicas=64, iteration_num=3000)
    seen = []
    inner = env.run

    def run(policy, hops, explore=None, model="buffer"):
        # the policy of this launch is the online networks' pack() as of now
        seen.append((model, bool(torch.equal(policy, tr.q.pack())), policy.clone()))
        return inner(policy, hops, explore=explore, model=model)
    env.run = run
    before = tr.q.pack().clone()
    losses = train_fused(env, tr, 6, 256)
    cnt = env.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 6 * 256)
    assert len(losses) == 6 and np.all(np.isfinite(losses))
    assert not torch.equal(before, tr.q.pack())
    assert [m for m, _, _ in seen] == [kind] * 6 and all(ok for _, ok, _ in seen)
    assert seen[0][2].numel() == model_floats(kind, env.topo.n_nodes, env.topo.max_deg)
    assert all(not torch.equal(seen[i][2], seen[i + 1][2]) for i in range(5))       # refreshed every launch
    k = int(tr.buffers.count.min())
    assert k > 0 and torch.all(tr.buffers.action[:, :k] < tr.deg[:, None]) and torch.all(tr.buffers.action[:, :k] >= 0)
    env.close()


# ---- 9. refusals ---------------------------------------------------------------------------------
# the library's refusals, whole: status PRISMA_ERR_CONFIG (-1) and the text.  An exploring run is
# refused by prisma_run_explore before the model is looked at.
REFUSAL_MEMORY = ("prisma error -1: PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3: the memory-resident engine has no "
                  "instances with the reduced DQN-buffer models")
REFUSAL_CTRL = ("prisma error -1: PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3: this env runs the step kernels with the "
                "ctrl paths (train, notify_dest, ns-3 streams, or a tunnelled overlay with log_capacity >= 2^18), which "
                "have no instances with the reduced DQN-buffer models")
REFUSAL_EXPLORE_MEMORY = "prisma error -1: prisma_run_explore: the memory-resident engine has no exploring instances"
REFUSAL_EXPLORE_CTRL = ("prisma error -1: prisma_run_explore: this env runs the step kernels with the ctrl paths (train, "
                        "notify_dest, ns-3 streams, or a tunnelled overlay with log_capacity >= 2^18), which have no "
                        "exploring instances")


@pytest.mark.parametrize("kw", [dict(train=1), dict(engine=PRISMA_ENGINE_MEMORY)], ids=["train", "memory-engine"])
def test_refusals(oracle_mod, kw):
    topo = _topo("abilene", 1.0)
    params = engine_params(topo, sim_time_s=1.0, **kw)
    eng = PrismaEngine(topo, params, 2)
    try:
        assert eng.kernel_info()["ctrl"] == 1 or eng.engine_kind == PRISMA_ENGINE_MEMORY
        eng.reset(0)
        for kind in NEW_KINDS:
            w = torch.from_numpy(_net(topo, kind)[1]).cuda()
            with pytest.raises(PrismaError) as err:
                eng.run(w, 100, model=kind)
            assert str(err.value) == (REFUSAL_MEMORY if "engine" in kw else REFUSAL_CTRL)
            with pytest.raises(PrismaError) as err:
                eng.run(w, 100, model=kind, explore=0.1)
            assert str(err.value) == (REFUSAL_EXPLORE_MEMORY if "engine" in kw else REFUSAL_EXPLORE_CTRL)
        # the DQN-buffer model still runs here, with and without model="buffer"
        wb = _net(topo, "buffer")[1]
        dev = torch.from_numpy(wb).cuda()
        eng.run(dev, 100)
        eng.run(dev, 100, model="buffer")
        torch.cuda.synchronize()
        cnt = eng.counters()
        assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 200)
        o = oracle_mod.OracleSim(topo, params, replica=0)
        assert o.run_mlp(wb, 200) == 200
        want = o.records()
        assert eng.records(0, 0, len(want)).tobytes() == want.tobytes()
        o.close()
    finally:
        eng.close()


def test_wrong_element_count():
    topo = _topo("abilene", 1.0)
    eng = PrismaEngine(topo, engine_params(topo, sim_time_s=1.0), 2)
    try:
        eng.reset(0)
        lite = torch.from_numpy(_net(topo, "buffer_lite")[1]).cuda()
        with pytest.raises(PrismaError, match="buffer_lighter"):
            eng.run(lite, 100, model="buffer_lighter")
        with pytest.raises(PrismaError, match="DQN-buffer"):
            eng.run(lite, 100)                            # model="buffer" by default
        with pytest.raises(PrismaError, match="buffer_lite"):
            eng.run(lite[:-1], 100, model="buffer_lite")
        with pytest.raises(PrismaError, match="model must be"):
            eng.run(lite, 100, model="buffer_ff")
        eng.run(lite, 100, model="buffer_lite")
        torch.cuda.synchronize()
        cnt = eng.counters()
        assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 100)
    finally:
        eng.close()
