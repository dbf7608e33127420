"""History-weighted ("smart") exploration inside the fused kernels (prisma_run_explore_smart)
against the CPU oracle stepped under the same rule with a host history of its own
(smart_explore_util.SmartSteppedOracle: nothing is read from the GPU): records byte for byte, the
counters, and the device history against the host's; the refusals; train_fused with the trainer's
history.  Every case asserts a floor on its own reference (explored, changed, picks that differ
from the uniform pick), so an unweighted implementation cannot pass unnoticed."""
import functools

import numpy as np
import pytest
import torch

from prisma_amd import explore
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaEngine, PrismaError
from prisma_amd.topology import Topology, sp_next_hop_table

import synth_topology
from parity_util import assert_counters_equal
from smart_explore_util import SmartSteppedOracle, histogram, history_rows

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

LOG = 16384
HUGE = 1 << 30


@functools.lru_cache(maxsize=None)
def _topo(name):
    return Topology.example(name, 0, 1.0)


def _reference(oracle_mod, topo, params, R, thr, policy, hist=None):
    return [SmartSteppedOracle(oracle_mod, topo, params, params["replica_base"] + r, thr, policy,
                               hist=None if hist is None else hist[r]).run() for r in range(R)]


def _device_hist(hist):
    """The device history's bits as uint32 counts on the host."""
    torch.cuda.synchronize()
    return hist.cpu().numpy().view(np.uint32)


def _compare_whole_episode(eng, refs, hist, label):
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    got_hist = _device_hist(hist)
    for r, ref in enumerate(refs):
        c = cnt[r]
        assert int(c["error"]) == 0, (label, r, int(c["error"]))
        assert int(c["episode_over"]) == 1, (label, r)
        want = ref.records()
        assert int(c["dec_count"]) == len(want) <= eng.log_capacity, (label, r, int(c["dec_count"]), len(want))
        got = eng.records(r, 0, len(want), log_host=log)
        if got.tobytes() != want.tobytes():
            bad = next(i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes())
            raise AssertionError(f"{label} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {want[bad]}")
        assert_counters_equal(c, ref.counters(), r, f" ({label})")
        if not np.array_equal(got_hist[r], ref.hist):
            bad = np.nonzero(got_hist[r] != ref.hist)[0]
            raise AssertionError(f"{label} replica {r}: history differs at columns {bad[:8]}: engine "
                                 f"{got_hist[r][bad[:8]]}, host {ref.hist[bad[:8]]}")


def test_layout_and_new_history():
    for name in ("abilene", "abilene_on_geant"):
        topo = _topo(name)
        eng = PrismaEngine(topo, engine_params(topo, sim_time_s=1.0), 3)
        row, total = eng.action_history_layout()
        assert row.dtype == np.int32 and np.array_equal(row, history_rows(topo)) and total == int(topo.degrees.sum())
        h = eng.new_action_history()
        assert h.shape == (3, total) and h.dtype == torch.int32 and h.is_cuda and bool((h == 1).all())
        assert bool((eng.new_action_history(fill=7) == 7).all())
        eng.close()
    assert (_topo("abilene_on_geant").degrees == 0).any()  # empty rows for the nodes outside the overlay


_abilene_ref = {}


def _abilene_case(oracle_mod):
    """Cases 1 and 2 share scenario and reference: node i explores with eps 0.05 i, history of ones."""
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=2.0, replica_base=5, log_capacity=LOG)
    eps = 0.05 * np.arange(topo.n_nodes)
    table = sp_next_hop_table(topo)
    if "refs" not in _abilene_ref:
        _abilene_ref["refs"] = _reference(oracle_mod, topo, params, 4, explore.thresholds(eps), ("table", table))
        for ref in _abilene_ref["refs"]:
            print(f"abilene reference: {ref.decisions} decisions, {ref.explored} explored, {ref.changed} changed, "
                  f"{ref.differing} differ from the uniform pick")
    for ref in _abilene_ref["refs"]:
        assert ref.explored > 100 and ref.changed > 50 and ref.differing > 30
    return topo, params, eps, table, _abilene_ref["refs"]


def test_table_per_node_eps_one_launch(oracle_mod):
    topo, params, eps, table, refs = _abilene_case(oracle_mod)
    eng = PrismaEngine(topo, params, 4)
    assert eng.kernel_info()["ctrl"] == 0
    hist = eng.new_action_history()
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), HUGE, explore=torch.from_numpy(eps).cuda(), action_history=hist)
    _compare_whole_episode(eng, refs, hist, "abilene table")
    for ref in refs:                                       # the history is ones plus what the records say
        assert np.array_equal(ref.hist.astype(np.int64), 1 + histogram(topo, ref.records()))
    eng.close()


def test_table_split_across_launches(oracle_mod):
    """step(None) first: the first fused launch finishes a pending decision through the rule (the
    first hook site); then 257 hops per launch, the history carried in the caller's buffer."""
    topo, params, eps, table, refs = _abilene_case(oracle_mod)
    eng = PrismaEngine(topo, params, 4)
    hist = eng.new_action_history()
    eng.reset(0)
    _, mask, _ = eng.step(None)
    assert bool(mask.all())
    dev = torch.from_numpy(table).cuda()
    for launch in range(200):
        eng.run(dev, 257, explore=eps, action_history=hist)
        if all(int(c["episode_over"]) for c in eng.counters()):
            break
    else:
        raise AssertionError("200 launches of 257 hops did not end a 2 s episode")
    assert launch > 3
    _compare_whole_episode(eng, refs, hist, "abilene table, 257-hop launches")
    eng.close()


def test_extremes(oracle_mod):
    topo = _topo("abilene")
    table = sp_next_hop_table(topo)
    dev = torch.from_numpy(table).cuda()
    params = engine_params(topo, sim_time_s=1.0, log_capacity=LOG)
    row = history_rows(topo)
    eng = PrismaEngine(topo, params, 2)
    # eps 1 everywhere, each node's action 0 starting at 1000 and the others at 1
    start = np.ones((2, int(row[-1])), dtype=np.uint32)
    start[:, row[:-1]] = 1000
    hist = torch.from_numpy(start.view(np.int32)).cuda()
    eng.reset(0)
    eng.run(dev, HUGE, explore=1.0, action_history=hist)
    refs = _reference(oracle_mod, topo, params, 2, explore.thresholds(np.ones(topo.n_nodes)), ("table", table), hist=start)
    for ref in refs:
        share = np.mean([a == 0 for _, a, hit in ref.taken if hit])
        print(f"eps 1: {ref.explored} explored, {ref.differing} differ from the uniform pick, action 0 share {share:.3f}")
        assert ref.explored == ref.decisions > 500 and ref.differing > 300 and share < 0.15
    _compare_whole_episode(eng, refs, hist, "eps 1")
    # eps 0 with a history: prisma_run's records, and the history counts them
    hist = eng.new_action_history(fill=3)
    eng.reset(0)
    eng.run(dev, HUGE, explore=0.0, action_history=hist)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    got_hist = _device_hist(hist)
    for r in range(2):
        o = oracle_mod.OracleSim(topo, params, replica=r)
        o.run_table(table, 10 ** 9)
        want = o.records()
        assert int(cnt[r]["error"]) == 0 and int(cnt[r]["dec_count"]) == len(want)
        assert eng.records(r, 0, len(want), log_host=log).tobytes() == want.tobytes()
        assert_counters_equal(cnt[r], o.counters(), r, " (eps 0)")
        assert np.array_equal(got_hist[r].astype(np.int64), 3 + histogram(topo, want))
    eng.close()


def test_dqn_buffer_and_reduced_model(oracle_mod):
    from prisma_amd.policies import StackedQNet
    import lightq_util as LQ
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.5, log_capacity=LOG)
    thr = explore.thresholds(np.full(topo.n_nodes, 0.3))
    for kind in ("buffer", "buffer_lighter_3"):
        w = StackedQNet(topo, kind, seed=11).pack()
        wh = w.cpu().numpy()
        policy = ("mlp", wh) if kind == "buffer" else ("host", (LQ.HostMLP(oracle_mod, topo, kind), wh))
        eng = PrismaEngine(topo, params, 2)
        hist = eng.new_action_history()
        eng.reset(0)
        eng.run(w, HUGE, explore=0.3, model=kind, action_history=hist)
        refs = _reference(oracle_mod, topo, params, 2, thr, policy)
        for ref in refs:
            print(f"{kind}: {ref.explored} explored, {ref.changed} changed, {ref.differing} differ from the uniform pick")
            assert ref.explored > 200 and ref.changed > 100 and ref.differing > 30
        _compare_whole_episode(eng, refs, hist, f"abilene {kind}")
        eng.close()


def test_tunnelled_overlay(oracle_mod):
    topo = _topo("abilene_on_geant")
    params = engine_params(topo, sim_time_s=1.5, log_capacity=LOG)
    table = sp_next_hop_table(topo)
    eps = np.where(topo.degrees > 0, 0.3, 0.0)
    eng = PrismaEngine(topo, params, 2)
    ki = eng.kernel_info()
    assert ki["tunnels"] == 1 and ki["ctrl"] == 0
    row, total = eng.action_history_layout()
    assert np.array_equal(row, history_rows(topo)) and (np.diff(row) == 0).any()     # rows by underlay id
    hist = eng.new_action_history()
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), HUGE, explore=eps, action_history=hist)
    refs = _reference(oracle_mod, topo, params, 2, explore.thresholds(eps), ("table", table))
    for ref in refs:
        print(f"abilene on geant: {ref.explored} explored, {ref.changed} changed, {ref.differing} differ")
        assert ref.explored > 200 and ref.changed > 100 and ref.differing > 30
    _compare_whole_episode(eng, refs, hist, "abilene on geant")
    eng.close()


@pytest.mark.parametrize("kind", ["buffer", "buffer_lighter_3"])
def test_tunnelled_overlay_models(oracle_mod, kind):
    """The smart_mlp and smart_lightq slots of a tunnelled overlay (the table one: above): the
    small full-mesh overlay on Abilene, a whole episode."""
    from prisma_amd.policies import StackedQNet
    import lightq_util as LQ
    topo = Topology.example("overlay_full_mesh_3n_abilene", 0, 10.0)
    params = engine_params(topo, sim_time_s=1.5, log_capacity=LOG)
    eps = np.where(topo.degrees > 0, 0.3, 0.0)
    w = StackedQNet(topo, kind, seed=11).pack()
    wh = w.cpu().numpy()
    policy = ("mlp", wh) if kind == "buffer" else ("host", (LQ.HostMLP(oracle_mod, topo, kind), wh))
    eng = PrismaEngine(topo, params, 2)
    ki = eng.kernel_info()
    assert ki["tunnels"] == 1 and ki["ctrl"] == 0
    hist = eng.new_action_history()
    eng.reset(0)
    eng.run(w, HUGE, explore=eps, model=kind, action_history=hist)
    refs = _reference(oracle_mod, topo, params, 2, explore.thresholds(eps), policy)
    for ref in refs:
        print(f"overlay mesh {kind}: {ref.explored} explored, {ref.changed} changed, {ref.differing} differ, "
              f"{int(ref.counters()['ov_lost'])} lost")
        assert ref.explored > 100 and ref.changed > 30 and ref.differing > 10
    _compare_whole_episode(eng, refs, hist, f"overlay mesh {kind}")
    eng.close()


def test_episode_boundary_inside_a_launch(oracle_mod):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.0, auto_reset=1, log_capacity=LOG)
    table = sp_next_hop_table(topo)
    thr = explore.thresholds(np.full(topo.n_nodes, 0.3))
    R = 2
    eng = PrismaEngine(topo, params, R)
    hist = eng.new_action_history()
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), 3000, explore=0.3, action_history=hist)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    got_hist = _device_hist(hist)
    for r in range(R):
        c = cnt[r]
        # (as in test_gpu_explore.py: episode 1 may end inside the launch as well, so records only,
        # up to the carried-over dec_count)
        assert int(c["error"]) == 0 and int(c["episode"]) >= 1 and int(c["hops_total"]) <= 3000, (r, c)
        e0 = SmartSteppedOracle(oracle_mod, topo, params, r, thr, ("table", table)).run()
        base = e0.n_records()
        total = int(c["dec_count"])
        assert base < total <= LOG
        assert eng.records(r, 0, base, log_host=log).tobytes() == e0.records().tobytes(), (r, "episode 0")
        # episode 1 (the second inlined event loop): drawn with e = 1 and the global d, on the history
        # episode 0 left
        e1 = SmartSteppedOracle(oracle_mod, topo, params, r, thr, ("table", table), hist=e0.hist, episode=1, base=base)
        e1.run(until_records=total - base)
        want = e1.records(0, total - base)
        assert len(want) == total - base > 100 and e1.explored > 20 and e1.differing > 2
        assert np.all(want["episode"] == 1)
        assert eng.records(r, base, total - base, log_host=log).tobytes() == want.tobytes(), (r, "episode 1")
        # every record of the launch with a valid action is counted once, over the boundary
        both = np.concatenate([e0.records(), want])
        assert np.array_equal(got_hist[r].astype(np.int64), 1 + histogram(topo, both)), (r, "history")
    eng.close()


@pytest.mark.parametrize("d", [33, 55])
def test_wide_star(oracle_mod, d):
    """A hub of degree d: the scan crosses a 16-lane row (and the 32-lane half), and with row v
    starting at (i + 1) << 21 for action i the sums need more than 32 bits."""
    topo = synth_topology.star(d, 64, 7)
    params = engine_params(topo, sim_time_s=1.0, log_capacity=LOG)
    table = sp_next_hop_table(topo)
    hub = int(np.argmax(topo.degrees))
    assert int(topo.degrees[hub]) == d and np.all(np.delete(topo.degrees, hub) == 1)
    eps = np.zeros(topo.n_nodes)
    eps[hub] = 0.5
    row = history_rows(topo)
    start = np.zeros((1, int(row[-1])), dtype=np.uint32)
    for v in range(topo.n_nodes):
        start[0, row[v]:row[v + 1]] = (np.arange(int(topo.degrees[v]), dtype=np.uint32) + 1) << 21
    eng = PrismaEngine(topo, params, 1)
    hist = torch.from_numpy(start.view(np.int32)).cuda()
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), HUGE, explore=eps, action_history=hist)
    refs = _reference(oracle_mod, topo, params, 1, explore.thresholds(eps), ("table", table), hist=start)
    ref = refs[0]
    hub_actions = {a for v, a, _ in ref.taken if v == hub}
    print(f"star {d}: {ref.explored} explored, min W 2^{np.log2(ref.min_W):.1f}, {ref.differing} differ from the uniform "
          f"pick, {sum(a >= 32 for v, a, _ in ref.taken if v == hub)} hub actions >= 32")
    assert hub_actions == set(range(d)) and ref.differing > 80 and ref.min_W >= 1 << 32
    assert all(v == hub for v, _, hit in ref.taken if hit)
    _compare_whole_episode(eng, refs, hist, f"star {d}")
    eng.close()


# the library's refusals, whole: status PRISMA_ERR_CONFIG (-1) and the text
REFUSAL_MEMORY = "prisma error -1: prisma_run_explore_smart: the memory-resident engine has no exploring instances"
REFUSAL_CTRL = ("prisma error -1: prisma_run_explore_smart: this env runs the step kernels with the ctrl paths (train, "
                "notify_dest, ns-3 streams, or a tunnelled overlay with log_capacity >= 2^18), which have no exploring "
                "instances")


@pytest.mark.parametrize("kw", [dict(train=1), dict(rng="ns3"), dict(engine=PRISMA_ENGINE_MEMORY)],
                         ids=["train", "ns3-rng", "memory-engine"])
def test_refusals(kw):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.0, **kw)
    eng = PrismaEngine(topo, params, 2)
    assert eng.kernel_info()["ctrl"] == 1 or eng.engine_kind == PRISMA_ENGINE_MEMORY
    eng.reset(0)
    dev = torch.from_numpy(sp_next_hop_table(topo)).cuda()
    hist = eng.new_action_history()
    with pytest.raises(PrismaError) as err:
        eng.run(dev, 100, explore=0.1, action_history=hist)
    assert str(err.value) == (REFUSAL_MEMORY if "engine" in kw else REFUSAL_CTRL)
    assert bool((hist == 1).all())
    eng.run(dev, 100)                                      # the plain run still works
    torch.cuda.synchronize()
    cnt = eng.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 100)
    eng.close()


def test_refuses_a_wrong_history():
    topo = _topo("abilene")
    eng = PrismaEngine(topo, engine_params(topo, sim_time_s=1.0), 2)
    eng.reset(0)
    dev = torch.from_numpy(sp_next_hop_table(topo)).cuda()
    good = eng.new_action_history()
    T = good.shape[1]
    bad = [torch.ones((2, T + 1), dtype=torch.int32, device="cuda"),           # shape
           torch.ones((3, T), dtype=torch.int32, device="cuda"),
           torch.ones(2 * T, dtype=torch.int32, device="cuda"),
           torch.ones((2, T), dtype=torch.int64, device="cuda"),               # dtype
           torch.ones((2, T), dtype=torch.float32, device="cuda"),
           torch.ones((2, T), dtype=torch.int32),                              # device
           torch.ones((T, 2), dtype=torch.int32, device="cuda").t(),           # contiguity
           np.ones((2, T), dtype=np.int32)]
    for h in bad:
        with pytest.raises(PrismaError, match="prisma_run_explore_smart"):
            eng.run(dev, 100, explore=0.1, action_history=h)
    with pytest.raises(PrismaError, match="prisma_run_explore_smart"):
        eng.run(dev, 100, action_history=good)             # action_history without explore
    torch.cuda.synchronize()
    assert int(eng.counters()["hops_total"].sum()) == 0 and bool((good == 1).all())
    eng.run(dev, 100, explore=0.1, action_history=good)
    torch.cuda.synchronize()
    assert int(good.sum()) == 2 * T + int(eng.counters()["hops_total"].sum())
    eng.close()


@pytest.mark.parametrize("kind", ["routing", "buffer"])
def test_train_fused(kind):
    from prisma_amd.env import VecRoutingEnv
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    R = 64
    env = VecRoutingEnv("abilene", n_replicas=R, sim_time_s=30.0)
    tr = QRoutingTrainer(env.topo, kind, batch_size=32, buffer_size=1 << 15, seed=0, n_replicas=R,
                         iteration_num=3000, smart_exploration=True)
    T = int(env.topo.degrees.sum())
    assert tr.action_history.shape == (R, T) and tr.stats()["action_history_total"] == R * T
    losses = train_fused(env, tr, 4, 256)
    cnt = env.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 4 * 256)
    assert int(tr.buffers.total.sum()) > 0 and len(losses) == 4 and np.all(np.isfinite(losses))
    # every hop is a data decision with a valid action (uniform or weighted picks, argmins)
    assert tr.stats()["action_history_total"] == R * T + int(cnt["hops_total"].sum())
    assert int(tr.action_history.min()) >= 1
    env.close()
