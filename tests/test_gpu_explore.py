"""Epsilon-greedy exploration inside the fused kernels (prisma_run_explore) against the CPU oracle
stepped under the same rule (explore_util.SteppedOracle: nothing is read from the GPU), the
refusals, and training from the fused rollouts (trainer.train_fused)."""
import functools

import numpy as np
import pytest
import torch

from prisma_amd import explore
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaEngine, PrismaError
from prisma_amd.topology import Topology, sp_next_hop_table

from explore_util import SteppedOracle
from parity_util import assert_counters_equal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

LOG = 16384
HUGE = 1 << 30


@functools.lru_cache(maxsize=None)
def _topo(name):
    return Topology.example(name, 0, 1.0)


def _reference(oracle_mod, topo, params, R, thr, policy):
    return [SteppedOracle(oracle_mod, topo, params, params["replica_base"] + r, thr, policy).run() for r in range(R)]


def _compare_whole_episode(eng, refs, label):
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
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


_abilene_ref = {}


def _abilene_case(oracle_mod):
    """Cases 1 and 2 share scenario and reference: node i explores with eps 0.05 i."""
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=2.0, replica_base=5, log_capacity=LOG)
    eps = 0.05 * np.arange(topo.n_nodes)
    table = sp_next_hop_table(topo)
    if "refs" not in _abilene_ref:
        _abilene_ref["refs"] = _reference(oracle_mod, topo, params, 4, explore.thresholds(eps), ("table", table))
    return topo, params, eps, table, _abilene_ref["refs"]


def test_table_per_node_eps_one_launch(oracle_mod):
    topo, params, eps, table, refs = _abilene_case(oracle_mod)
    assert explore.thresholds(eps)[0] == 0
    eng = PrismaEngine(topo, params, 4)
    assert eng.kernel_info()["ctrl"] == 0
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), HUGE, explore=torch.from_numpy(eps).cuda())
    _compare_whole_episode(eng, refs, "abilene table")
    for ref in refs:
        rec = ref.records()
        assert ref.explored > 100 and ref.changed > 50
        z = rec[(rec["node"] == 0) & (rec["status"] != 3)]
        assert len(z) and np.all(z["action"] == table[0, z["dst"]])          # node 0 never explores
    eng.close()


def test_table_split_across_launches(oracle_mod):
    """step(None) first: the first fused launch finishes a pending decision through the rule (the
    first hook site); then 257 hops per launch, with a numpy array of epsilons."""
    topo, params, eps, table, refs = _abilene_case(oracle_mod)
    eng = PrismaEngine(topo, params, 4)
    eng.reset(0)
    _, mask, _ = eng.step(None)
    assert bool(mask.all())
    dev = torch.from_numpy(table).cuda()
    for launch in range(200):
        eng.run(dev, 257, explore=eps)
        if all(int(c["episode_over"]) for c in eng.counters()):
            break
    else:
        raise AssertionError("200 launches of 257 hops did not end a 2 s episode")
    assert launch > 3
    _compare_whole_episode(eng, refs, "abilene table, 257-hop launches")
    eng.close()


def test_extremes(oracle_mod):
    topo = _topo("abilene")
    table = sp_next_hop_table(topo)
    dev = torch.from_numpy(table).cuda()
    params = engine_params(topo, sim_time_s=1.0, log_capacity=LOG)
    # eps 0 everywhere: the greedy run
    eng = PrismaEngine(topo, params, 2)
    eng.reset(0)
    eng.run(dev, HUGE, explore=0.0)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    for r in range(2):
        o = oracle_mod.OracleSim(topo, params, replica=r)
        o.run_table(table, 10 ** 9)
        want = o.records()
        assert int(cnt[r]["error"]) == 0 and int(cnt[r]["dec_count"]) == len(want)
        assert eng.records(r, 0, len(want), log_host=log).tobytes() == want.tobytes()
        assert_counters_equal(cnt[r], o.counters(), r, " (eps 0)")
    # eps 1 everywhere: every decision is the uniform pick
    eng.reset(0)
    eng.run(dev, HUGE, explore=1.0)
    refs = _reference(oracle_mod, topo, params, 2, explore.thresholds(np.ones(topo.n_nodes)), ("table", table))
    assert all(ref.explored == ref.decisions > 500 for ref in refs)
    _compare_whole_episode(eng, refs, "eps 1")
    eng.close()


def test_dqn_buffer(oracle_mod):
    from prisma_amd.policies import StackedQNet
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.5, log_capacity=LOG)
    w = StackedQNet(topo, "buffer", seed=11).pack()
    wh = w.cpu().numpy()
    eng = PrismaEngine(topo, params, 3)
    eng.reset(0)
    eng.run(w, HUGE, explore=0.3)
    refs = _reference(oracle_mod, topo, params, 3, explore.thresholds(np.full(topo.n_nodes, 0.3)), ("mlp", wh))
    assert all(ref.explored > 200 and ref.changed > 100 for ref in refs)
    _compare_whole_episode(eng, refs, "abilene DQN-buffer")
    eng.close()


def test_tunnelled_overlay(oracle_mod):
    topo = _topo("abilene_on_geant")
    params = engine_params(topo, sim_time_s=1.5, log_capacity=LOG)
    table = sp_next_hop_table(topo)
    eps = np.where(topo.degrees > 0, 0.3, 0.0)
    eng = PrismaEngine(topo, params, 2)
    ki = eng.kernel_info()
    assert ki["tunnels"] == 1 and ki["ctrl"] == 0
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), HUGE, explore=torch.from_numpy(eps).float().cuda())
    # (float32 epsilons: 0.3f * 2^24 rounds to the same threshold as 0.3)
    assert explore.thresholds(np.float32(0.3)) == explore.thresholds(0.3)
    refs = _reference(oracle_mod, topo, params, 2, explore.thresholds(eps), ("table", table))
    assert all(ref.explored > 200 and ref.changed > 100 for ref in refs)
    _compare_whole_episode(eng, refs, "abilene on geant")
    eng.close()


def test_episode_boundary_inside_a_launch(oracle_mod):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.0, auto_reset=1, log_capacity=LOG)
    table = sp_next_hop_table(topo)
    thr = explore.thresholds(np.full(topo.n_nodes, 0.3))
    R = 2
    eng = PrismaEngine(topo, params, R)
    eng.reset(0)
    eng.run(torch.from_numpy(table).cuda(), 3000, explore=0.3)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    for r in range(R):
        c = cnt[r]
        # (a 1 s Abilene episode is ~1 300 hops, so episode 1 may end inside the launch as well: the
        # replica stops there, and the reset after the launch has then started episode 2, whose
        # fresh counters these are -- hence records only, up to the carried-over dec_count)
        assert int(c["error"]) == 0 and int(c["episode"]) >= 1 and int(c["hops_total"]) <= 3000, (r, c)
        e0 = SteppedOracle(oracle_mod, topo, params, r, thr, ("table", table)).run()
        base = e0.n_records()
        total = int(c["dec_count"])
        assert base < total <= LOG
        assert eng.records(r, 0, base, log_host=log).tobytes() == e0.records().tobytes(), (r, "episode 0")
        # episode 1 (the second inlined event loop): its records so far, drawn with e = 1 and the global d
        e1 = SteppedOracle(oracle_mod, topo, params, r, thr, ("table", table), episode=1, base=base)
        e1.run(until_records=total - base)
        want = e1.records(0, total - base)
        assert len(want) == total - base > 100 and e1.explored > 20
        assert np.all(want["episode"] == 1)
        assert eng.records(r, base, total - base, log_host=log).tobytes() == want.tobytes(), (r, "episode 1")
    eng.close()


# the library's refusals, whole: status PRISMA_ERR_CONFIG (-1) and the text
REFUSAL_MEMORY = "prisma error -1: prisma_run_explore: the memory-resident engine has no exploring instances"
REFUSAL_CTRL = ("prisma error -1: prisma_run_explore: this env runs the step kernels with the ctrl paths (train, "
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
    with pytest.raises(PrismaError) as err:
        eng.run(dev, 100, explore=0.1)
    assert str(err.value) == (REFUSAL_MEMORY if "engine" in kw else REFUSAL_CTRL)
    eng.run(dev, 100)                                      # the plain run still works
    torch.cuda.synchronize()
    cnt = eng.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 100)
    with pytest.raises(PrismaError, match="n_nodes"):
        eng.run(dev, 100, explore=np.zeros(3))
    eng.close()


@pytest.mark.parametrize("kind", ["routing", "buffer"])
def test_train_fused(kind):
    from prisma_amd.env import VecRoutingEnv
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    env = VecRoutingEnv("abilene", n_replicas=64, sim_time_s=30.0)
    tr = QRoutingTrainer(env.topo, kind, batch_size=32, buffer_size=1 << 15, seed=0, n_replicas=64,
                         iteration_num=3000)
    yielded = []
    inner = env.transitions
    env.transitions = lambda: yielded.append(inner()) or yielded[-1]
    eps0 = tr.explore_eps().clone()
    assert torch.all(eps0 == 1.0)
    losses = train_fused(env, tr, 6, 256)
    cnt = env.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 6 * 256)
    n = sum(int(t["node"].numel()) for t in yielded)
    assert len(yielded) == 6 and n > 0
    per_node = sum(torch.bincount(t["node"].long(), minlength=env.topo.n_nodes) for t in yielded)
    assert torch.equal(tr.buffers.total, per_node) and int(tr.buffers.total.sum()) == n
    assert torch.equal(tr.transitions_seen, per_node)
    assert len(losses) == 6 and np.all(np.isfinite(losses))
    assert torch.all(tr.explore_eps() < eps0)
    # the actions in the buffers are valid at their nodes (uniform picks while eps is 1)
    k = int(tr.buffers.count.min())
    assert k > 0 and torch.all(tr.buffers.action[:, :k] < tr.deg[:, None]) and torch.all(tr.buffers.action[:, :k] >= 0)
    env.close()
    if kind == "routing":
        small = VecRoutingEnv("abilene", n_replicas=64, sim_time_s=30.0, log_capacity=1024)
        with pytest.raises(RuntimeError, match="log_capacity"):
            train_fused(small, QRoutingTrainer(small.topo, kind, batch_size=32, n_replicas=64), 2, 4096)
        small.close()
        nn = QRoutingTrainer(env.topo, kind, batch_size=32, n_replicas=64, signaling_type="NN")
        with pytest.raises(ValueError, match="ideal"):
            train_fused(None, nn, 1, 256)
