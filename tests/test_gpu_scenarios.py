"""Per-replica traffic scenarios on the device (prisma_create_scenarios): every replica against one
CPU oracle on ITS OWN scenario's topology, records and counters byte for byte after every launch
(scenario_util), over the step-kernel sets, both engines, episode ends, the external step loop,
sharding, prisma_scenario_stats and train_fused.  The precondition -- the scenarios used here differ
from record 0 on, so a kernel that binds the wrong image cannot pass -- is tests/test_scenarios.py's."""
import numpy as np
import pytest
import torch

from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine
from prisma_amd.env import VecRoutingEnv
from prisma_amd.scenarios import STATS_DTYPE, STATS_F64_FIELDS, STATS_INT_FIELDS, stats_host
from prisma_amd.topology import sp_next_hop_table

from parity_util import assert_counters_equal
from scenario_util import ABILENE_4, run_explore_both, run_scenarios_both, scenario_set

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

MEM, REG = PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER


# ---- 1. the headline fused instance, with the draw cache ------------------------------------------
def test_headline_fused_instance(oracle_mod):
    sc = scenario_set("abilene", ABILENE_4)
    params = engine_params(sc.topos[0], replica_base=5)
    from prisma_amd import engine
    pl = engine.plan(sc.topos[0], params)
    assert pl["lds_bytes"] > pl["lds_state_bytes"]                 # the table sits in LDS: the fused-only instance
    cnt, _ = run_scenarios_both(oracle_mod, sc, [0, 1, 2, 3, 1, 0], params, 1000,
                                ("table", sp_next_hop_table(sc.topos[0])), launches=3, label="abilene fused",
                                kernel=dict(engine=REG, flow_slots=2, link_slots=1, tunnels=0, ctrl=0),
                                kernel_name="prisma_step_kernel_fused_t<2, 1,")
    # replicas of one scenario still differ (their Philox keys), scenarios differ in their clocks
    assert cnt[1]["now_ns"] != cnt[4]["now_ns"] and cnt[2]["now_ns"] < cnt[0]["now_ns"] < cnt[1]["now_ns"]


# ---- 2. GEANT, in-kernel DQN-buffer model (FS = 8: no draw cache) ---------------------------------
def test_geant_dqn_buffer(oracle_mod):
    from prisma_amd.policies import StackedQNet
    sc = scenario_set("geant", ((0, 1.0), (1, 0.5), (2, 2.0)))
    topo = sc.topos[0]
    params = engine_params(topo, replica_base=2)
    wh = StackedQNet(topo, "buffer", seed=3).pack().cpu().numpy()
    net_cpu = StackedQNet(topo, "buffer", seed=3, device="cpu")
    run_scenarios_both(oracle_mod, sc, [0, 1, 2], params, 1000, ("mlp", wh), launches=2, net_cpu=net_cpu,
                       label="geant mlp", kernel=dict(engine=REG, flow_slots=8, ctrl=0),
                       kernel_name="prisma_step_kernel_t<8, ")


# ---- 3. the exploring set ------------------------------------------------------------------------
def test_exploring_set(oracle_mod):
    sc = scenario_set("abilene", ((0, 1.0), (2, 2.0)))
    params = engine_params(sc.topos[0], replica_base=3)
    run_explore_both(oracle_mod, sc, [0, 1, 1, 0], params, 500, 2, 0.1, sp_next_hop_table(sc.topos[0]),
                     label="abilene explore")


# ---- 4. a tunnelled overlay ----------------------------------------------------------------------
def test_tunnelled_overlay(oracle_mod):
    sc = scenario_set("abilene_on_geant", ((0, 1.0), (3, 2.0)))
    params = engine_params(sc.topos[0], replica_base=1)
    run_scenarios_both(oracle_mod, sc, [1, 0], params, 1000, ("table", sp_next_hop_table(sc.topos[0])), launches=2,
                       label="abilene on geant", kernel=dict(engine=REG, tunnels=1, ctrl=0))


# ---- 5. the memory-resident engine ---------------------------------------------------------------
@pytest.mark.parametrize("mlp", [False, True], ids=["table", "mlp"])
def test_memory_engine(oracle_mod, mlp):
    sc = scenario_set("geant", ((0, 1.0), (1, 0.5), (2, 2.0)))
    topo = sc.topos[0]
    params = engine_params(topo, engine=MEM, replica_base=7)
    net_cpu = None
    if mlp:
        from prisma_amd.policies import StackedQNet
        pol = ("mlp", StackedQNet(topo, "buffer", seed=5).pack().cpu().numpy())
        net_cpu = StackedQNet(topo, "buffer", seed=5, device="cpu")
    else:
        pol = ("table", sp_next_hop_table(topo))
    run_scenarios_both(oracle_mod, sc, [2, 0, 1], params, 1000, pol, launches=2, net_cpu=net_cpu,
                       label=f"geant memory engine {pol[0]}", kernel=dict(engine=MEM))


# ---- 6. episode ends with auto_reset: the spare image and reset mode 3 bind the scenario too -------
@pytest.mark.parametrize("kind,launches", [(REG, 1), (MEM, 3)], ids=["register", "memory"])
def test_episode_ends_with_auto_reset(oracle_mod, kind, launches):
    sc = scenario_set("abilene", ((2, 2.0), (1, 0.5)))
    params = engine_params(sc.topos[0], sim_time_s=0.75, auto_reset=1, engine=kind, replica_base=5)
    cnt, chains = run_scenarios_both(oracle_mod, sc, [0, 1, 1], params, 3000, ("table", sp_next_hop_table(sc.topos[0])),
                                     launches=launches, label=f"auto_reset engine {kind}", kernel=dict(engine=kind))
    # a 3 000-hop launch holds more than two episodes of either scenario.  Register engine: the first
    # end continues from the spare image inside the launch, the second stops the replica and reset
    # mode 3 starts episode 2.  Memory engine: one episode per launch.
    assert [int(c["episode"]) for c in cnt] == ([2, 2, 2] if kind == REG else [3, 3, 3])
    for r, ch in chains.items():
        assert len(ch.done) >= 2
        # the episodes' lengths are their own scenario's (973 hops at tm2 / 2.0, 229 at tm1 / 0.5 for
        # replica 5; the others of the scenario are close)
        hops = [int(c["hops"]) for _, _, c in ch.done]
        assert all(700 < h < 1300 for h in hops) if r == 0 else all(120 < h < 400 for h in hops), (r, hops)


# ---- 7. the external step loop -------------------------------------------------------------------
@pytest.mark.parametrize("extra", [{}, {"train": 1}, {"rng": "ns3"}], ids=["plain", "train", "ns3"])
def test_external_step_loop(oracle_mod, extra):
    sc = scenario_set("abilene", ((0, 1.0), (2, 2.0)))
    topo = sc.topos[0]
    params = engine_params(topo, sim_time_s=10.0, replica_base=4, **extra)
    so = [0, 1, 1, 0]
    R = len(so)
    eng = PrismaEngine(topo, params, R, scenarios=sc, scenario_of=so)
    assert eng.kernel_info()["ctrl"] == (1 if extra else 0)
    eng.reset(0)
    orcs = [oracle_mod.OracleSim(sc.topos[so[r]], params, replica=4 + r) for r in range(R)]
    ref_obs = [o.step(-1) for o in orcs]
    obs, mask, node = eng.step(None)
    rng = np.random.default_rng(1)
    for s in range(300):
        g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
        acts = np.zeros(R, dtype=np.int32)
        for r in range(R):
            assert ref_obs[r] is not None and m[r] == 1, (s, r)
            assert np.array_equal(ref_obs[r], g[r]), (s, r, g[r], ref_obs[r])
            assert nd[r] == orcs[r].pending_node()
            acts[r] = rng.integers(0, topo.degrees[nd[r]] + (1 if rng.random() < 0.05 else 0))
        ref_obs = [orcs[r].step(int(acts[r])) for r in range(R)]
        obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    for r in range(R):
        ref = orcs[r].records()
        assert eng.records(r, 0, len(ref), log_host=log).tobytes() == ref.tobytes(), r
        assert_counters_equal(cnt[r], orcs[r].counters(), r)
    eng.close()


# ---- 8. S = 1 is prisma_create -------------------------------------------------------------------
def test_one_scenario_equals_create():
    sc = scenario_set("abilene", ((1, 1.5),))
    topo = sc.topos[0]
    params = engine_params(topo, replica_base=9)
    table = torch.from_numpy(sp_next_hop_table(topo)).cuda()
    out = []
    for kw in ({}, dict(scenarios=sc, scenario_of=[0, 0, 0])):
        eng = PrismaEngine(topo, params, 3, **kw)
        assert eng.n_scenarios == 1 and eng.scenario_of_host.tolist() == [0, 0, 0]
        eng.reset(0)
        for _ in range(2):
            eng.run(table, 700)
        torch.cuda.synchronize()
        out.append((eng.state_bytes, eng.lds_bytes, eng.kernel_info(), eng.counters().tobytes(),
                    eng.log_tensor().cpu().numpy().tobytes(), eng.scenario_stats().cpu().numpy().tobytes()))
        eng.close()
    assert out[0] == out[1]


# ---- 9. sharding ---------------------------------------------------------------------------------
def test_shards_equal_the_unsharded_env():
    sc = scenario_set("abilene", ABILENE_4)
    topo = sc.topos[0]
    table = torch.from_numpy(sp_next_hop_table(topo)).cuda()

    def run(base, n):
        params = engine_params(topo, replica_base=base)
        env = VecRoutingEnv(scenarios=sc, n_replicas=n, replica_base=base)
        assert env.params == params and env.topo is sc.topos[0] and env.scenarios is sc
        assert env.engine.scenario_of.cpu().tolist() == sc.assign(n, replica_base=base).tolist()
        env.reset()
        for _ in range(2):
            env.run(table, 600)
        torch.cuda.synchronize()
        res = env.counters(), env.engine.log_tensor().cpu().numpy()
        env.close()
        return res

    cnt, log = run(0, 6)
    for base, n in ((0, 4), (4, 2)):
        c, l = run(base, n)
        assert c.tobytes() == cnt[base:base + n].tobytes(), base
        assert l.tobytes() == log[base:base + n].tobytes(), base


# ---- 10. prisma_scenario_stats -------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["running", "episodes_over"])
def test_scenario_stats(shape):
    sc = scenario_set("abilene", ((0, 1.0), (2, 2.0), (1, 0.5)))
    so = np.array([0] + [1] * 64 + [2] * 65, dtype=np.int32)
    rng = np.random.default_rng(4)
    rng.shuffle(so)                                         # scenario sizes 1, 64 and 65, interleaved
    R = len(so)
    extra = dict(sim_time_s=0.75) if shape == "episodes_over" else {}
    env = VecRoutingEnv(scenarios=sc, scenario_of=so, n_replicas=R, **extra)
    assert env.engine.n_scenarios == 3
    env.reset()
    env.run(torch.from_numpy(sp_next_hop_table(sc.topos[0])).to(env.device), 500)
    st_dev = env.engine.scenario_stats()
    assert st_dev.is_cuda and tuple(st_dev.shape) == (3, STATS_DTYPE.itemsize)
    got = st_dev.cpu().numpy().reshape(-1).view(STATS_DTYPE)
    cnt = env.counters()
    want = stats_host(cnt, so, 3)
    assert got["n_replicas"].tolist() == [1, 64, 65]
    for k in ("n_error", "n_over") + STATS_INT_FIELDS:
        assert got[k].tolist() == want[k].tolist(), k
    for s in range(3):                                      # the integer sums against numpy directly
        assert int(got["hops"][s]) == int(cnt["hops"][so == s].sum()) > 0
        assert int(got["now_ns"][s]) == int(cnt["now_ns"][so == s].sum())
    for k in STATS_F64_FIELDS:                              # bit for bit in the stated order
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert np.all(got["reward_sum"] > 0) and np.all(got["e2e_sum"] > 0)
    if shape == "episodes_over":
        # 500 hops outlast a 0.75-s episode of (tm1, 0.5) (about 229 hops) but not of (tm2, 2.0) (973)
        assert got["n_over"].tolist() == [int((cnt["episode_over"][so == s] != 0).sum()) for s in range(3)]
        assert got["n_over"][2] == 65 and got["n_over"][1] == 0
    else:
        assert got["n_over"].tolist() == [0, 0, 0]
    assert got["n_error"].tolist() == [0, 0, 0]
    d = env.scenario_stats()
    assert d["hops"].tolist() == got["hops"].tolist()
    assert np.array_equal(d["avg_e2e_delay"], got["e2e_sum"] / got["e2e_n"])
    assert d["loss_ratio"][2] <= d["loss_ratio"][0] <= d["loss_ratio"][1]
    env.close()


# ---- 11. train_fused needs no change --------------------------------------------------------------
def test_train_fused_on_a_two_scenario_env(oracle_mod):
    from explore_util import SteppedOracle
    from prisma_amd import explore
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    sc = scenario_set("abilene", ((2, 2.0), (0, 1.0)))
    so = sc.assign(8)
    out = []
    for fused in (True, False):
        env = VecRoutingEnv(scenarios=sc, n_replicas=8, sim_time_s=30.0)
        tr = QRoutingTrainer(env.topo, "routing", batch_size=32, buffer_size=1 << 14, seed=0, n_replicas=8)
        launches = []
        run0 = env.run

        def run(table, hops, explore=None, **kw):
            run0(table, hops, explore=explore, **kw)
            torch.cuda.synchronize()
            launches.append((table.cpu().numpy().copy(), explore.cpu().numpy().copy(),
                             int(env.counters()[0]["dec_count"])))
        env.run = run
        losses = train_fused(env, tr, 3, 256, fused_ingest=fused)
        torch.cuda.synchronize()
        assert len(losses) == 3
        out.append((tr, env, launches))
    (ta, ea, la), (tb, eb, _) = out
    # the buffers' totals: the device ingest against env.transitions() on the twin env
    assert int(ta.buffers.total.sum()) > 1000
    assert torch.equal(ta.buffers.total, tb.buffers.total) and torch.equal(ea._consumed, eb._consumed)
    assert torch.equal(ta.buffers.reward, tb.buffers.reward)
    # replica 0's ingested rewards are those of its own scenario's oracle under the launches' policies
    params = ea.params
    ref = SteppedOracle(oracle_mod, sc.topos[int(so[0])], params, params["replica_base"], np.zeros(sc.topos[0].n_nodes),
                        ("table", la[0][0]), scalar_check=False)
    for table, eps, dec in la:
        ref.pol, ref.thr = table, explore.thresholds(eps)
        ref.run(until_records=dec)
    n = int(ea._consumed[0])
    rec = ref.records(0, n)
    want = sorted([(int(rec["node"][p]), float(np.float32(w))) for p, w in zip(rec["prev"], rec["reward"]) if p >= 0]
                  + [(int(v), float(np.float32(params["loss_penalty"]))) for v in rec["node"][rec["status"] == 2]])
    b = ta.buffers
    mine = (b.replica == 0) & (torch.arange(b.size, device=b.count.device)[None, :] < b.count[:, None])
    got = sorted((int(u), float(w)) for u, w in zip(mine.nonzero()[:, 0].cpu(), b.reward[mine].cpu()))
    assert len(got) > 100 and got == want
    ea.close()
    eb.close()
