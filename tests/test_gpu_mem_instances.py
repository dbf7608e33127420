"""The memory-resident engine against the CPU oracle, bit-exact, at the boundaries of its 64-ary
event tree: the case matrix of tests/synth_topology.py MEMORY_CASES.  Every identity case of the
register engine's matrix forced onto the memory engine (Lk and FG at 64, 65, 128, 129, 256, 512)
through the four prisma_mem_step_kernel<MLP, CTRL> instances, and the cases only it can hold: a
last flow block, and a last flow group, of one flow; a full top level (63 link blocks and a flow
group in lane 63; 60 link blocks and 4 groups); the big-signalling generators' leaf alone in a
block and in a group; and the saturated 32-bit key reductions of fblock_min, fgroup_min and
select_event (a slow flow alone in its block, and alone in its group beside 4 096 busy flows; the
generators' leaf with a 5-s period; a network idle between pings, on both engines).

Every case: 3 replicas from replica_base 7, the case's hops (at most 16 000 per replica, or to the
episode's end) over 2 launches; tests/test_mem_instance_matrix.py checks on the CPU that each
case's run reaches those boundaries."""
import functools

import numpy as np
import pytest
import torch

import synth_topology as S
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine

from parity_util import assert_counters_equal, first_difference, run_fused_both

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

MEM = PRISMA_ENGINE_MEMORY


@functools.lru_cache(maxsize=None)
def _net(name):
    """The torch DQN-buffer model of a case on the CPU and its packed weights (numpy)."""
    from prisma_amd.policies import StackedQNet
    net = StackedQNet(S.build_mem(name), "buffer", seed=S.MLP_SEED, device="cpu")
    return net, net.pack().numpy()


def _run(oracle_mod, name, mlp=0, launches=2, hops=None, **kw):
    """The case's hops of the table or the DQN-buffer MLP on the memory engine and on the oracle:
    every record and counter (now_ns, events, ping_rounds among them) of every replica."""
    c = S.MEMORY_CASES[name]
    params = S.mem_params(name, **kw)
    ctrl = int(bool(params["train"] or params["notify_dest"] or params["rng_mode"]))
    if hops is None:
        hops, launches = (c["hops"], launches) if c["hops"] else (S.RUN_TO_END, 1)
    return run_fused_both(oracle_mod, S.build_mem(name), params, S.R, hops,
                          ("mlp", _net(name)[1]) if mlp else ("table", S.mem_table(name)), launches=launches,
                          kernel=dict(engine=MEM, ctrl=ctrl),
                          net_cpu=_net(name)[0] if mlp else None, label=f"{name} mlp {mlp} {kw}")


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("mlp", [0, 1], ids=["table", "mlp"])
@pytest.mark.parametrize("name", list(S.MEM_IDENTITY))
def test_identity_cases_on_the_memory_engine(oracle_mod, name, mlp, train):
    _run(oracle_mod, name, mlp, train=train)


def _trains(name):
    return [1] if S.MEM_NEW[name]["params"].get("big_signaling") else [0, 1]


@pytest.mark.parametrize("name,train", [(n, t) for n in S.MEM_NEW for t in _trains(n)])
def test_new_cases_table(oracle_mod, name, train):
    cnt, _ = _run(oracle_mod, name, train=train)
    c = S.MEM_NEW[name]
    assert np.all(cnt["episode_over"] == int(c["hops"] is None)) and np.all(cnt["ping_rounds"] >= 3)
    if c["params"].get("big_signaling"):
        assert np.all(cnt["bytes_signaling"] > 0)


# m_top64: 256-way one-hot inputs.  m_slow65: the first 16 000 hops (the MLP's routes are longer than
# the table's; flow 64's first long gaps lie inside them, tests/test_mem_instance_matrix.py)
@pytest.mark.parametrize("name,hops", [("m_f513", None), ("m_top64", None), ("m_slow65", S.SLOW_MLP_HOPS)])
def test_new_cases_mlp(oracle_mod, name, hops):
    _run(oracle_mod, name, 1, hops=hops)


@pytest.mark.parametrize("name", ["m_f513", "m_f4097"])
def test_new_cases_ns3_streams(oracle_mod, name):
    _run(oracle_mod, name, rng="ns3")


def test_idle_network_on_the_register_engine(oracle_mod):
    """m_idle's quiet ping rounds saturate the register engine's select_event the same way."""
    params = S.mem_params("m_idle", engine=PRISMA_ENGINE_REGISTER)
    cnt, _ = run_fused_both(oracle_mod, S.build_mem("m_idle"), params, S.R, S.RUN_TO_END, ("table", S.mem_table("m_idle")),
                            kernel=dict(engine=PRISMA_ENGINE_REGISTER, flow_slots=1, link_slots=1, ctrl=0),
                            label="m_idle register")
    assert np.all(cnt["episode_over"] == 1) and np.all(cnt["ping_rounds"] == 8)


def test_multi_launch_carries_the_tree(oracle_mod):
    """m_f4097 in 8 launches: top_store / top_load carry 7 top lanes (5 link blocks, 2 flow groups) and
    the LDS image 65 flow block minima from launch to launch."""
    _run(oracle_mod, "m_f4097", launches=8)


@pytest.mark.parametrize("ping", [0, 1])
@pytest.mark.parametrize("name", ["m_f513", "l129_f64"])
def test_external_step_loop_on_the_memory_engine(oracle_mod, name, ping):
    """prisma_step with random actions (2 % out of range: discarded) for 300 steps, after 1 500 fused
    hops, then 300 fused hops again (tests/test_gpu_instances.py test_external_step_loop)."""
    topo, table = S.build_mem(name), S.mem_table(name)
    params = S.mem_params(name, ping_as_obs=ping)
    eng = PrismaEngine(topo, params, S.R)
    orcs = []
    try:
        ki = eng.kernel_info()
        assert ki["engine"] == MEM and ki["ctrl"] == 0
        eng.reset(0)
        dev = torch.from_numpy(table).cuda()
        eng.run(dev, 1500)
        orcs = [oracle_mod.OracleSim(topo, params, replica=S.REPLICA_BASE + r) for r in range(S.R)]
        for o in orcs:
            assert o.run_table(table, 1500) == 1500
        ref_obs = [o.step(-1) for o in orcs]
        obs, mask, node = eng.step(None)
        rng_a = np.random.default_rng(1)
        for s in range(300):
            g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
            acts = np.zeros(S.R, dtype=np.int32)
            for r in range(S.R):
                assert ref_obs[r] is not None and m[r] == 1, (s, r)
                assert np.array_equal(ref_obs[r], g[r]), (s, r, g[r], ref_obs[r])
                assert nd[r] == orcs[r].pending_node()
                acts[r] = rng_a.integers(0, topo.degrees[nd[r]] + (1 if rng_a.random() < 0.02 else 0))
            ref_obs = [orcs[r].step(int(acts[r])) for r in range(S.R)]
            obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
        eng.run(dev, 300)                        # the pending decision is finished by the table
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(S.R):
            assert orcs[r].run_table(table, 300) == 300
            ref = orcs[r].records()
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["dec_count"]) == len(ref) <= eng.log_capacity
            got = eng.records(r, 0, len(ref), log_host=log)
            bad = first_difference(got, ref)
            assert bad is None, f"{name} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {ref[bad]}"
            assert_counters_equal(cnt[r], orcs[r].counters(), r, f" ({name} step loop)")
    finally:
        for o in orcs:
            o.close()
        eng.close()
