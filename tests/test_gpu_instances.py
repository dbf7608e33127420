"""Every (flow_slots, link_slots) instance of the register-resident step kernel against the CPU
oracle, bit-exact: the case matrix of tests/synth_topology.py (all 12 shapes at their slot
boundaries, tunnelled overlays, stars up to the widest record) through the lite / ctrl table and
MLP instances and the explore ones, the external-policy step loop, ns-3 streams, the draw cache
laid out and not, big signalling at 64 flows, and the stars on the memory-resident engine too.

Every case: 3 replicas from replica_base 7, a 6-s episode, 3 000 hops over 2 launches, a log of
8 192 records; tests/test_instance_matrix.py checks on the CPU that each case's run reaches the
boundary slots.

S.VARIANTS drives seven of the thirteen step-kernel sets (ctrl, ctrl_mlp, lite, lite_mlp, explore,
explore_mlp, and fused where the table sits in LDS).  The other six -- lightq, explore_lightq, smart,
smart_mlp, smart_lightq, stoch -- have a variant table of their own, S.SET_VARIANTS, run over the
same cases by tests/test_gpu_set_instances.py; the ledger of which (set, shape, overlay kind) the two
tables reach together is tests/test_set_instance_matrix.py's test_ledger_every_set_reaches_every_shape."""
import functools

import numpy as np
import pytest
import torch

import synth_topology as S
from prisma_amd import explore
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine
from prisma_amd.topology import sp_next_hop_table

from explore_util import SteppedOracle
from parity_util import assert_counters_equal, first_difference, run_fused_both

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]


@functools.lru_cache(maxsize=None)
def _table(name):
    return sp_next_hop_table(S.build(name))


@functools.lru_cache(maxsize=None)
def _net(name):
    """The torch DQN-buffer model of a case on the CPU and its packed weights (numpy)."""
    from prisma_amd.policies import StackedQNet
    net = StackedQNet(S.build(name), "buffer", seed=21, device="cpu")
    return net, net.pack().numpy()


def _policy(name, mlp):
    return ("mlp", _net(name)[1]) if mlp else ("table", _table(name))


def _kernel(name, ctrl, engine=PRISMA_ENGINE_REGISTER):
    """The instance tests/test_instance_matrix.py sees prisma_plan pick."""
    c = S.CASES[name]
    if engine == PRISMA_ENGINE_MEMORY:
        return dict(engine=engine, ctrl=ctrl)
    return dict(engine=engine, flow_slots=c["shape"][0], link_slots=c["shape"][1],
                tunnels=int(c["kind"] == "tunnelled"), ctrl=ctrl)


def _eps(topo):
    """Per-node epsilons: 0, 1 and values between by overlay index, 0 off the overlay."""
    eps = np.zeros(topo.n_nodes)
    eps[topo.overlay_nodes] = [(0.0, 1.0, 0.3, 0.05)[i % 4] for i in range(topo.n_overlay)]
    return eps


def _run_explore(oracle_mod, name, mlp):
    """run(..., explore=eps) for H hops over 2 launches, then step(None) to the next pending
    decision: the state of an oracle stepped H decisions under the same rule (SteppedOracle), so
    every record, the pending one included, and the counters compare byte for byte."""
    topo, params = S.build(name), S.case_params(name)
    policy = _policy(name, mlp)
    eps = _eps(topo)
    thr = explore.thresholds(eps)
    assert thr.min() == 0 and thr.max() == 1 << 24
    eng = PrismaEngine(topo, params, S.R)
    try:
        ki = eng.kernel_info()
        want = _kernel(name, 0)
        assert {k: ki[k] for k in want} == want, ki
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(policy[1])).cuda()
        dev_eps = torch.from_numpy(eps).cuda()
        for _ in range(2):
            eng.run(dev, S.H // 2, explore=dev_eps)
        _, mask, _ = eng.step(None)
        torch.cuda.synchronize()
        assert bool(mask.all())
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(S.R):
            ref = SteppedOracle(oracle_mod, topo, params, S.REPLICA_BASE + r, thr, policy, scalar_check=False)
            for _ in range(S.H):
                assert ref.step()
            assert ref.explored > 100 and ref.changed > 50 and ref.explored < ref.decisions
            want = ref.records()
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["hops_total"]) == S.H
            assert int(cnt[r]["dec_count"]) == len(want) <= eng.log_capacity
            got = eng.records(r, 0, len(want), log_host=log)
            bad = first_difference(got, want)
            assert bad is None, f"{name} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {want[bad]}"
            assert_counters_equal(cnt[r], ref.counters(), r, f" ({name}, explore)")
    finally:
        eng.close()


@pytest.mark.parametrize("variant", list(S.VARIANTS))
@pytest.mark.parametrize("name", list(S.IDENTITY) + list(S.TUNNELLED))
def test_instance_parity(oracle_mod, name, variant):
    mlp, train, expl = S.VARIANTS[variant]
    if expl:
        return _run_explore(oracle_mod, name, mlp)
    run_fused_both(oracle_mod, S.build(name), S.case_params(name, train=train), S.R, S.H, _policy(name, mlp),
                   launches=2, kernel=_kernel(name, train), net_cpu=_net(name)[0] if mlp else None,
                   label=f"{name} {variant}")


@pytest.mark.parametrize("engine", [PRISMA_ENGINE_REGISTER, PRISMA_ENGINE_MEMORY], ids=["register", "memory"])
@pytest.mark.parametrize("pol", ["table_buf", "table_ping", "mlp"])
@pytest.mark.parametrize("d", S.STAR_DEGREES)
def test_star_parity(oracle_mod, d, pol, engine):
    """Hub degrees at the edges of mlp_action's layer-1 chunk paths and at the widest record
    (degree 55: the last observation word in lane 63 of the record store), on both engines."""
    name = f"star{d}"
    params = S.case_params(name, engine=engine, ping_as_obs=int(pol != "table_buf"))
    mlp = pol == "mlp"
    _, refs = run_fused_both(oracle_mod, S.build(name), params, S.R, S.H, _policy(name, mlp), launches=2,
                             kernel=_kernel(name, 0, engine), net_cpu=_net(name)[0] if mlp else None,
                             label=f"{name} {pol} engine {engine}")
    hub = np.concatenate([r[r["node"] == 0] for r in refs])
    assert hub["obs"].shape[1] == (1 + d + 3) & ~3 and (hub["obs"][:, d] != 0).any()


STEP_CASES = ["l256_f129", "l64_f257", "l65_f65", "l129_f64"]          # (4,4) (8,1) (2,2) (1,4)


@pytest.mark.parametrize("ping,rng", [(0, "philox"), (1, "philox"), (1, "ns3")])
@pytest.mark.parametrize("name", STEP_CASES)
def test_external_step_loop(oracle_mod, name, ping, rng):
    """prisma_step with random actions (2 % out of range: discarded) for 300 steps, after 1 500
    fused hops have every flow of the first half second running, then 300 fused hops again."""
    topo = S.build(name)
    params = S.case_params(name, ping_as_obs=ping, rng=rng)
    table = _table(name)
    eng = PrismaEngine(topo, params, S.R)
    try:
        ki = eng.kernel_info()
        assert (ki["flow_slots"], ki["link_slots"]) == S.CASES[name]["shape"] and ki["ctrl"] == int(rng == "ns3")
        eng.reset(0)
        dev = torch.from_numpy(table).cuda()
        eng.run(dev, S.H // 2)
        orcs = [oracle_mod.OracleSim(topo, params, replica=S.REPLICA_BASE + r) for r in range(S.R)]
        for o in orcs:
            assert o.run_table(table, S.H // 2) == S.H // 2
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
        eng.close()


@pytest.mark.parametrize("name,ma_size,cached", S.DCACHE_CASES)
def test_draw_cache_laid_out_and_not(oracle_mod, name, ma_size, cached):
    """The flows' draw cache is a layout decision (two cached send delays per flow, one, or none:
    where it costs no replica per CU, and never at FS >= 4): the same topology at moving-average
    windows under which prisma_plan lays it out and does not, each against the oracle."""
    assert S.dcache_bytes(name, ma_size=ma_size) == cached * 8 * S.build(name).n_flows
    for mlp in (0, 1):
        run_fused_both(oracle_mod, S.build(name), S.case_params(name, ma_size=ma_size), S.R, S.H, _policy(name, mlp),
                       launches=2, kernel=_kernel(name, 0), label=f"{name} ma_size {ma_size} mlp {mlp}")


def test_big_signalling_pushes_64_flows_to_two_slots(oracle_mod):
    """64 flows fill slot 0; the big-signalling generators' shared event slot is the 65th: FS = 2."""
    name = "l64_f64"
    params = S.case_params(name, train=1, signaling_type="NN", big_signaling=1, sync_step_s=0.25)
    cnt, _ = run_fused_both(oracle_mod, S.build(name), params, S.R, S.H, _policy(name, 0), launches=2,
                            kernel=dict(engine=PRISMA_ENGINE_REGISTER, flow_slots=2, link_slots=1, ctrl=1),
                            label="l64_f64 big signalling")
    assert np.all(cnt["bytes_signaling"] > 0)
