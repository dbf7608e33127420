"""Both engines against the CPU oracle, bit-exact, at link, buffer, packet and ping parameters away
from the reference's defaults: the case matrix of tests/param_cases.py.  Wire capacities of 2 to 64
slots on the register-resident engine and 2 to 16 on the memory-resident one (its 64-word link
record from 8 up), ping-back rings of 2 to 64 slots, FIFOs that hold 0, 1 and 300 data packets,
moving-average windows of 1 and 64 words, explicit loss penalties, an episode that ends inside the
run; through the lite / ctrl table and MLP instances, the tunnelled and the exploring ones and the
external-policy step loop.

Every case: 3 replicas from replica_base 7, 3 000 hops (9 000 at 64-B packets, of which the last
8 192 records are compared) over 2 launches, a log of 8 192 records;
tests/test_param_matrix.py checks on the CPU that each case's run fills the wires, FIFOs and
windows it is here for."""
import numpy as np
import pytest
import torch

import param_cases as P
from prisma_amd import explore
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER, PrismaEngine
from prisma_amd.records import ST_DROPPED

from explore_util import SteppedOracle
from parity_util import assert_counters_equal, first_difference, run_fused_both

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SHAPES = {"abilene": (2, 1), "geant": (8, 2), "abilene_on_geant": (2, 1)}      # (flow_slots, link_slots)
ENGINES = {"register": PRISMA_ENGINE_REGISTER, "memory": PRISMA_ENGINE_MEMORY}


def _kernel(name, tname, engine):
    """The prisma_kernel_info fields a case must report: the ctrl instances with --train."""
    ctrl = P.case_params(name, tname)["train"]
    if engine == PRISMA_ENGINE_MEMORY:
        return dict(engine=engine, ctrl=ctrl)
    return dict(engine=engine, flow_slots=SHAPES[tname][0], link_slots=SHAPES[tname][1],
                tunnels=int(tname == P.TUNNELLED), ctrl=ctrl)


def _both(oracle_mod, name, tname, pol, engine, **kw):
    return run_fused_both(oracle_mod, P.case_topo(name, tname), P.case_params(name, tname, engine=engine, **kw), P.R,
                          P.CASES[name]["hops"],
                          P.policy(tname, pol), launches=2, kernel=_kernel(name, tname, engine),
                          net_cpu=P.net(tname)[0] if pol == "mlp" else None, label=f"{name} {tname} {pol} engine {engine}")


def _ids(runs):
    return ["-".join(r) for r in runs]


@pytest.mark.parametrize("name,tname,pol", P.REGISTER_RUNS, ids=_ids(P.REGISTER_RUNS))
def test_register_engine(oracle_mod, name, tname, pol):
    _both(oracle_mod, name, tname, pol, PRISMA_ENGINE_REGISTER)


@pytest.mark.parametrize("name,tname,pol", P.MEMORY_RUNS, ids=_ids(P.MEMORY_RUNS))
def test_memory_engine(oracle_mod, name, tname, pol):
    """Wire capacities 2, 4, 8 and 16: the 32-word link record and, from 8 slots, the 64-word one."""
    _both(oracle_mod, name, tname, pol, PRISMA_ENGINE_MEMORY)


@pytest.mark.parametrize("name", P.TUNNELLED_RUNS)
def test_tunnelled(oracle_mod, name):
    """Abilene on GEANT under a random table with the ping observation: rings in multiples of
    max(WCAP, 4) behind the 4-slot LDS FIFO windows, drops inside tunnels."""
    _, refs = _both(oracle_mod, name, P.TUNNELLED, "table", PRISMA_ENGINE_REGISTER, ping_as_obs=1)
    if name.startswith("buf54"):
        assert all((r["status"] == ST_DROPPED).any() for r in refs)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_loss_penalty_reaches_the_sums(oracle_mod, engine):
    """A penalty of 0 and one of 12.5 on Abilene: the same records (the table policy takes no
    notice of rewards), and reward_sum and cost_sum apart by 12.5 per dropped packet, the fp32
    cost sum within its rounding (a running sum of a few thousand terms of up to 12.5).  A dropped
    record's own reward field is its arrival's; the penalty is booked in the sums alone."""
    (c0, r0), (c1, r1) = (_both(oracle_mod, n, "abilene", "table", ENGINES[engine]) for n in ("penalty0", "penalty12_5"))
    for r in range(P.R):
        assert r0[r].tobytes() == r1[r].tobytes()
        drops = int((r0[r]["status"] == ST_DROPPED).sum())
        lost = int(c1[r]["ov_lost"])
        assert drops > 300 and lost >= drops and lost == int(c0[r]["ov_lost"])
        assert abs(float(c1[r]["reward_sum"]) - float(c0[r]["reward_sum"]) - 12.5 * drops) < 1e-6
        assert abs(float(c1[r]["cost_sum"]) - float(c0[r]["cost_sum"]) - 12.5 * lost) < 1e-3 * 12.5 * lost


def _eps(topo):
    """Per-node epsilons: 0, 1 and values between by overlay index, 0 off the overlay."""
    eps = np.zeros(topo.n_nodes)
    eps[topo.overlay_nodes] = [(0.0, 1.0, 0.3, 0.05)[i % 4] for i in range(topo.n_overlay)]
    return eps


@pytest.mark.parametrize("pol", ["table", "mlp"])
@pytest.mark.parametrize("name,tname", P.EXPLORE_RUNS)
def test_exploring_kernels(oracle_mod, name, tname, pol):
    """run(..., explore=eps) for H hops over 2 launches, then step(None) to the next pending
    decision, against an oracle stepped H decisions under the same rule (SteppedOracle): every
    record, the pending one included, and the counters byte for byte."""
    topo, params = P.case_topo(name, tname), P.case_params(name, tname)
    policy = P.policy(tname, pol)
    eps = _eps(topo)
    thr = explore.thresholds(eps)
    eng = PrismaEngine(topo, params, P.R)
    try:
        ki = eng.kernel_info()
        want = _kernel(name, tname, PRISMA_ENGINE_REGISTER)
        assert {k: ki[k] for k in want} == want, ki
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(policy[1])).cuda()
        dev_eps = torch.from_numpy(eps).cuda()
        for _ in range(2):
            eng.run(dev, P.H // 2, explore=dev_eps)
        _, mask, _ = eng.step(None)
        torch.cuda.synchronize()
        assert bool(mask.all())
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(P.R):
            ref = SteppedOracle(oracle_mod, topo, params, P.REPLICA_BASE + r, thr, policy, scalar_check=False)
            for _ in range(P.H):
                assert ref.step()
            assert ref.explored > 100 and ref.changed > 50 and ref.explored < ref.decisions
            want = ref.records()
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["hops_total"]) == P.H
            assert int(cnt[r]["dec_count"]) == len(want) <= eng.log_capacity
            got = eng.records(r, 0, len(want), log_host=log)
            bad = first_difference(got, want)
            assert bad is None, f"{name} {tname} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {want[bad]}"
            assert_counters_equal(cnt[r], ref.counters(), r, f" ({name} {tname}, explore)")
    finally:
        eng.close()


@pytest.mark.parametrize("name,tname,engine", P.STEP_RUNS, ids=_ids(P.STEP_RUNS))
def test_external_step_loop(oracle_mod, name, tname, engine):
    """prisma_step with random actions (2 % out of range: discarded) for 300 steps after 1 500
    fused hops, then 300 fused hops again."""
    topo = P.case_topo(name, tname)
    params = P.case_params(name, tname, engine=ENGINES[engine])
    table = P.table(tname)
    eng = PrismaEngine(topo, params, P.R)
    try:
        ki = eng.kernel_info()
        want = _kernel(name, tname, ENGINES[engine])
        assert {k: ki[k] for k in want} == want, ki
        eng.reset(0)
        dev = torch.from_numpy(table).cuda()
        eng.run(dev, P.H // 2)
        orcs = [oracle_mod.OracleSim(topo, params, replica=P.REPLICA_BASE + r) for r in range(P.R)]
        for o in orcs:
            assert o.run_table(table, P.H // 2) == P.H // 2
        ref_obs = [o.step(-1) for o in orcs]
        obs, mask, node = eng.step(None)
        rng_a = np.random.default_rng(1)
        for s in range(300):
            g, m, nd = obs.cpu().numpy(), mask.cpu().numpy(), node.cpu().numpy()
            acts = np.zeros(P.R, dtype=np.int32)
            for r in range(P.R):
                assert ref_obs[r] is not None and m[r] == 1, (s, r)
                assert np.array_equal(ref_obs[r], g[r]), (s, r, g[r], ref_obs[r])
                assert nd[r] == orcs[r].pending_node()
                acts[r] = rng_a.integers(0, topo.degrees[nd[r]] + (1 if rng_a.random() < 0.02 else 0))
            ref_obs = [orcs[r].step(int(acts[r])) for r in range(P.R)]
            obs, mask, node = eng.step(torch.from_numpy(acts).cuda())
        eng.run(dev, 300)                        # the pending decision is finished by the table
        torch.cuda.synchronize()
        cnt = eng.counters()
        log = eng.log_tensor().cpu().numpy()
        for r in range(P.R):
            assert orcs[r].run_table(table, 300) == 300
            ref = orcs[r].records()
            assert int(cnt[r]["error"]) == 0 and int(cnt[r]["dec_count"]) == len(ref) <= eng.log_capacity
            got = eng.records(r, 0, len(ref), log_host=log)
            bad = first_difference(got, ref)
            assert bad is None, f"{name} replica {r}: record {bad} differs\n engine {got[bad]}\n oracle {ref[bad]}"
            assert_counters_equal(cnt[r], orcs[r].counters(), r, f" ({name} step loop)")
    finally:
        eng.close()
