"""The step-kernel sets added after tests/test_gpu_instances.py's S.VARIANTS -- lightq, explore_lightq,
smart, smart_mlp, smart_lightq and stoch (S.SET_VARIANTS) -- at every (flow_slots, link_slots) shape
and on the tunnelled shapes, bit-exact against one stepped CPU oracle per replica
(set_instance_util: nothing is read from the GPU): the case matrix of tests/synth_topology.py
through run(..., model=), run(..., explore=, action_history=) and run_stochastic.

Every case: 3 replicas from replica_base 7, a 6-s episode, a log of 8 192 records, a step(None) that
leaves a decision pending (so the first launch opens at the rule's pending-decision site), then the
variant's hops over 2 launches.  tests/test_set_instance_matrix.py checks on the CPU that each
reference reaches the boundary slots and that the variant's rule decided often enough to matter, and
keeps the ledger of which (set, shape, overlay kind) the two variant tables reach.

Then the episode-end path (the second copy of the event loop, the kernel arguments read again, the
history and routing-table pointers moved to SGPRs) off the (2, 1) shape, and the one case whose
fused-only table instance has shape (8, 4)."""
import numpy as np
import pytest
import torch

import set_instance_util as U
import synth_topology as S
from parity_util import assert_counters_equal, check_near_ties, first_difference, run_fused_both
from prisma_amd.engine import PRISMA_ENGINE_REGISTER, PrismaEngine
from test_gpu_lightq import _compare

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]


def _kernel(name):
    c = S.CASES[name]
    return dict(engine=PRISMA_ENGINE_REGISTER, flow_slots=c["shape"][0], link_slots=c["shape"][1],
                tunnels=int(c["kind"] == "tunnelled"), ctrl=0)


class _Run:
    """An engine of a case and the device inputs of a variant's launches."""

    def __init__(self, name, variant, params):
        self.v = S.SET_VARIANTS[variant]
        self.x = S.set_variant_inputs(name, variant)
        self.eng = PrismaEngine(S.build(name), params, S.R)
        ki = self.eng.kernel_info()
        want = _kernel(name)
        assert {k: ki[k] for k in want} == want, (name, variant, ki)
        if self.v["set"] == "stoch":
            self.dev = self.eng.stochastic_table(self.x["policy"])
        else:
            self.dev = torch.from_numpy(np.ascontiguousarray(self.x["policy"])).cuda()
        self.eps = None if self.x["eps"] is None else torch.from_numpy(self.x["eps"]).cuda()
        self.hist = self.eng.new_action_history() if self.v["smart"] else None
        self.eng.reset(0)

    def step_to_decision(self):
        _, mask, _ = self.eng.step(None)
        assert bool(mask.all())

    def launch(self, hops):
        if self.v["set"] == "stoch":
            self.eng.run_stochastic(self.dev, hops)
        else:
            self.eng.run(self.dev, hops, model=self.x["kind"] or "buffer", explore=self.eps, action_history=self.hist)

    def outputs(self):
        torch.cuda.synchronize()
        hist = None if self.hist is None else self.hist.cpu().numpy().view(np.uint32)
        return self.eng.counters(), self.eng.log_tensor().cpu().numpy(), hist


def _assert_history(got, ref, label):
    bad = np.nonzero(got != ref.hist)[0]
    assert bad.size == 0, (f"{label}: history differs at columns {bad[:8]}: engine {got[bad[:8]]}, "
                           f"host {ref.hist[bad[:8]]}")


@pytest.mark.parametrize("variant", list(S.SET_VARIANTS))
@pytest.mark.parametrize("name", list(S.IDENTITY) + list(S.TUNNELLED))
def test_set_instance_parity(oracle_mod, name, variant):
    hops = S.SET_VARIANTS[variant]["hops"]
    assert hops % 2 == 0
    run = _Run(name, variant, S.case_params(name))
    try:
        run.step_to_decision()
        for _ in range(2):
            run.launch(hops // 2)
        if U.ends_pending(variant):
            run.step_to_decision()
        cnt, log, hist = run.outputs()
        for r in range(S.R):
            label = f"{name} {variant}"
            ref = U.run_reference(oracle_mod, name, variant, r)
            assert int(cnt[r]["hops_total"]) == hops, (label, r, int(cnt[r]["hops_total"]))
            assert int(cnt[r]["dec_count"]) <= run.eng.log_capacity
            got = _compare(run.eng, r, ref, cnt, log, None, None, None, label)
            assert_counters_equal(cnt[r], ref.counters(), r, f" ({label})")
            if hist is not None:
                _assert_history(hist[r], ref, f"{label} replica {r}")
            if run.x["net"] is not None:
                left = U.policy_decisions(ref, got)
                assert len(left) > 100
                check_near_ties(run.x["net"], run.x["policy"], U.near_tie_checker(ref), left)
    finally:
        run.eng.close()


@pytest.mark.parametrize("variant", U.EPISODE_VARIANTS)
@pytest.mark.parametrize("name", list(U.EPISODE_S))
def test_episode_end_inside_a_launch(oracle_mod, name, variant):
    """auto_reset and a short episode: one launch whose budget (from the reference's own episode
    lengths) crosses every replica's episode end once and spends 300 hops or more in episode 1."""
    params, budget, e0, e1, h0 = U.episode_references(oracle_mod, name, variant)
    run = _Run(name, variant, params)
    try:
        run.launch(budget)
        if U.ends_pending(variant):
            run.step_to_decision()
        cnt, log, hist = run.outputs()
        for r in range(S.R):
            label = f"{name} {variant} over an episode end"
            c = cnt[r]
            assert int(c["error"]) == 0 and int(c["episode"]) == 1 and int(c["hops_total"]) == budget, (label, r, c)
            base = e0[r].n_records()
            assert int(c["dec_count"]) <= run.eng.log_capacity
            got0 = run.eng.records(r, 0, base, log_host=log)
            bad = first_difference(got0, e0[r].records())
            assert bad is None, f"{label} replica {r}: record {bad} of episode 0 differs"
            got1 = _compare(run.eng, r, e1[r], cnt, log, None, None, None, label, first=base)
            assert np.all(got1["episode"] == 1)
            want = e1[r].counters().copy()
            want["dec_count"] += base
            assert_counters_equal(c, want, r, f" ({label})")
            if hist is not None:
                _assert_history(hist[r], e1[r], f"{label} replica {r}")
    finally:
        run.eng.close()


def test_fused_instance_of_shape_8_4(oracle_mod):
    """S.LDS_TABLE_8_4: (8, 4) with the action table in LDS, so run() with a table launches the
    fused-only instance of that shape (every other (8, 4) case keeps its table in HBM)."""
    name = S.LDS_TABLE_8_4
    eng = PrismaEngine(S.build(name), S.case_params(name), 1)
    try:
        assert eng.kernel_name == "prisma_step_kernel_fused_t<8, 4, false, false>"
    finally:
        eng.close()
    run_fused_both(oracle_mod, S.build(name), S.case_params(name), S.R, S.H, ("table", S.case_table(name)), launches=2,
                   kernel=_kernel(name), label=f"{name} fused")
