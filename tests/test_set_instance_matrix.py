"""The SET_VARIANTS matrix of tests/synth_topology.py -- the lightq, explore_lightq, smart, smart_mlp,
smart_lightq and stoch step-kernel sets over every identity and tunnelled case -- checked without a
GPU, as tests/test_instance_matrix.py checks S.VARIANTS: the stepped CPU reference of every (case,
variant), the one tests/test_gpu_set_instances.py compares the engine with (set_instance_util), meets
the conditions that make it worth a GPU parity run.  No error and no episode end, 3 ping rounds, the
boundary slots carry traffic, and the variant's rule decided often enough that a kernel without it
would write other records.  Then the ledger: which (set, shape, overlay kind) the two variant tables
reach together, from prisma_plan's answers and the library's dispatch restated.

Hops per case (S.SET_VARIANTS): 3 000 for lightq and stoch, 4 000 for the exploring variants (at 3 000
their 64-node cases stop before the third ping round).  No variant needed fewer hops than that: CPU
seconds per case (3 replicas, one core, inputs included), least - most over the 18 cases: lightq
(buffer_lite on the host restatement) 2.7 - 3.9, explore_lightq 1.7 - 2.4 and smart_lightq 1.9 - 2.5
(buffer_lighter_3), smart_mlp 0.6 - 0.8, smart_table 0.3 - 0.5, stoch 0.3 - 0.9.  The whole file: 2 min 45 s."""
import functools
import re

import numpy as np
import pytest

import lightq_util as LQ
import set_instance_util as U
import synth_topology as S
from prisma_amd import engine
from smart_explore_util import histogram
from test_step_sets import STEP_KERNEL_H, table_rows

NAMES = list(S.IDENTITY) + list(S.TUNNELLED)
# cases whose graph is a tree (m = n - 1): one path per pair, so path_split_routing's matrix is
# one-hot, no entry lies in (0, 1), no edge has a class, and the stoch rule can never follow
TREES = [n for n, c in S.IDENTITY.items() if c["args"][1] == c["args"][0] - 1]
# stoch: follows, draws and follows at an index other than 0 per replica, tests/test_gpu_opt_routing.py's
STOCH_FLOORS = (200, 200, 20)
# smart: picks that differ from the uniform pick, per replica.  On the trees most nodes have one or two
# neighbours, where the weighted and the uniform pick of one draw rarely differ: 20 there
DIFFERING_FLOOR = {n: 20 if n in TREES else 30 for n in NAMES}


def test_the_table_names_the_six_variants():
    assert TREES == ["l64_f64", "l64_f129", "l64_f257", "l40_f100"]
    assert {k: (v["set"], v["policy"], v["explore"], v["smart"]) for k, v in S.SET_VARIANTS.items()} == {
        "lightq": ("lightq", "buffer_lite", 0, 0),
        "explore_lightq": ("explore_lightq", "buffer_lighter_3", 1, 0),
        "smart_table": ("smart", "table", 1, 1),
        "smart_mlp": ("smart_mlp", "buffer", 1, 1),
        "smart_lightq": ("smart_lightq", "buffer_lighter_3", 1, 1),
        "stoch": ("stoch", "stoch", 0, 0)}
    assert LQ.DIMS["buffer_lite"][2] == 2                  # (two hidden layers)
    for v in S.SET_VARIANTS.values():
        assert v["hops"] % 2 == 0 and v["hops"] <= S.EXPLORE_H


def test_inputs_are_built_once_and_as_the_older_matrix_builds_them():
    import test_gpu_instances as G
    for name in ("l65_f65", "tun_k9_f60"):
        topo = S.build(name)
        assert np.array_equal(S.node_eps(topo), G._eps(topo))
        assert np.array_equal(S.case_table(name), G._table(name))
        a, b = S.set_variant_inputs(name, "smart_mlp"), S.set_variant_inputs(name, "smart_mlp")
        assert a["policy"] is b["policy"] and a["net"] is b["net"]
        assert np.array_equal(a["policy"], G._net(name)[1])
        assert a["thr"].min() == 0 and a["thr"].max() == 1 << 24
        assert S.set_variant_inputs(name, "stoch")["policy"] is S.case_routing(name)
    off = S.build("tun_k9_f60")
    assert off.n_overlay < off.n_nodes and S.node_eps(off)[off.degrees == 0].max() == 0


@functools.lru_cache(maxsize=None)
def _refs(name, variant):
    import oracle as O
    O.build()
    return [U.run_reference(O, name, variant, r) for r in range(S.R)]


@pytest.mark.parametrize("variant", list(S.SET_VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_worth_a_gpu_run(name, variant):
    v = S.SET_VARIANTS[variant]
    topo = S.build(name)
    refs = _refs(name, variant)
    for r, ref in enumerate(refs):
        cnt, recs = ref.counters(), ref.records()
        where = (name, variant, r)
        assert int(cnt["error"]) == 0 and int(cnt["episode_over"]) == 0 and int(cnt["hops"]) == v["hops"], where
        assert len(recs) <= S.LOG and int(cnt["ping_rounds"]) >= 3, (where, len(recs), int(cnt["ping_rounds"]))
        if v["explore"]:
            decisions = ref.hops if isinstance(ref, LQ.HostStepped) else ref.decisions
            assert decisions == v["hops"]
            assert ref.explored > 100 and ref.changed > 50 and ref.explored < decisions, (where, ref.explored, ref.changed)
        if v["smart"]:
            assert ref.differing > DIFFERING_FLOOR[name], (where, ref.differing)
            assert np.array_equal(ref.hist.astype(np.int64), 1 + histogram(topo, recs)), where
        if v["set"] == "stoch":
            got = (ref.follows, ref.draws, ref.follows_nonzero)
            floors = (0, STOCH_FLOORS[1], 0) if name in TREES else STOCH_FLOORS
            assert all(g >= f for g, f in zip(got, floors)) and ref.decisions == v["hops"], (where, got)
            assert name not in TREES or ref.follows == 0
        if v["policy"] not in ("table", "stoch"):
            assert len(U.policy_decisions(ref, recs)) > 100, where
    bad = U.boundary_failures(name, np.concatenate([ref.records() for ref in refs]))
    assert not bad, (name, variant, bad)


@pytest.mark.parametrize("variant", U.EPISODE_VARIANTS)
@pytest.mark.parametrize("name", list(U.EPISODE_S))
def test_episode_end_references(name, variant):
    """The launch of tests/test_gpu_set_instances.py test_episode_end_inside_a_launch crosses one
    episode end on every replica, stays in the log, and the rule decides in episode 1 too.  (Floors
    for about 200 - 500 hops of episode 1 and 1 300 in all, where the matrix's are for 3 000.)"""
    import oracle as O
    O.build()
    assert S.CASES[name]["shape"] != (2, 1)
    params, budget, e0, e1, h0 = U.episode_references(O, name, variant)
    assert params["auto_reset"] == 1 and budget <= S.H
    for r in range(S.R):
        assert min(h0) > 200 and U.EPISODE_EXTRA <= budget - h0[r]
        assert e0[r].n_records() + e1[r].n_records() <= S.LOG and e1[r].episode == 1 and e1[r].base == e0[r].n_records()
        assert np.all(e1[r].records()["episode"] == 1)
        if S.SET_VARIANTS[variant]["explore"]:
            assert e1[r].explored > 50 and e1[r].changed > 25, (name, variant, r, e1[r].explored, e1[r].changed)
        if S.SET_VARIANTS[variant]["smart"]:
            assert e0[r].differing + e1[r].differing > 15
            both = np.concatenate([e0[r].records(), e1[r].records()])
            assert np.array_equal(e1[r].hist.astype(np.int64), 1 + histogram(S.build(name), both))
        if variant == "stoch":
            assert e1[r].follows > 30 and e1[r].draws > 50 and e1[r].follows_nonzero > 10


# ---- the ledger ------------------------------------------------------------------------------
def _step_shapes():
    txt = open(STEP_KERNEL_H).read()
    line = next(l for l in txt.splitlines() if l.startswith("#define PRISMA_STEP_SHAPES(X)"))
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", line)]


def _launched(name, table, variant):
    """(set, (flow_slots, link_slots), tunnelled) of every step-kernel launch of a matrix run whose
    result is compared: prisma_create's and run_slot's choice (prisma_engine.hip) restated on
    prisma_plan's answers, the fused-only instances by engine.step_kernel_names' rule."""
    topo = S.build(name)
    if table == "SET_VARIANTS":
        train, sets = 0, {S.SET_VARIANTS[variant]["set"], "lite"}         # (step(None): prisma_step's set)
    else:
        mlp, train, expl = S.VARIANTS[variant]
        sets = {("explore_mlp" if mlp else "explore"), "lite"} if expl else {("ctrl_mlp" if train else "lite_mlp")}
    pl = engine.plan(topo, S.case_params(name, train=train))
    assert pl["engine"] == engine.PRISMA_ENGINE_REGISTER
    ki = dict(engine=pl["engine"], flow_slots=pl["flow_slots"], link_slots=pl["link_slots"],
              tunnels=int(not topo.identity), ctrl=train)
    if table == "VARIANTS" and not mlp and not expl:
        fused = engine.step_kernel_names(ki, pl)["table"].startswith("prisma_step_kernel_fused_t<")
        sets = {"fused" if fused else ("ctrl" if train else "lite")}
    return {(s, (ki["flow_slots"], ki["link_slots"]), ki["tunnels"]) for s in sets}


# what no case can reach, by name, with the reason
UNREACHABLE = {
    ("fused", shape, 1): "the fused-only table set has no tunnelled instances (prisma_pick_step gives null)"
    for shape in [(4, 2), (1, 2), (4, 4)]}


def test_ledger_every_set_reaches_every_shape():
    """Every row of PRISMA_STEP_SETS at every shape of PRISMA_STEP_SHAPES on an identity overlay, and
    at the three tunnelled shapes, is launched by a case of S.VARIANTS or S.SET_VARIANTS (fused (8, 4):
    by S.LDS_TABLE_8_4, the one (8, 4) case whose table sits in LDS) -- but for UNREACHABLE."""
    reached = set()
    for name in NAMES:
        for table, variants in (("VARIANTS", S.VARIANTS), ("SET_VARIANTS", S.SET_VARIANTS)):
            for variant in variants:
                reached |= _launched(name, table, variant)
    assert ("fused", (8, 4), 0) not in reached             # (l256_f512 keeps its table in HBM)
    reached |= _launched(S.LDS_TABLE_8_4, "VARIANTS", "lite_table")
    sets = [name for _, name in table_rows()]
    assert len(sets) == 13 and len(_step_shapes()) == 12
    tunnelled = sorted({S.CASES[n]["shape"] for n in S.TUNNELLED})
    assert len(tunnelled) == 3
    want = {(s, sh, 0) for s in sets for sh in _step_shapes()} | {(s, sh, 1) for s in sets for sh in tunnelled}
    assert set(UNREACHABLE) <= want and not set(UNREACHABLE) & reached
    missing = sorted(want - reached - set(UNREACHABLE))
    assert not missing, missing
    assert reached <= want, sorted(reached - want)
