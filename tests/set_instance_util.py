"""The references of the SET_VARIANTS matrix (tests/synth_topology.py), shared by its CPU test
(tests/test_set_instance_matrix.py: conditions on the reference alone) and its GPU test
(tests/test_gpu_set_instances.py: the engine against it): one stepped CPU oracle per replica under
the variant's rule -- lightq_util.HostStepped for the reduced models, SmartSteppedOracle for the
history-weighted exploration, OptSteppedOracle for stochastic routing -- built from
S.set_variant_inputs, so both tests see the same inputs.  Nothing is read from the GPU."""
from __future__ import annotations

import numpy as np

import lightq_util as LQ
import synth_topology as S
from opt_routing_util import OptSteppedOracle
from prisma_amd.records import ST_DROPPED, ST_ENQUEUED
from smart_explore_util import SmartSteppedOracle


def ends_pending(variant) -> bool:
    """Does the variant's reference stop at a pending decision (the smart and stoch oracles answer a
    decision and run on to the next one; HostStepped stops right after the answer, where a fused
    launch that ran out of hops stops)?  The engine then takes a step(None) after its launches."""
    return S.SET_VARIANTS[variant]["set"] in ("smart", "smart_mlp", "smart_lightq", "stoch")


def new_reference(oracle_mod, name, variant, replica, params=None, hist=None, episode=0, base=0):
    """The stepped oracle of one replica (global id `replica`) of a case under a variant's rule, at
    its start.  hist, episode, base: an episode after the first (the smart history carried over)."""
    v = S.SET_VARIANTS[variant]
    topo = S.build(name)
    params = S.case_params(name) if params is None else params
    x = S.set_variant_inputs(name, variant)
    if v["set"] == "stoch":
        return OptSteppedOracle(oracle_mod, topo, params, replica, x["policy"], episode=episode, base=base)
    if v["smart"]:
        if x["kind"] is None:
            policy = ("table", x["policy"])
        elif x["kind"] == "buffer":
            policy = ("mlp", x["policy"])
        else:
            policy = ("host", (LQ.HostMLP(oracle_mod, topo, x["kind"]), x["policy"]))
        return SmartSteppedOracle(oracle_mod, topo, params, replica, x["thr"], policy, hist=hist, episode=episode,
                                  base=base, scalar_check=False)
    return LQ.HostStepped(oracle_mod, topo, params, replica, LQ.HostMLP(oracle_mod, topo, x["kind"]), x["policy"],
                          thr=x["thr"], episode=episode, base=base)


def advance(ref, hops) -> int:
    """Up to `hops` hops of any of the three stepped oracles; the hops executed."""
    if isinstance(ref, LQ.HostStepped):
        return ref.advance(hops)
    n = 0
    while n < hops and ref.step():
        n += 1
    return n


def run_reference(oracle_mod, name, variant, r):
    """Replica r's reference after the variant's hops (asserted: no episode end on the way)."""
    ref = new_reference(oracle_mod, name, variant, S.REPLICA_BASE + r)
    hops = S.SET_VARIANTS[variant]["hops"]
    assert advance(ref, hops) == hops, (name, variant, r)
    return ref


# the episode-end runs: cases off the (2, 1) shape -- (2, 2) at 2 waves per SIMD and the tunnelled
# (4, 2) -- with auto_reset and an episode of this many seconds (a few hundred hops), under the
# variants whose kernels differ most there: the history and the routing table move through rfl_ptr
# after the kernel arguments are read again, and the reduced model decides in the second loop copy
EPISODE_S = {"l65_f65": 0.5, "tun_k14_f150": 1.0}
EPISODE_VARIANTS = ["smart_table", "smart_lightq", "stoch", "explore_lightq"]
EPISODE_EXTRA = 200                    # hops every replica spends in episode 1, at the least


def episode_references(oracle_mod, name, variant):
    """(params, budget, e0, e1, h0): every replica's episode 0 stepped to its end (h0 hops) and its
    episode 1 for the rest of one launch of `budget` hops, the longest episode 0 plus EPISODE_EXTRA
    (asserted: episode 1 does not end within it, so the launch crosses exactly one episode end)."""
    params = S.case_params(name, auto_reset=1, sim_time_s=EPISODE_S[name])
    e0 = [new_reference(oracle_mod, name, variant, S.REPLICA_BASE + r, params) for r in range(S.R)]
    h0 = [advance(e, 1 << 30) for e in e0]
    assert all(int(e.counters()["episode_over"]) == 1 and int(e.counters()["error"]) == 0 for e in e0)
    budget = max(h0) + EPISODE_EXTRA
    e1 = []
    for r in range(S.R):
        ref = new_reference(oracle_mod, name, variant, S.REPLICA_BASE + r, params, hist=getattr(e0[r], "hist", None),
                            episode=1, base=e0[r].n_records())
        assert advance(ref, budget - h0[r]) == budget - h0[r] and int(ref.counters()["episode_over"]) == 0
        e1.append(ref)
    return params, budget, e0, e1, h0


def decision_indices(records):
    """Indices of the records that carry an answered decision, in the order they were answered."""
    return np.flatnonzero((records["status"] == ST_ENQUEUED) | (records["status"] == ST_DROPPED))


def policy_decisions(ref, records):
    """The records of the decisions the rule left to the policy (for check_near_ties): every
    answered decision of a greedy run, the ones not explored of an exploring one."""
    idx = decision_indices(records)
    if isinstance(ref, LQ.HostStepped):
        return records[np.setdiff1d(idx, np.asarray(ref.explored_at, dtype=np.int64))]
    assert len(idx) == len(ref.taken) and np.array_equal(records["node"][idx], [v for v, _, _ in ref.taken])
    return records[idx[~np.array([hit for _, _, hit in ref.taken], dtype=bool)]]


def near_tie_checker(ref):
    """The `checker` of parity_util.check_near_ties for a model variant's reference."""
    if isinstance(ref, LQ.HostStepped):
        return ref.host
    return ref.o if ref.kind == "mlp" else ref.pol[0]


def boundary_failures(name, recs):
    """tests/test_instance_matrix.py test_oracle_run_exercises_the_boundaries' conditions on the R
    replicas' records of a case (concatenated): the list of the ones not met."""
    topo, c = S.build(name), S.CASES[name]
    bad = []
    flow_of = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(topo.flow_src, topo.flow_dst))}
    first = recs[recs["prev"] == -1]
    idx = np.array([flow_of[(int(a), int(b))] for a, b in zip(first["node"], first["dst"])])
    if not (idx >> 6 == (topo.n_flows - 1) >> 6).any():
        bad.append("no flow of the last occupied slot has sent")
    if (topo.n_flows - 1) >> 6 == c["shape"][0] - 1 and not idx.max() >= 64 * (c["shape"][0] - 1):
        bad.append("no flow of the shape's last slot has sent")
    if c["kind"] == "tunnelled":
        return bad
    dec = recs[decision_indices(recs)]
    s = S.last_switch_slot(topo)
    if not ((topo.row_ptr[dec["node"]] + dec["action"]) >> 6 == s).any():
        bad.append(f"no packet forwarded over a link of switch slot {s}")
    if (topo.row_ptr[:-1] >> 6 == s).any() and not (topo.row_ptr[dec["node"]] >> 6 == s).any():
        bad.append(f"no decision at a node that lies wholly in switch slot {s}")
    acc = S.access_only_nodes(topo)
    if len(acc) and not np.isin(first["node"], acc).any():
        bad.append("no flow sourced behind the last slot's access links has sent")
    return bad
