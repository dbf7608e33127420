"""The case matrix of tests/synth_topology.py, checked without a GPU: prisma_plan picks the
expected engine, (flow_slots, link_slots) and action-table placement for every case, the matrix
covers all 12 step-kernel shapes for every instance set, and the oracle's own run of each case
meets the conditions that make it worth a GPU parity run (tests/test_gpu_instances.py): the
boundary slots carry traffic, pings run, packets drop."""
import functools

import numpy as np
import pytest

import synth_topology as S
from prisma_amd import engine
from prisma_amd.records import ST_DROPPED, ST_ENQUEUED
from prisma_amd.topology import sp_next_hop_table


@functools.lru_cache(maxsize=None)
def _plan(name, train):
    return engine.plan(S.build(name), S.case_params(name, train=train))


@pytest.mark.parametrize("name", list(S.CASES))
def test_plan_picks_the_expected_instance(name):
    c = S.CASES[name]
    for train in (0, 1):
        p = _plan(name, train)
        assert p["engine"] == engine.PRISMA_ENGINE_REGISTER
        assert (p["flow_slots"], p["link_slots"]) == c["shape"], (name, train)
        assert int(p["lds_bytes"] > p["lds_state_bytes"]) == c["table_in_lds"][train], (name, train, p)
    topo = S.build(name)
    if c["kind"] == "synth":
        n, m, f = c["args"]
        assert (topo.n_nodes, topo.n_links, topo.n_flows) == (n, 2 * m, f)
    if c["kind"] == "star":
        assert topo.max_deg == c["args"][0] == int(topo.degrees[0])
        m = engine.plan(topo, S.case_params(name, engine=engine.PRISMA_ENGINE_MEMORY))
        assert m["engine"] == engine.PRISMA_ENGINE_MEMORY and m["obs_width"] == topo.obs_width
    if c["kind"] == "tunnelled":
        assert not topo.identity and int(topo.tun_len.max()) <= 8 and int(topo.tun_len.max()) > 1


def test_matrix_covers_every_shape_for_every_instance_set():
    """All 12 PK(...) shapes of step_kernel.h, for the lite / ctrl table, lite / ctrl MLP and
    explore instances; the action table both in LDS and in HBM for the table policy and for the
    MLP (whose activations alias the table's LDS when it is there), on both the lite and ctrl side."""
    for variant, (mlp, train, explore) in S.VARIANTS.items():
        shapes = {(p["flow_slots"], p["link_slots"]) for p in (_plan(n, train) for n in S.CASES)}
        assert sorted(shapes) == S.PK_SHAPES, (variant, sorted(set(S.PK_SHAPES) - shapes))
    for train in (0, 1):
        assert {int(_plan(n, train)["lds_bytes"] > _plan(n, train)["lds_state_bytes"]) for n in S.CASES} == {0, 1}
    # the 1-wave-per-SIMD shapes (LS = 4) and FS = 4 have identity and tunnelled cases
    assert {S.CASES[n]["shape"] for n in S.TUNNELLED} == {(4, 2), (1, 2), (4, 4)}


def test_more_than_512_flows_go_to_the_memory_engine():
    topo = S.synth(*S.MEMORY_ONLY, S.SEED)
    from prisma_amd.config import engine_params
    assert topo.n_flows == 513
    assert engine.plan(topo, engine_params(topo))["engine"] == engine.PRISMA_ENGINE_MEMORY
    with pytest.raises(engine.PrismaError, match="register-resident"):
        engine.plan(topo, engine_params(topo, engine=engine.PRISMA_ENGINE_REGISTER))


@functools.lru_cache(maxsize=None)
def _oracle_runs(name, train=0):
    """The SP-table run of the case's R replicas on the oracle alone: (records, counters) each."""
    import oracle as O
    O.build()
    topo = S.build(name)
    params = S.case_params(name, train=train)
    table = sp_next_hop_table(topo)
    out = []
    for r in range(S.R):
        o = O.OracleSim(topo, params, replica=S.REPLICA_BASE + r)
        got = o.run_table(table, S.H)
        out.append((got, o.records(), o.counters()))
        o.close()
    return out


@pytest.mark.parametrize("name", list(S.CASES))
def test_oracle_run_exercises_the_boundaries(name):
    topo = S.build(name)
    c = S.CASES[name]
    for train in (0, 1):
        for got, recs, cnt in _oracle_runs(name, train):
            assert got == S.H == int(cnt["hops"]) and int(cnt["episode_over"]) == 0 and int(cnt["error"]) == 0
            assert int(cnt["ping_rounds"]) >= 3
            assert len(recs) <= S.LOG
    recs = np.concatenate([r for _, r, _ in _oracle_runs(name)])
    # the last occupied flow slot: a first-hop record of one of its flows
    flow_of = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(topo.flow_src, topo.flow_dst))}
    first = recs[recs["prev"] == -1]
    idx = np.array([flow_of[(int(a), int(b))] for a, b in zip(first["node"], first["dst"])])
    last_flow_slot = (topo.n_flows - 1) >> 6
    assert (idx >> 6 == last_flow_slot).any(), (name, "no flow of the last occupied slot has sent")
    if (topo.n_flows - 1) >> 6 == c["shape"][0] - 1:
        assert idx.max() >= 64 * (c["shape"][0] - 1)
    if c["kind"] == "tunnelled":
        return
    # the last slot with switch links: a packet forwarded over one of its links, and, where a whole
    # node lies in it, a decision at such a node
    dec = recs[(recs["status"] == ST_ENQUEUED) | (recs["status"] == ST_DROPPED)]
    out_link = topo.row_ptr[dec["node"]] + dec["action"]
    s = S.last_switch_slot(topo)
    assert (out_link >> 6 == s).any(), (name, "no packet forwarded over a link of switch slot", s)
    if (topo.row_ptr[:-1] >> 6 == s).any():
        assert (topo.row_ptr[dec["node"]] >> 6 == s).any()
    # slots past it hold access links only (link 64 of the 65-link case): a flow sourced there has sent
    acc = S.access_only_nodes(topo)
    if len(acc):
        assert np.isin(first["node"], acc).any(), (name, "no flow sourced behind the last slot's access links")
    if c["kind"] == "star":
        # the hub's last observation word (its last action's buffer; lane 63 of the record store at
        # degree 55) is non-zero at least once, with the buffer and with the ping observation
        d = c["args"][0]
        for ping in (0, 1):
            import oracle as O
            o = O.OracleSim(topo, S.case_params(name, ping_as_obs=ping), replica=S.REPLICA_BASE)
            o.run_table(sp_next_hop_table(topo), S.H)
            hub = o.records()
            hub = hub[hub["node"] == 0]
            assert (1 + d + 3) & ~3 == hub["obs"].shape[1] and (hub["obs"][:, d] != 0).any(), (name, ping)
            assert (hub["obs"][:, d + 1:] == 0).all()


def test_half_of_the_identity_cases_drop():
    dropping = [n for n in S.IDENTITY
                if any((r["status"] == ST_DROPPED).any() for _, r, _ in _oracle_runs(n))]
    assert 2 * len(dropping) >= len(S.IDENTITY), dropping


@pytest.mark.parametrize("name,ma_size,cached", S.DCACHE_CASES)
def test_draw_cache_layout_cases(name, ma_size, cached):
    """The cases test_gpu_instances.py runs with the draw cache laid out and not: 8 B per cached
    send delay and flow, only at FS <= 2."""
    assert S.dcache_bytes(name, ma_size=ma_size) == cached * 8 * S.build(name).n_flows
    assert cached == 0 or S.CASES[name]["shape"][0] <= 2
    p = engine.plan(S.build(name), S.case_params(name, ma_size=ma_size))
    assert (p["flow_slots"], p["link_slots"]) == S.CASES[name]["shape"]


def test_big_signalling_case_takes_two_flow_slots():
    p = engine.plan(S.build("l64_f64"), S.case_params("l64_f64", train=1, signaling_type="NN", big_signaling=1,
                                                        sync_step_s=0.25))
    assert S.build("l64_f64").n_flows == 64 and (p["flow_slots"], p["link_slots"]) == (2, 1)
