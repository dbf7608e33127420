"""The memory-resident engine's case matrix (tests/synth_topology.py MEMORY_CASES), checked without
a GPU: prisma_plan picks the memory engine with the recorded event-tree shape (Lk, FG, n_lb, n_fb,
n_top) and the LDS image that shape gives, the top level's 64 lanes are the refusal boundary, and
the oracle's own run of each case meets the conditions that make it worth a GPU parity run
(tests/test_gpu_mem_instances.py): the boundary leaves carry events, pings run, and the slow and
idle cases really leave every key more than 2^32 ns ahead of the clock."""
import functools

import numpy as np
import pytest

import synth_topology as S
from prisma_amd import engine
from prisma_amd.records import ST_DROPPED, ST_ENQUEUED

MEM = engine.PRISMA_ENGINE_MEMORY
# two first-hop records of one flow this far apart: its sends were more than 2^32 ns (4.295 s) apart,
# with 0.2 s of margin for what the access link in front of the first hop can add
SLOW_GAP_NS = 4_500_000_000


def test_matrix_names_the_issue_s_cases():
    assert set(S.MEM_IDENTITY) == set(S.IDENTITY)
    assert {"m_f513", "m_f4096", "m_f4097", "m_top64", "m_bsig65", "m_bsig4097", "m_slow65", "m_idle", "m_g1slow",
            "m_bsig65_slow"} <= set(S.MEM_NEW)
    assert S.MEM_NEW["m_f513"]["args"] == S.MEMORY_ONLY
    for name, c in S.MEMORY_CASES.items():
        assert c["hops"] is None or c["hops"] <= 16000, name
    # Lk and FG on both sides of one and of two blocks, and of the register engine's limits
    lk = {c["shape"][0] for c in S.MEMORY_CASES.values()}
    fg = {c["shape"][1] for c in S.MEMORY_CASES.values()}
    assert {64, 65, 128, 129, 256, 4032} <= lk and {64, 65, 128, 129, 256, 257, 512, 513, 4096, 4097} <= fg
    # the top level full, with one flow group in lane 63
    assert S.MEM_NEW["m_top64"]["shape"][2:] == (63, 10, 64)


@pytest.mark.parametrize("name", list(S.MEMORY_CASES))
def test_plan_picks_the_memory_engine_with_the_recorded_tree(name):
    c = S.MEMORY_CASES[name]
    topo = S.build_mem(name)
    assert topo.identity
    for train in sorted({0, 1, c["params"].get("train", 0)}):
        if c["params"].get("big_signaling") and not train:
            continue                               # big signalling is a --train option
        for rng in ("philox", "ns3"):
            params = S.mem_params(name, train=train, rng=rng)
            p = engine.plan(topo, params)
            assert p["engine"] == MEM and p["flow_slots"] == 0 and p["link_slots"] == 0
            shape = S.tree_shape(topo, params["big_signaling"])
            assert shape == c["shape"], (name, shape)
            assert shape[0] == topo.n_links + topo.n_nodes and shape[4] <= 64
            assert p["lds_state_bytes"] == S.mem_lds_state_bytes(shape, topo.obs_width, ns3=rng == "ns3"), (name, p)
            assert p["lds_bytes"] == p["lds_state_bytes"]            # the action table stays in HBM
    if S.MEMORY_CASES[name]["shape"][1] > 512:
        from prisma_amd.config import engine_params
        assert engine.plan(topo, engine_params(topo))["engine"] == MEM      # beyond the register engine
        with pytest.raises(engine.PrismaError, match="register-resident"):
            engine.plan(topo, S.mem_params(name, engine=engine.PRISMA_ENGINE_REGISTER))


def test_big_signalling_adds_the_generators_leaf():
    for name in ("m_bsig65", "m_bsig4097", "m_bsig65_slow"):
        topo = S.build_mem(name)
        assert S.tree_shape(topo, 0)[1] == topo.n_flows == S.MEMORY_CASES[name]["shape"][1] - 1
        assert topo.n_flows % 64 == 0
    assert S.build_mem("m_bsig4097").n_flows == 64 * 64


def test_a_65th_top_level_entry_is_refused():
    """m_top64 fills the top level (63 link blocks + 1 flow group); one more chord -- Lk = 4 034, the
    next value past 4 032 a 256-node graph can have, since Lk - n = 2 m is even -- opens link block
    63 and is refused, as are m_top64's links with a second flow group."""
    c = S.MEMORY_CASES["m_top64"]
    n, k, chords, f = c["args"]
    assert S.tree_shape(S.build_mem("m_top64"))[4] == 64
    engine.plan(S.build_mem("m_top64"), S.mem_params("m_top64"))
    from prisma_amd.config import engine_params
    more = S.circulant(n, k, chords + 1, f, c["seed"], c["rate"])
    assert S.tree_shape(more)[0] == 4034 and S.tree_shape(more)[2:] == (64, 10, 65)
    with pytest.raises(engine.PrismaError, match="64 link blocks"):
        engine.plan(more, engine_params(more, engine=MEM))
    wide = S.circulant(n, k, chords, 4097, c["seed"], c["rate"])
    assert S.tree_shape(wide)[2:] == (63, 65, 65)
    with pytest.raises(engine.PrismaError, match="64 link blocks"):
        engine.plan(wide, engine_params(wide, engine=MEM))
    # and 60 link blocks leave room for exactly 4 groups
    g = S.MEMORY_CASES["m_top64_groups"]
    over = S.circulant(*g["args"][:3], 4 * 4096 + 1, g["seed"], g["rate"])
    assert S.tree_shape(over)[2:] == (60, 257, 65)
    with pytest.raises(engine.PrismaError, match="64 link blocks"):
        engine.plan(over, engine_params(over, engine=MEM))


def test_bfs_table_follows_the_topology_s_routing():
    for name in ("m_f513", "m_top64", "m_idle"):
        topo = S.build_mem(name)
        table = S.mem_table(name)
        assert table.shape == (topo.n_nodes, topo.n_nodes) and table.dtype == np.uint8
        rng = np.random.default_rng(0)
        for u, d in rng.integers(0, topo.n_nodes, (200, 2)):
            if u != d:
                assert table[u, d] < topo.degrees[u]
                v = topo.neighbors(int(u))[table[u, d]]
                assert v == topo.next_hop[u, d] and topo.dist[v, d] == topo.dist[u, d] - 1


@functools.lru_cache(maxsize=None)
def _oracle_runs(name):
    """The case's table run of its R replicas on the oracle alone: (hops, records, counters) each."""
    import oracle as O
    O.build()
    c = S.MEMORY_CASES[name]
    topo, params, table = S.build_mem(name), S.mem_params(name), S.mem_table(name)
    out = []
    for r in range(S.R):
        o = O.OracleSim(topo, params, replica=S.REPLICA_BASE + r)
        got = o.run_table(table, c["hops"] or S.RUN_TO_END)
        out.append((got, o.records(), o.counters()))
        o.close()
    return out


def _first_hops(topo, recs):
    """(first-hop records, the flow of each)."""
    flow_of = {(int(s), int(d)): k for k, (s, d) in enumerate(zip(topo.flow_src, topo.flow_dst))}
    first = recs[recs["prev"] == -1]
    return first, np.array([flow_of[(int(a), int(b))] for a, b in zip(first["node"], first["dst"])])


@pytest.mark.parametrize("name", list(S.MEMORY_CASES))
def test_oracle_run_exercises_the_tree_s_boundaries(name):
    c = S.MEMORY_CASES[name]
    topo = S.build_mem(name)
    runs = _oracle_runs(name)
    for got, recs, cnt in runs:
        assert int(cnt["error"]) == 0 and int(cnt["ping_rounds"]) >= 3 and got == int(cnt["hops"])
        assert len(recs) <= c["log"] == S.mem_params(name)["log_capacity"]
        assert int(cnt["episode_over"]) == int(c["hops"] is None) and (c["hops"] is None or got == c["hops"])
        if c["params"].get("big_signaling"):
            assert int(cnt["bytes_signaling"]) > 0
    recs = np.concatenate([r for _, r, _ in runs])
    first, idx = _first_hops(topo, recs)
    # the last occupied flow block (partial in most cases: one flow in m_f513, m_f4097, m_slow65)
    # (m_g1slow's last block is its slow flow: silent on purpose, see its own test)
    last_block = (topo.n_flows - 1 - int(name == "m_g1slow")) >> 6
    assert (idx >> 6 == last_block).any(), (name, "no flow of the last occupied flow block has sent")
    # the last block with switch links: a packet forwarded over one of its links
    dec = recs[(recs["status"] == ST_ENQUEUED) | (recs["status"] == ST_DROPPED)]
    out_link = topo.row_ptr[dec["node"]] + dec["action"]
    s = S.last_switch_slot(topo)
    assert (out_link >> 6 == s).any(), (name, "no packet forwarded over a link of switch-link block", s)
    acc = S.access_only_nodes(topo)
    if len(acc):
        assert np.isin(first["node"], acc).any(), (name, "no flow sourced behind the last block's access links")


def test_last_flow_sends_on_every_replica_of_m_f4097():
    """The 8-launch GPU run carries block 64's and group 1's minimum across launches on every replica."""
    topo = S.build_mem("m_f4097")
    for _, recs, _ in _oracle_runs("m_f4097"):
        assert (_first_hops(topo, recs)[1] == 4096).any()
    topo = S.build_mem("m_f4096")
    assert (_first_hops(topo, np.concatenate([r for _, r, _ in _oracle_runs("m_f4096")]))[1] >> 6 == 63).any()


def test_m_top64_reaches_the_last_link_blocks():
    topo = S.build_mem("m_top64")
    assert S.last_switch_slot(topo) == 58 and len(S.access_only_nodes(topo)) == topo.n_nodes
    recs = np.concatenate([r for _, r, _ in _oracle_runs("m_top64")])
    first, _ = _first_hops(topo, recs)
    # link block 62, the last: the access links of nodes 192 .. 255
    assert ((topo.n_links + first["node"].astype(np.int64)) >> 6 == 62).any()


def test_m_top64_groups_reaches_the_last_group():
    topo = S.build_mem("m_top64_groups")
    _, idx = _first_hops(topo, np.concatenate([r for _, r, _ in _oracle_runs("m_top64_groups")]))
    assert {int(g) for g in idx >> 12} == {0, 1, 2, 3}


def test_m_slow65_leaves_block_1_beyond_32_bits_of_the_clock():
    topo = S.build_mem("m_slow65")
    assert topo.n_flows == 65 and int(topo.flow_rate_bps[64]) == 585 and (topo.flow_rate_bps[:64] == 8192).all()
    for r, (_, recs, cnt) in enumerate(_oracle_runs("m_slow65")):
        first, idx = _first_hops(topo, recs)
        t = np.sort(first["t_ns"][idx == 64].astype(np.int64))
        assert len(t) >= 2 and (np.diff(t) > SLOW_GAP_NS).any(), (r, t)
        assert int(cnt["now_ns"]) > 39 * 10 ** 9


def test_m_slow65_mlp_run_has_the_gap_within_its_hops():
    """The DQN-buffer MLP's routes are longer than the table's: 16 000 hops end at about 16 s, and
    flow 64 has its first long gap inside them on every replica."""
    import oracle as O
    from prisma_amd.policies import StackedQNet
    O.build()
    topo, params = S.build_mem("m_slow65"), S.mem_params("m_slow65")
    w = StackedQNet(topo, "buffer", seed=S.MLP_SEED, device="cpu").pack().numpy()
    for r in range(S.R):
        o = O.OracleSim(topo, params, replica=S.REPLICA_BASE + r)
        assert o.run_mlp(w, S.SLOW_MLP_HOPS) == S.SLOW_MLP_HOPS <= 16000
        recs, cnt = o.records(), o.counters()
        o.close()
        first, idx = _first_hops(topo, recs)
        t = np.sort(first["t_ns"][idx == 64].astype(np.int64))
        assert int(cnt["error"]) == 0 and len(recs) <= params["log_capacity"]
        assert (np.diff(t) > SLOW_GAP_NS).any(), (r, t)


def _trace(name, hops):
    """Per replica: the oracle's executed events (t_ns, seq, kind, id) over `hops` hops of the case's
    table run, and its clock after the case's own hops."""
    import oracle as O
    O.build()
    c = S.MEMORY_CASES[name]
    topo, params, table = S.build_mem(name), S.mem_params(name), S.mem_table(name)
    for r in range(S.R):
        o = O.OracleSim(topo, params, replica=S.REPLICA_BASE + r)
        o.enable_trace()
        o.run_table(table, c["hops"] or S.RUN_TO_END)
        t_run = int(o.counters()["now_ns"])
        o.run_table(table, hops)
        yield o.trace(), t_run, int(o.counters()["episode_over"])
        o.close()


EV_START, EV_SEND, EV_BSTART, EV_BSEND = 1, 2, 5, 6            # oracle/prisma_oracle.c


def test_m_g1slow_leaves_group_1_beyond_32_bits_of_the_clock():
    """Flow 4096's start event runs inside the case's hops and its first send lies more than 2^32 ns
    later (here: beyond the end of the 6-s episode, which the oracle is run on to)."""
    topo = S.build_mem("m_g1slow")
    assert int(topo.flow_rate_bps[4096]) == 585 and (topo.flow_rate_bps[:4096] == 4000).all()
    for tr, t_run, over in _trace("m_g1slow", S.RUN_TO_END):
        mine = tr[(tr[:, 3] == 4096) & ((tr[:, 2] == EV_START) | (tr[:, 2] == EV_SEND))]
        assert over == 1 and len(mine) >= 1 and mine[0, 2] == EV_START and mine[0, 0] < t_run
        nxt = int(mine[1, 0]) if len(mine) > 1 else int(tr[-1, 0])
        assert nxt - int(mine[0, 0]) > 1 << 32, mine[:2]


def test_m_bsig65_slow_rearms_the_generators_leaf_beyond_32_bits():
    for tr, _, over in _trace("m_bsig65_slow", 0):
        start, send = tr[tr[:, 2] == EV_BSTART], tr[tr[:, 2] == EV_BSEND]
        assert over == 1 and len(start) and len(send) == len(start)
        assert int(send[:, 0].min()) - int(start[:, 0].max()) > 1 << 32


def test_m_idle_has_a_ping_round_with_nothing_else_pending():
    iv = 7 * 10 ** 9
    assert S.mem_params("m_idle")["ping_interval_s"] == 7.0 and S.mem_params("m_idle")["sim_time_s"] == 60.0
    for r, (_, recs, cnt) in enumerate(_oracle_runs("m_idle")):
        t = recs["t_ns"].astype(np.int64)
        quiet = [k for k in range(1, 8) if not ((t > k * iv - 5 * 10 ** 8) & (t < (k + 1) * iv)).any()]
        assert quiet, (r, "every ping round has a record between 0.5 s before it and the next")
        assert int(cnt["episode_over"]) == 1 and int(cnt["ping_rounds"]) == 8
    # the register engine's select_event saturates the same way
    p = engine.plan(S.build_mem("m_idle"), S.mem_params("m_idle", engine=engine.PRISMA_ENGINE_REGISTER))
    assert p["engine"] == engine.PRISMA_ENGINE_REGISTER and (p["flow_slots"], p["link_slots"]) == (1, 1)
