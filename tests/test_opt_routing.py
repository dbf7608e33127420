"""Stochastic multipath routing (the reference's "opt" agent), the parts that need no GPU: the
packing of a routing matrix (classes and weights), the host restatement of the rule against a
big-integer loop and against the probabilities, the derived tag against a literal restatement of
optimal_routing_decision with an explicit per-packet tag, the rule driving the CPU oracle, and the
C-ABI entry."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from prisma_amd import config, engine, optrouting
from prisma_amd.config import engine_params
from prisma_amd.topology import Topology, sp_next_hop_table

from opt_routing_util import OptSteppedOracle, big_pick, literal_decision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _abilene():
    return Topology.example("abilene", 0, 1.0)


def _hand(topo, s, t, v, probs):
    """A routing matrix that is zero but for node v's row of (s, t)."""
    row = optrouting.edge_rows(topo)
    rt = np.zeros((topo.n_overlay, topo.n_overlay, int(row[-1])))
    rt[s, t, row[v]: row[v] + len(probs)] = probs
    return rt


def test_pack_routing_classes_and_weights():
    topo = _abilene()
    row = optrouting.edge_rows(topo)
    v = int(np.argmax(topo.degrees))
    assert int(topo.degrees[v]) == 3
    r0 = int(row[v])
    third = 1.0 / 3.0
    tab = optrouting.pack_routing(topo, _hand(topo, 2, 5, v, [third, 0.5, third]))
    e = tab[2, 5, r0:r0 + 3]
    cls, wt = e >> 24, e & 0xFFFFFF
    assert cls[0] == cls[2] == 1 and cls[1] == 2           # equal floats share a class, ascending values
    rowsum = third + 0.5 + third
    assert [int(x) for x in wt] == [int(np.floor(p / rowsum * 2 ** 24 + 0.5)) for p in (third, 0.5, third)]
    assert np.count_nonzero(tab) == 3 and tab.dtype == np.uint32 and tab.shape == (11, 11, int(row[-1]))
    # 1.0 and 0.0 get class 0; a one-hot row gives weight 2^24 - 1 (the clamp)
    e = optrouting.pack_routing(topo, _hand(topo, 0, 1, v, [0.0, 1.0, 0.0]))[0, 1, r0:r0 + 3]
    assert [int(x) for x in e] == [0, (1 << 24) - 1, 0]
    e = optrouting.pack_routing(topo, _hand(topo, 0, 1, v, [0.0, 0.25, 0.0]))[0, 1, r0:r0 + 3]
    assert [int(x) for x in e] == [0, (1 << 24) | ((1 << 24) - 1), 0]
    # values >= 1 are class 0 and still weigh; a next-representable float is another class
    e = optrouting.pack_routing(topo, _hand(topo, 0, 1, v, [2.0, 0.5, np.nextafter(0.5, 1.0)]))[0, 1, r0:r0 + 3]
    assert [int(x) >> 24 for x in e] == [0, 1, 2] and int(e[0]) == int(np.floor(2.0 / 3.0 * 2 ** 24 + 0.5))
    # classes are per (s, t), over all of its edges
    rt = _hand(topo, 3, 4, v, [0.5, 0.25, 0.25])
    u = (v + 1) % topo.n_nodes
    rt[3, 4, row[u]] = 0.125
    tab = optrouting.pack_routing(topo, rt)
    assert [int(x) >> 24 for x in tab[3, 4, r0:r0 + 3]] == [3, 2, 2] and int(tab[3, 4, row[u]]) >> 24 == 1
    assert int(tab[3, 4, row[u]]) & 0xFFFFFF == (1 << 24) - 1


def test_pack_routing_refuses():
    topo = _abilene()
    row = optrouting.edge_rows(topo)
    T = int(row[-1])
    good = np.zeros((11, 11, T))
    optrouting.pack_routing(topo, good)
    for bad in (np.zeros((11, 11, T + 1)), np.zeros((11, T)), np.zeros((10, 11, T))):
        with pytest.raises(ValueError, match="shape"):
            optrouting.pack_routing(topo, bad)
    for val in (-1e-9, np.nan):
        rt = good.copy()
        rt[1, 2, 3] = val
        with pytest.raises(ValueError):
            optrouting.pack_routing(topo, rt)
    # 256 distinct values in (0, 1) for one (s, t) raise; 255 fit
    vals = (np.arange(256) + 1) / 1000.0
    many = _many_edges()
    Tm = int(optrouting.edge_rows(many)[-1])
    assert Tm >= 256
    rt = np.zeros((many.n_overlay, many.n_overlay, Tm))
    rt[0, 1, :255] = vals[:255]
    assert int((optrouting.pack_routing(many, rt)[0, 1] >> 24).max()) == 255
    rt[0, 1, :256] = vals
    with pytest.raises(ValueError, match="255"):
        optrouting.pack_routing(many, rt)


def _many_edges():
    """A 24-node ring with chords: more than 256 directed edges."""
    n = 24
    adj = np.zeros((n, n), dtype=int)
    for i in range(n):
        for k in range(1, 7):
            adj[i, (i + k) % n] = adj[(i + k) % n, i] = 1
    tm = np.full((n, n), "10Kbps", dtype=object)
    return Topology.from_matrices(adj, tm, name="ring24")


def test_stoch_action_against_big_integers():
    rng = np.random.default_rng(5)
    fallback = 0
    for deg in range(1, 56):
        topo_row = np.array([0, deg])                      # one node of degree deg
        n = 40
        wt = rng.integers(0, 1 << 24, size=(n, deg), dtype=np.uint32)
        wt[rng.random(n) < 0.1] = 0
        one = rng.random(n) < 0.1
        wt[one] = 0
        wt[one, rng.integers(0, deg, size=int(one.sum()))] = (1 << 24) - 1
        c1 = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
        c1[0], c1[1] = 0xFFFFFFFF, 0
        for i in range(n):
            want = big_pick(c1[i], wt[i])
            assert 0 <= want < deg
            got = optrouting.stoch_pick(int(c1[i]), wt[i])
            assert isinstance(got, int) and got == want, (deg, i)
            W = int(wt[i].astype(np.uint64).sum())
            fallback += int(W == 0)
            if W:
                assert wt[i, want] > 0                     # a zero-weight edge is never drawn
        # the vectorised form over many draws of one row
        got = optrouting.stoch_pick(c1, wt[2])
        assert got.dtype == np.int64 and [int(x) for x in got] == [big_pick(c, wt[2]) for c in c1]
        # and through stoch_action with a real draw: a fresh packet at the one node
        tab = wt[3].reshape(1, 1, deg)
        a = optrouting.stoch_action(tab, topo_row, 0, 0, 0, None, 100, 7, deg, 0)
        c = optrouting.stoch_draw(100, 7, deg, 0)
        assert a == big_pick(c[1], wt[3])
    assert fallback > 100


def test_zero_weight_fallback_is_the_uniform_pick():
    from prisma_amd import explore
    d = np.arange(5000)
    c = optrouting.stoch_draw(100, 3, d, 0)
    # domain 3: other words than exploration's for the same decision
    assert not np.array_equal(c, explore.explore_draw(100, 3, d, 0))
    for deg in (1, 2, 7, 55):
        a = optrouting.stoch_pick(c[:, 1], np.zeros(deg, dtype=np.uint32))
        assert np.array_equal(a, (c[:, 1].astype(np.uint64) * np.uint64(deg)) >> np.uint64(32))
        assert a.min() == 0 and a.max() == deg - 1


def test_pick_frequencies():
    n = 1 << 16
    c1 = optrouting.stoch_draw(100, 9, np.arange(n), 2)[:, 1]
    rng = np.random.default_rng(3)
    for deg in (2, 3, 17, 55):
        wt = rng.integers(0, 1 << 24, size=deg, dtype=np.uint32)
        wt[rng.integers(0, deg)] = 0
        a = optrouting.stoch_pick(c1, wt)
        p = wt.astype(np.float64) / float(wt.astype(np.uint64).sum())
        cnt = np.bincount(a, minlength=deg)
        sigma = np.sqrt(n * p * (1 - p))
        assert np.all(np.abs(cnt - n * p) <= 5 * sigma + 1e-9), (deg, cnt, n * p)
        assert np.all(cnt[wt == 0] == 0)


def test_follow_and_draw_branches_by_hand():
    topo = _abilene()
    row = optrouting.edge_rows(topo)
    v = int(np.argmax(topo.degrees))
    u = topo.neighbors(v)[0]
    a_u = topo.neighbors(u).index(v)
    rt = _hand(topo, 1, 9, v, [0.2, 0.3, 0.3])
    rt[1, 9, row[u] + a_u] = 0.3
    tab = optrouting.pack_routing(topo, rt)
    # the previous edge's fraction 0.3 is found at index 1 first: followed, whatever the draw
    for d in range(50):
        assert optrouting.stoch_action(tab, row, 1, 9, v, (u, a_u), 100, 0, d, 0, with_branch=True) == (1, True)
    # a fresh packet, an invalid previous action and a previous edge of class 0 all draw
    seen = set()
    for d in range(200):
        for prev in (None, (u, -1), (u, 99), (u, (a_u + 1) % int(topo.degrees[u]))):
            a, followed = optrouting.stoch_action(tab, row, 1, 9, v, prev, 100, 0, d, 0, with_branch=True)
            assert not followed
            seen.add(a)
    assert seen == {0, 1, 2}
    # a tag that no edge of the node carries draws as well
    rt[1, 9, row[u] + a_u] = 0.31
    tab = optrouting.pack_routing(topo, rt)
    assert not optrouting.stoch_action(tab, row, 1, 9, v, (u, a_u), 100, 0, 0, 0, with_branch=True)[1]


_prefix = {}


def _abilene_prefix(oracle_mod):
    """One Abilene episode prefix under path_split_routing, shared by the tests below."""
    if "ref" not in _prefix:
        topo = _abilene()
        params = engine_params(topo, sim_time_s=2.0, replica_base=0, log_capacity=16384)
        rt = optrouting.path_split_routing(topo, 3, seed=1)
        _prefix["ref"] = OptSteppedOracle(oracle_mod, topo, params, 0, rt).run(until_records=3000)
    return _prefix["ref"]


def test_rule_drives_the_oracle_through_both_branches(oracle_mod):
    ref = _abilene_prefix(oracle_mod)
    print(f"abilene path-split prefix: {ref.decisions} decisions, {ref.follows} followed "
          f"({ref.follows_nonzero} at an index other than 0), {ref.draws} drawn")
    assert ref.decisions > 2000 and ref.follows > 200 and ref.draws > 200 and ref.follows_nonzero > 20
    rec = ref.records(0, 3000)
    hops = rec[rec["status"] != 3]
    assert np.all((hops["action"] >= 0) & (hops["action"] < ref.topo.degrees[hops["node"]]))
    assert (rec["status"] == 3).sum() > 300                # packets arrive: the matrix routes


def test_derived_tag_equals_the_literal_per_packet_tag(oracle_mod):
    """The reference's decision with an explicit tag per packet (keyed by uid, None at the source),
    replayed over the rule-stepped oracle's trace with the rule's own drawn index injected where
    the literal draws: the same branch and the same action at every decision."""
    ref = _abilene_prefix(oracle_mod)
    tags = {}
    follows = 0
    for e in ref.trace:
        if e["prev"] is None:
            tags[e["uid"]] = None                          # forwarder.py:350
        probs = ref.node_probs(e["s"], e["t"], e["v"])
        a, tag, followed = literal_decision(probs, tags[e["uid"]], e["action"])
        assert (a, followed) == (e["action"], e["followed"]), e
        assert e["followed"] or e["W"] > 0                 # (no zero row on this trace: the reference's crash)
        tags[e["uid"]] = tag
        follows += int(followed)
    assert follows == ref.follows > 0


def test_generators():
    for name in ("abilene", "abilene_on_geant"):
        topo = Topology.example(name, 0, 1.0)
        edges, col = optrouting.reference_edges(topo)
        assert sorted(col) == list(range(len(edges))) and edges == sorted(edges)
        ecmp = optrouting.ecmp_routing(topo)
        ps = optrouting.path_split_routing(topo, 3, seed=1)
        assert ecmp.shape == ps.shape == (topo.n_overlay, topo.n_overlay, len(edges))
        sp = sp_next_hop_table(topo)
        for s in range(topo.n_overlay):
            for t in range(topo.n_overlay):
                if s == t:
                    continue
                # flow conservation at the source: everything leaves it
                out_s = [k for k, (a, _) in enumerate(edges) if a == s]
                assert abs(ecmp[s, t, out_s].sum() - 1.0) < 1e-12 and abs(ps[s, t, out_s].sum() - 1.0) < 1e-12
                # the SP next hop is among the ECMP next hops
                u = int(topo.overlay_nodes[s])
                k = out_s[int(sp[u, int(topo.overlay_nodes[t])])]
                assert ecmp[s, t, k] > 0
        assert (ecmp == 0.5).any() and len(np.unique(ps)) > 20
        assert np.array_equal(ps, optrouting.path_split_routing(topo, 3, seed=1))
        assert not np.array_equal(ps, optrouting.path_split_routing(topo, 3, seed=2))
    # the table's columns follow the underlay ids, the matrix's the overlay indices
    topo = Topology.example("abilene_on_geant", 0, 1.0)
    assert not np.array_equal(optrouting.reference_edges(topo)[1], np.arange(topo.n_tunnels))


def test_load_optimal_solution(tmp_path):
    topo = _abilene()
    rt = optrouting.path_split_routing(topo, 2, seed=4)
    p = tmp_path / "sol.json"
    p.write_text(json.dumps({"routing": rt.tolist(), "rejected_flows": np.zeros((11, 11)).tolist()}))
    got, rej = optrouting.load_optimal_solution(str(p))
    assert np.array_equal(got, rt) and rej.shape == (11, 11)
    assert np.array_equal(optrouting.pack_routing(topo, got), optrouting.pack_routing(topo, rt))


def test_abi_entry_and_config():
    header = open(os.path.join(ROOT, "include", "prisma.h")).read()
    assert re.search(r"^int prisma_run_stochastic\(prisma_env_t\* env, const uint32_t\* tab, uint64_t tab_words,\s*"
                     r"int32_t max_hops, void\* stream\);", header, re.M)
    assert "#define PRISMA_ABI_VERSION 10" in header
    assert "prisma_run_stochastic" in engine.EXPORTS
    lib = engine.load_library()
    assert lib.prisma_abi_version() == engine.ABI_VERSION == 10
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T prisma_run_stochastic$", out, re.M)
    # a null env is a status code
    assert lib.prisma_run_stochastic(None, None, 0, 1, None) == -5
    from prisma_amd import buildid
    assert "prisma_engine_stoch.hip" in buildid.ENGINE_SOURCES
    assert config.AGENT_FUSED_KINDS["opt"] == "opt" and "opt" in config.AGENT_TYPES
    assert "opt" not in config.AGENT_MODEL_KINDS
