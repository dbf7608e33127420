"""Synthetic topologies that reach every (flow_slots, link_slots) instance of the register-resident
step kernel at its slot boundaries, and the case matrix tests/test_instance_matrix.py (CPU: the
plan and the oracle's own run) and tests/test_gpu_instances.py (GPU parity) both import, with a
second variant table for the newer instance sets (SET_VARIANTS: tests/test_set_instance_matrix.py
and tests/test_gpu_set_instances.py); then the
same for the memory-resident engine's 64-ary event tree (MEMORY_CASES, at the end of the file:
tests/test_mem_instance_matrix.py and tests/test_gpu_mem_instances.py).

numpy only, seeded, deterministic.  On an identity overlay the engine numbers the 2m directed
switch links first (CSR order) and then one access link per node, so it has 2m + n links: link
2m + v is node v's access link.  Flows are numbered in (src, dst) order.  A register slot holds 64
links / flows: slot j of a link is (index >> 6)."""
from __future__ import annotations

import functools

import numpy as np

from prisma_amd.topology import Topology

LINK_BPS = 500000


def _tree_plus_edges(n, m, rng):
    """A shallow random tree (node i hangs off a node in [(i-1)/4, (i-1)/2]: depth O(log n),
    degree <= 6 before the extra edges) plus m - (n - 1) random extra edges."""
    if not n - 1 <= m <= n * (n - 1) // 2:
        raise ValueError("m must be in [n - 1, n (n - 1) / 2]")
    adj = np.zeros((n, n), dtype=np.int64)
    for i in range(1, n):
        p = int(rng.integers((i - 1) // 4, (i - 1) // 2 + 1))
        adj[i, p] = adj[p, i] = 1
    free = [(a, b) for a in range(n) for b in range(a + 1, n) if not adj[a, b]]
    for k in rng.permutation(len(free))[:m - (n - 1)]:
        a, b = free[int(k)]
        adj[a, b] = adj[b, a] = 1
    return adj


def _pick_flows(nodes, f, rng):
    """f ordered pairs of `nodes`; every node sources at least one when f >= len(nodes)."""
    nodes = [int(v) for v in nodes]
    pairs = [(a, b) for a in nodes for b in nodes if a != b]
    if f > len(pairs):
        raise ValueError("more flows than ordered pairs")
    chosen = set()
    if f >= len(nodes):
        for a in nodes:
            others = [b for b in nodes if b != a]
            chosen.add((a, others[int(rng.integers(len(others)))]))
    rest = [p for p in pairs if p not in chosen]
    for k in rng.permutation(len(rest))[:f - len(chosen)]:
        chosen.add(rest[int(k)])
    return sorted(chosen)


def default_rate(m, f):
    """Per-flow rate that loads the 2m directed switch links to about 0.9 if every packet crossed
    three of them: hub links of the tree go over, so FIFOs fill and drop."""
    return int(0.9 * LINK_BPS * 2 * m / (3 * f))


def synth(n, m, f, seed, rate=None):
    """Identity overlay: n nodes, m undirected edges, f flows of `rate` b/s each."""
    rng = np.random.default_rng([seed, n, m, f])
    adj = _tree_plus_edges(n, m, rng)
    tm = np.zeros((n, n), dtype=object)
    for a, b in _pick_flows(range(n), f, rng):
        tm[a, b] = int(default_rate(m, f) if rate is None else rate)
    return Topology.from_matrices(adj, tm, name=f"synth{n}_{m}_{f}")


def star(d, f, seed, rate=None):
    """Hub 0 with d leaves and f leaf-to-leaf flows; leaf d (the hub's last action, whose buffer
    fills the hub's last observation word) is the destination of at least a quarter of them."""
    rng = np.random.default_rng([seed, d, f])
    n = d + 1
    adj = np.zeros((n, n), dtype=np.int64)
    adj[0, 1:] = adj[1:, 0] = 1
    leaves = list(range(1, n))
    to_last = [(a, d) for a in leaves[:-1]]
    k = min(len(to_last), max(1, f // 4))
    chosen = {to_last[int(i)] for i in rng.permutation(len(to_last))[:k]}
    rest = [(a, b) for a in leaves for b in leaves if a != b and (a, b) not in chosen]
    for i in rng.permutation(len(rest))[:f - len(chosen)]:
        chosen.add(rest[int(i)])
    tm = np.zeros((n, n), dtype=object)
    # (each leaf-to-leaf packet crosses two switch links; the links into leaf d run hot)
    r = int(0.9 * LINK_BPS * d / f) if rate is None else int(rate)
    for a, b in chosen:
        tm[a, b] = r
    return Topology.from_matrices(adj, tm, name=f"star{d}")


def tunnelled(n, m, k, f, seed, rate=None, inner=False):
    """A tree-plus-edges underlay as synth's with k overlay nodes (underlay leaves first; inner:
    inner underlay nodes first) joined as an overlay ring with one chord, f flows between overlay
    nodes.  The shallow tree keeps every tunnel at 8 links or fewer (asserted)."""
    rng = np.random.default_rng([seed, n, m, f])
    adj = _tree_plus_edges(n, m, rng)
    # underlay leaves first: no tunnel crosses them, so few overlay nodes are ping bystanders (a
    # ping-back that crosses one of lower overlay degree can carry a tunnel index beyond it, which
    # both engines and the oracle flag as PRISMA_EBIT_PINGIDX and end the episode on).  inner: the
    # opposite order, whose tunnels do cross overlay nodes (ERROR_CASES)
    order = rng.permutation(n)
    on = np.sort(np.array(sorted(order, key=lambda v: (adj[v].sum() <= 1) if inner else (adj[v].sum() > 1))[:k]))
    mapo = np.full(n, -1, dtype=np.int64)
    mapo[on] = np.arange(k)
    oadj = np.zeros((k, k), dtype=np.int64)
    for i in range(k):
        oadj[i, (i + 1) % k] = oadj[(i + 1) % k, i] = 1
    oadj[0, k // 2] = oadj[k // 2, 0] = 1
    tm = np.zeros((n, n), dtype=object)
    for a, b in _pick_flows(on, f, rng):
        tm[a, b] = int(default_rate(m, f) if rate is None else rate)
    topo = Topology.from_matrices(adj, tm, name=f"tun{n}_{m}_{k}_{f}", map_overlay=mapo, overlay_adjacency=oadj)
    assert int(topo.tun_len.max()) <= 8
    return topo


# ---- the case matrix ---------------------------------------------------------------------
# name: builder and its arguments, (flow_slots, link_slots), table_in_lds at (train=0, train=1),
# per-flow rate (None: the builder's default) and engine params beyond the common ones.  The
# shapes and table_in_lds are what prisma_plan reports (tests/test_instance_matrix.py asserts
# them).  The n = 64 cases and the widest star run at a lower rate, so that 3 000 hops span 3 ping
# rounds; the seeds of the cases with one flow alone in the last slot are ones under which that
# flow's start offset (uniform in the first second) falls inside the run.
def _c(kind, args, shape, lds, rate=None, **params):
    return dict(kind=kind, args=args, shape=shape, table_in_lds=lds, rate=rate, params=params)


def _r64(f):
    return int(0.45 * default_rate(96, f))


IDENTITY = {
    # 64 links, 64 flows: both slots exactly full
    "l64_f64": _c("synth", (22, 21, 64), (1, 1), (1, 0)),
    # 65 links: link 64 = node 20's access link, alone in slot 1; flow 64 alone in slot 1
    "l65_f65": _c("synth", (21, 22, 65), (2, 2), (1, 1)),
    "l64_f129": _c("synth", (22, 21, 129), (4, 1), (1, 1)),
    "l64_f257": _c("synth", (22, 21, 257), (8, 1), (1, 1)),
    "l128_f64": _c("synth", (30, 49, 64), (1, 2), (1, 0)),
    "l129_f128": _c("synth", (31, 49, 128), (2, 4), (1, 0)),
    "l128_f256": _c("synth", (30, 49, 256), (4, 2), (1, 0)),
    "l128_f512": _c("synth", (30, 49, 512), (8, 2), (1, 0)),
    "l129_f64": _c("synth", (43, 43, 64), (1, 4), (1, 1)),
    "l256_f65": _c("synth", (64, 96, 65), (2, 4), (0, 0), rate=_r64(65)),
    "l256_f129": _c("synth", (64, 96, 129), (4, 4), (0, 0), rate=_r64(129), seed=3),
    # every limit of the register engine at once
    "l256_f512": _c("synth", (64, 96, 512), (8, 4), (0, 0), rate=_r64(512)),
    # 256 links of which 216 are switch links: the n = 64 cases fill slot 3 with access links
    # only, here nodes decide over and observe links of slot 3
    "l256d_f130": _c("synth", (40, 108, 130), (4, 4), (1, 1), rate=int(0.5 * default_rate(108, 130))),
    "l40_f100": _c("synth", (14, 13, 100), (2, 1), (1, 1)),
    "l100_f128": _c("synth", (26, 37, 128), (2, 2), (0, 1)),
}
# tunnelled overlays of other shapes than Abilene-on-GEANT's (2, 1); about a third of the identity
# rate, since every overlay hop crosses several links
TUNNELLED = {
    "tun_k14_f150": _c("tunnelled", (40, 52, 14, 150), (4, 2), (1, 1), rate=34000),
    "tun_k9_f60": _c("tunnelled", (30, 40, 9, 60), (1, 2), (1, 1), rate=66000),
    "tun_k16_f200": _c("tunnelled", (64, 80, 16, 200), (4, 4), (1, 1), rate=40000),
}
# hub degrees at the edges of mlp_action's layer-1 chunk paths (16 | 17, 32 | 33) and at the
# widest record both engines can write (55: obs_width 56, the last word in lane 63); 3d + 1 links
STAR_DEGREES = (4, 5, 16, 17, 32, 33, 55)
_STAR_LS = {4: 1, 5: 1, 16: 1, 17: 1, 32: 2, 33: 2, 55: 4}
_STAR_LDS = {17: (1, 0)}
STARS = {f"star{d}": _c("star", (d, min(64, d * (d - 1))), (1, _STAR_LS[d]), _STAR_LDS.get(d, (1, 1)),
                        rate=int(0.6 * 0.9 * LINK_BPS * 55 / 64) if d == 55 else None)
         for d in STAR_DEGREES}
# l256d_f130's graph with 257 flows: shape (8, 4) with the action table in LDS (40 nodes: 1 600 B),
# where l256_f512's 4 096 B stay in HBM -- the one way to a fused-only table instance of that shape.
# Beside IDENTITY, so of the GPU matrices only tests/test_gpu_set_instances.py runs it, on that instance
LDS_TABLE_8_4 = "l256d_f257"
EXTRA = {LDS_TABLE_8_4: _c("synth", (40, 108, 257), (8, 4), (1, 1), rate=int(0.5 * default_rate(108, 257)))}
CASES = {**IDENTITY, **TUNNELLED, **STARS, **EXTRA}

# inner underlay nodes as overlay nodes: a ping-back crosses an overlay node of lower degree within
# the first ping rounds, so every replica ends on PRISMA_EBIT_PINGIDX (tests/test_error_flags.py);
# name: (builder arguments, builder seed, per-flow rate)
ERROR_CASES = {
    "inner_k9_s5": ((30, 40, 9, 60), 5, 30000),
    "inner_k9_s6": ((30, 40, 9, 60), 6, 30000),
    "inner_k8_s5": ((20, 26, 8, 40), 5, 30000),
}

# 513 flows: beyond the register engine (AUTO plans the memory engine, _REGISTER refuses)
MEMORY_ONLY = (24, 23, 513)

SEED = 5
H = 3000                               # hops per case, over 2 launches on the GPU
R = 3
REPLICA_BASE = 7
SIM_TIME_S = 6.0
LOG = 8192

# the instance sets: (MLP policy, train = the ctrl instances, run(..., explore=))
VARIANTS = {"lite_table": (0, 0, 0), "ctrl_table": (0, 1, 0), "lite_mlp": (1, 0, 0), "ctrl_mlp": (1, 1, 0),
            "explore_table": (0, 0, 1), "explore_mlp": (1, 0, 1)}
PK_SHAPES = [(fs, ls) for fs in (1, 2, 4, 8) for ls in (1, 2, 4)]

# the sets added after VARIANTS (tests/test_set_instance_matrix.py on the CPU, tests/test_gpu_set_instances.py
# on the GPU): the step-kernel set the run launches, its policy ("table": the SP table; a DQN-buffer
# family kind: StackedQNet(topo, kind, seed=MLP_SEED); "stoch": optrouting.path_split_routing(topo, 3,
# SEED)), whether node_eps explores, whether a history of ones weights the exploring picks, and the hops
# per case, over 2 launches on the GPU.  The exploring variants take 4 000: a quarter of the nodes
# explore at every decision, packets wander, and on the 64-node cases 3 000 hops end at 0.53 - 0.6 s,
# before the third ping round (0.6 s); 4 000 reach it on every case and replica
EXPLORE_H = 4000


def _v(set_, policy, hops, explore=0, smart=0):
    return dict(set=set_, policy=policy, hops=hops, explore=explore, smart=smart)


SET_VARIANTS = {
    "lightq": _v("lightq", "buffer_lite", H),
    "explore_lightq": _v("explore_lightq", "buffer_lighter_3", EXPLORE_H, explore=1),
    "smart_table": _v("smart", "table", EXPLORE_H, explore=1, smart=1),
    "smart_mlp": _v("smart_mlp", "buffer", EXPLORE_H, explore=1, smart=1),
    "smart_lightq": _v("smart_lightq", "buffer_lighter_3", EXPLORE_H, explore=1, smart=1),
    "stoch": _v("stoch", "stoch", H),
}


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    fn = {"synth": synth, "star": star, "tunnelled": tunnelled}[c["kind"]]
    return fn(*c["args"], SEED, c["rate"])


@functools.lru_cache(maxsize=None)
def build_error(name):
    args, seed, rate = ERROR_CASES[name]
    return tunnelled(*args, seed, rate, inner=True)


def error_params(name, **kw):
    """engine_params of an ERROR_CASES topology: the matrix's replicas, episode and log."""
    from prisma_amd.config import engine_params
    args = dict(sim_time_s=SIM_TIME_S, replica_base=REPLICA_BASE, log_capacity=LOG, seed=100 + ERROR_CASES[name][1])
    args.update(kw)
    return engine_params(build_error(name), **args)


def case_params(name, **kw):
    """engine_params of a matrix case: R = 3 replicas from replica_base 7, a 6-s episode, a log of
    8 192 records, the case's own overrides (a seed), then the caller's."""
    from prisma_amd.config import engine_params
    args = dict(sim_time_s=SIM_TIME_S, replica_base=REPLICA_BASE, log_capacity=LOG, seed=100 + SEED)
    args.update(CASES[name]["params"])
    args.update(kw)
    return engine_params(build(name), **args)


def node_eps(topo):
    """Per-node epsilons of the exploring variants: 0, 1, 0.3 and 0.05 by overlay index, 0 off the
    overlay (tests/test_gpu_instances.py's _eps)."""
    eps = np.zeros(topo.n_nodes)
    eps[topo.overlay_nodes] = [(0.0, 1.0, 0.3, 0.05)[i % 4] for i in range(topo.n_overlay)]
    return eps


@functools.lru_cache(maxsize=None)
def case_table(name):
    from prisma_amd.topology import sp_next_hop_table
    return sp_next_hop_table(build(name))


@functools.lru_cache(maxsize=None)
def case_net(name, kind):
    """(torch model on the CPU, its packed weights as numpy) of a case and a DQN-buffer family kind."""
    from prisma_amd.policies import StackedQNet
    net = StackedQNet(build(name), kind, seed=MLP_SEED, device="cpu")
    return net, net.pack().numpy()


@functools.lru_cache(maxsize=None)
def case_routing(name):
    """The stoch variant's routing matrix, float64 [NO, NO, T] in the reference's edge order."""
    from prisma_amd import optrouting
    return optrouting.path_split_routing(build(name), 3, seed=SEED)


def set_variant_inputs(name, variant):
    """What a SET_VARIANTS run of a case takes, the same objects on the CPU and on the GPU:
    dict(policy=the SP table | packed fp32 weights | the routing matrix, kind=the model kind or None,
    net=the torch model or None, eps=per-node epsilons or None, thr=their thresholds or None)."""
    from prisma_amd import explore
    v = SET_VARIANTS[variant]
    topo = build(name)
    out = dict(kind=None, net=None, eps=None, thr=None)
    if v["policy"] == "table":
        out["policy"] = case_table(name)
    elif v["policy"] == "stoch":
        out["policy"] = case_routing(name)
    else:
        out["kind"] = v["policy"]
        out["net"], out["policy"] = case_net(name, v["policy"])
    if v["explore"]:
        out["eps"] = node_eps(topo)
        out["thr"] = explore.thresholds(out["eps"])
    return out


def last_switch_slot(topo):
    """The last register slot (the memory-resident engine: 64-leaf link block) that holds a
    switch link of an identity overlay."""
    return (topo.n_links - 1) >> 6


def access_only_nodes(topo):
    """Nodes whose access link (index n_links + v) lies in a slot past the last switch link's."""
    v = np.arange(topo.n_nodes)
    return v[(topo.n_links + v) >> 6 > last_switch_slot(topo)]


# (case, ma_size, cached send delays per flow): the draw cache's layout on one FS <= 2 shape (two
# per flow, one, none as the moving-average windows grow the LDS image) and one FS >= 4 (never)
DCACHE_CASES = [("l40_f100", 5, 2), ("l40_f100", 16, 1), ("l40_f100", 32, 0), ("l64_f129", 5, 0), ("l64_f129", 32, 0)]
RNG_BYTES = 112                        # the ns-3 streams' state at the end of the LDS image


def dcache_bytes(name, **kw):
    """Bytes of the flows' draw cache in a case's LDS image, from prisma_plan alone: the image
    with Philox streams (the cache, where laid out) against the one with ns-3 streams (never a
    cache; RNG_BYTES of stream state instead)."""
    from prisma_amd import engine
    a = engine.plan(build(name), case_params(name, **kw))
    b = engine.plan(build(name), case_params(name, rng="ns3", **kw))
    return a["lds_state_bytes"] - (b["lds_state_bytes"] - RNG_BYTES)


# ---- the memory-resident engine's matrix --------------------------------------------------
# Its event tree is 64-ary: 64 link leaves (Lk = n_links + n_nodes of them) per link block, 64 flow
# leaves (FG = the flows, plus one leaf the big-signalling generators share) per flow block, 64 flow
# blocks per flow group; the n_lb link blocks and the flow groups are the n_top <= 64 lanes of the
# top level (prisma_engine.hip layout_mem).  tests/test_mem_instance_matrix.py (CPU: the plan and
# the oracle's own run) and tests/test_gpu_mem_instances.py (GPU parity) import what follows.
def circulant(n, k, chords, f, seed, rate):
    """Identity overlay on a ring of n nodes, each joined to its k nearest nodes on either side,
    plus `chords` chords of offset k + 1 from nodes 0 .. chords - 1: 2 (n k + chords) switch links."""
    rng = np.random.default_rng([seed, n, k, chords, f])
    adj = np.zeros((n, n), dtype=np.int64)
    v = np.arange(n)
    for d in range(1, k + 1):
        adj[v, (v + d) % n] = adj[(v + d) % n, v] = 1
    c = np.arange(chords)
    adj[c, (c + k + 1) % n] = adj[(c + k + 1) % n, c] = 1
    tm = np.zeros((n, n), dtype=object)
    for a, b in _pick_flows(range(n), f, rng):
        tm[a, b] = int(rate)
    return Topology.from_matrices(adj, tm, name=f"circ{n}_{k}_{chords}_{f}")


def slow_tail(n, m, f, seed, rate, tail_rate):
    """synth's graph and flows, but the last flow (alone in its flow block when f = 64 j + 1) sends
    at `tail_rate`."""
    rng = np.random.default_rng([seed, n, m, f])
    adj = _tree_plus_edges(n, m, rng)
    tm = np.zeros((n, n), dtype=object)
    flows = _pick_flows(range(n), f, rng)
    for a, b in flows:
        tm[a, b] = int(rate)
    tm[flows[-1]] = int(tail_rate)
    return Topology.from_matrices(adj, tm, name=f"slow{n}_{m}_{f}")


def line(n, flows, seed, rate):
    """A path of n nodes with the given (src, dst) flows; the seed is not used."""
    adj = np.zeros((n, n), dtype=np.int64)
    v = np.arange(n - 1)
    adj[v, v + 1] = adj[v + 1, v] = 1
    tm = np.zeros((n, n), dtype=object)
    for a, b in flows:
        tm[a, b] = int(rate)
    return Topology.from_matrices(adj, tm, name=f"line{n}")


def bfs_next_hop_table(topo):
    """[N, N] uint8 action table of an identity overlay from the topology's own BFS routing
    (route_tables: the lowest-numbered neighbour one hop nearer).  sp_next_hop_table's bidirectional
    search per pair is slow at 256 nodes; parity only needs the same table on both sides."""
    assert topo.identity and topo.max_deg <= 255
    rank = np.cumsum(topo.adjacency, axis=1) - 1                     # neighbour v is action rank[u, v] of u
    table = np.take_along_axis(rank, np.maximum(topo.next_hop, 0).astype(np.int64), axis=1)
    np.fill_diagonal(table, 0)
    return np.ascontiguousarray(table, dtype=np.uint8)


def tree_shape(topo, big_signaling=0):
    """(Lk, FG, n_lb, n_fb, n_top) of an identity overlay by layout_mem's formulas; with big
    signalling the generators (one per flow between neighbours) share one more flow leaf."""
    lk = topo.n_links + topo.n_nodes
    n_gen = int(topo.adjacency[topo.flow_src, topo.flow_dst].sum()) if big_signaling else 0
    fg = topo.n_flows + int(n_gen > 0)
    n_lb, n_fb = (lk + 63) // 64, (fg + 63) // 64
    return lk, fg, n_lb, n_fb, n_lb + (n_fb + 63) // 64


def mem_lds_state_bytes(shape, obs_width, ns3=False):
    """The LDS part of the memory-resident engine's state image: header, counters, pending
    observation, flow block minima, top-level image, link leaf keys and kinds (16-B aligned each)."""
    lk, _, _, n_fb, n_top = shape
    a16 = lambda b: (b + 15) & ~15
    return 128 + 160 + a16(4 * obs_width) + 16 * n_fb + 16 * n_top + a16(8 * lk) + a16(lk) + (RNG_BYTES if ns3 else 0)


# name: builder and its arguments, builder seed, per-flow rate(s), hops per replica (None: to the
# episode's end), log capacity, the expected tree shape (Lk, FG, n_lb, n_fb, n_top), engine params
# beyond the common ones.  The rates of the large cases are set so that the hops span 3 ping rounds.
def _m(kind, args, shape, hops=H, bseed=SEED, rate=None, log=LOG, **params):
    return dict(kind=kind, args=args, seed=bseed, rate=rate, hops=hops, log=log, shape=shape, params=params)


_BSIG = dict(train=1, signaling_type="NN", big_signaling=1, sync_step_s=0.25)
_MEM_IDENTITY_SHAPES = {
    "l64_f64": (64, 64, 1, 1, 2), "l65_f65": (65, 65, 2, 2, 3), "l64_f129": (64, 129, 1, 3, 2),
    "l64_f257": (64, 257, 1, 5, 2), "l128_f64": (128, 64, 2, 1, 3), "l129_f128": (129, 128, 3, 2, 4),
    "l128_f256": (128, 256, 2, 4, 3), "l128_f512": (128, 512, 2, 8, 3), "l129_f64": (129, 64, 3, 1, 4),
    "l256_f65": (256, 65, 4, 2, 5), "l256_f129": (256, 129, 4, 3, 5), "l256_f512": (256, 512, 4, 8, 5),
    "l256d_f130": (256, 130, 4, 3, 5), "l40_f100": (40, 100, 1, 2, 2), "l100_f128": (100, 128, 2, 2, 3),
}
# every IDENTITY case forced onto the memory-resident engine: Lk and FG at 64, 65, 128, 129, 256, 512
MEM_IDENTITY = {n: _m(c["kind"], c["args"], _MEM_IDENTITY_SHAPES[n], rate=c["rate"], **c["params"])
                for n, c in IDENTITY.items()}
MEM_NEW = {
    # 9 flow blocks, flow 512 alone in the last
    "m_f513": _m("synth", MEMORY_ONLY, (70, 513, 2, 9, 3), hops=6000),
    # one flow group exactly full (64 blocks) | flow 4096 alone in block 64, alone in group 1; about
    # one packet per flow in 16 000 hops: engine seed 110 is one under which flow 4096 sends on every
    # replica (found by a CPU search of seeds 105-112)
    "m_f4096": _m("synth", (66, 100, 4096), (266, 4096, 5, 64, 6), hops=16000, rate=4000, log=32768),
    "m_f4097": _m("synth", (66, 100, 4097), (266, 4097, 5, 65, 7), hops=16000, rate=4000, log=32768, seed=110),
    # 256 nodes, 3 776 switch links: 63 link blocks (59 with switch links, 4 with the access links)
    # and one flow group in lane 63 of the top level, whose last flow block holds 24 flows
    "m_top64": _m("circulant", (256, 7, 96, 600), (4032, 600, 63, 10, 64), hops=12000, rate=15000, log=16384),
    # 60 link blocks and 4 flow groups, the last with one block: lanes 60-63
    "m_top64_groups": _m("circulant", (256, 7, 0, 12352), (3840, 12352, 60, 193, 64), hops=16000, rate=900,
                         log=32768),
    # big signalling: the generators' leaf (FG = flows + 1) alone in block 1 | alone in group 1
    "m_bsig65": _m("synth", (22, 21, 64), (64, 65, 1, 2, 2), **_BSIG),
    "m_bsig4097": _m("synth", (66, 100, 4096), (266, 4097, 5, 65, 7), hops=16000, rate=4000, log=32768, **_BSIG),
    # flows 0-63 send every 0.5 s on average, flow 64 (block 1's only leaf) every 7 s: when its send
    # re-reduces block 1, the block's only key is more than 2^32 ns ahead of the clock (the saturated
    # reduction of fblock_min_cached, beside a busy block 0).  To the end of a 40-s episode; engine seed 113: flow 64
    # has two sends that far apart on every replica, in the table's run and within the first 16 000
    # hops of the DQN-buffer MLP's (seed 21), whose routes are longer (CPU search of seeds 105-120)
    "m_slow65": _m("slow_tail", (12, 20, 65), (52, 65, 1, 2, 2), hops=None, rate=(8192, 585), log=32768,
                   sim_time_s=40.0, seed=113),
    # m_f4097 with a flow 4096 that sends every 7 s on average: its start event (within the first
    # second) schedules its first send more than 2^32 ns ahead, the only key of block 64 and of group
    # 1 (fgroup_min's saturated reduction over a partial group, next to 4 096 busy flows).  Engine
    # seed 115: so on every replica (CPU search of seeds 105-124); flow 4096 never sends in the run
    "m_g1slow": _m("slow_tail", (66, 100, 4097), (266, 4097, 5, 65, 7), hops=16000, rate=(4000, 585), log=32768,
                   seed=115),
    # m_bsig65 with a 5-s period: the generators' leaf, block 1's only one, is re-armed more than
    # 2^32 ns ahead at their start, and fires once before the 6-s episode ends
    "m_bsig65_slow": _m("synth", (22, 21, 64), (64, 65, 1, 2, 2), hops=None, rate=20000, log=16384,
                        **dict(_BSIG, sync_step_s=5.0)),
    # three flows that send every 13.7 s on average and a ping every 7 s: between ping rounds every
    # key of the top level and the ping timer are more than 2^32 ns ahead (select_event's saturated
    # reduction, on either engine).  To the end of a 60-s episode; engine seed 108: every replica has
    # a ping round with no record from 0.5 s before it to the next (CPU search of seeds 105-116)
    "m_idle": _m("line", (4, ((0, 3), (3, 0), (1, 2))), (10, 3, 1, 1, 2), hops=None, rate=300,
                 sim_time_s=60.0, ping_interval_s=7.0, seed=108),
}
RUN_TO_END = 10 ** 6                   # hops of the cases that run to the episode's end (hops=None)
MLP_SEED = 21                          # StackedQNet(topo, "buffer", seed=) of the MLP runs
SLOW_MLP_HOPS = 16000                  # m_slow65 under the MLP: about 16 s of the episode
MEMORY_CASES = {**MEM_IDENTITY, **MEM_NEW}


@functools.lru_cache(maxsize=None)
def build_mem(name):
    c = MEMORY_CASES[name]
    fn = {"synth": synth, "circulant": circulant, "slow_tail": slow_tail, "line": line}[c["kind"]]
    rate = c["rate"] if isinstance(c["rate"], tuple) else (c["rate"],)
    return fn(*c["args"], c["seed"], *rate)


@functools.lru_cache(maxsize=None)
def mem_table(name):
    return bfs_next_hop_table(build_mem(name))


def mem_params(name, **kw):
    """engine_params of a memory case: case_params' conventions (R = 3 replicas from replica_base 7,
    a 6-s episode), the case's log, the memory-resident engine, the case's overrides, the caller's."""
    from prisma_amd.config import engine_params
    from prisma_amd.engine import PRISMA_ENGINE_MEMORY
    c = MEMORY_CASES[name]
    args = dict(sim_time_s=SIM_TIME_S, replica_base=REPLICA_BASE, log_capacity=c["log"], seed=100 + SEED,
                engine=PRISMA_ENGINE_MEMORY)
    args.update(c["params"])
    args.update(kw)
    return engine_params(build_mem(name), **args)
