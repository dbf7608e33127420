"""Synthetic topologies that reach every (flow_slots, link_slots) instance of the register-resident
step kernel at its slot boundaries, and the case matrix tests/test_instance_matrix.py (CPU: the
plan and the oracle's own run) and tests/test_gpu_instances.py (GPU parity) both import.

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
CASES = {**IDENTITY, **TUNNELLED, **STARS}

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


def last_switch_slot(topo):
    """The last register slot that holds a switch link of an identity overlay."""
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
