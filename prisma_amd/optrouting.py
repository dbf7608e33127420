"""Stochastic multipath routing -- the reference's "opt" agent (forwarder.py:87-88, 192-194;
utils.py:161-199 optimal_routing_decision) -- restated on the host for callers and tests: the rule
of include/prisma.h prisma_run_stochastic, the packing of a routing matrix into its device table,
a reader for the reference's solution files and two generators of routing matrices.

A routing matrix is float64 ``routing[s][t][k]``: the fraction of the flow from overlay node ``s``
to overlay node ``t`` that crosses overlay edge ``k``, edges in the order of ``list(G.edges)`` of
the reference's DiGraph (overlay node ascending, neighbour ascending; ``reference_edges``).

The tag.  The reference carries a per-packet ``tag``, which is always
``routing[src][dst][edge taken at the previous decision]`` (both branches of
optimal_routing_decision return the fraction of the edge they chose; a new packet starts with
None).  It therefore follows from the previous decision's (node, action) and the packet's source.

The float test made integer.  ``tag in prob_to_neighbors and tag < 1`` compares float64 values.
``pack_routing`` gives every entry of ``routing[s][t][:]`` a class: the distinct values x with
0 < x < 1 in ascending order get classes 1, 2, ...; 0 and values >= 1 get class 0.  Two entries are
equal as float64 and below 1 exactly when their classes are equal and non-zero.

The table.  uint32 ``tab[NO][NO][T]``, the last axis laid out as an action history is
(prisma_action_history_layout: node v's actions are columns row[v] .. row[v + 1], by underlay id):
bits 24-31 the class, bits 0-23 the weight ``min(floor(p / rowsum * 2^24 + 0.5), 2^24 - 1)`` with
``rowsum`` the float64 sum, left to right, of node v's entries for (s, t); 0 where rowsum == 0.

The decision, for data decision ``d`` (the numbering of the records' ``prev``) of episode ``e`` at
node ``v`` of degree ``deg``, in the replica with global id ``gid``, for a packet with source ``s``,
destination ``t`` and previous decision ``(u, a_u)`` or none:

    c_prev = (prev exists and 0 <= a_u < deg(u)) ? cls(tab[s][t][row[u] + a_u]) : 0
    M      = { i < deg : cls(tab[s][t][row[v] + i]) == c_prev }
    if c_prev != 0 and M not empty:   a = min M                      (no draw)
    else:  c = philox4x32_10(ctr = {d, 0, e, 3}, key = {seed & 0xffffffff, gid})
           W = sum_i wt_i
           a = W == 0 ? (uint32)(((uint64)c[1] * deg) >> 32)
                      : min { i : wt_0 + ... + wt_i > u },  u = (uint32)(((uint64)c[1] * W) >> 32)

Defined, not copied: Philox draws replace numpy's global stream; probabilities are quantised to 24
bits (an edge below 2^-25 of its row is never drawn); an all-zero row, a NaN and a crash in the
reference, takes the uniform pick; ``rejected_flows`` is read and ignored (the reference's use of
it is commented out).  numpy only.
"""
from __future__ import annotations

import json

import numpy as np

from .explore import philox4x32_10
from .topology import Topology, route_tables

STOCH_DOMAIN = 3
WT_ONE = 1 << 24
MAX_CLASSES = 255
_MASK = 0xFFFFFFFF


def edge_rows(topo: Topology) -> np.ndarray:
    """row [n_nodes + 1] of the table's last axis: node v's actions are columns row[v] ..
    row[v + 1], by underlay id (prisma_action_history_layout); row[-1] = T."""
    return np.asarray(topo.ov_row_ptr, dtype=np.int64)


def reference_edges(topo: Topology):
    """(edges, col): the overlay edges (i, j) by overlay index in the order of the reference's
    ``list(G.edges)`` -- the order of a routing matrix's last axis -- and the table column of each."""
    row = edge_rows(topo)
    edges, col = [], []
    for i in range(topo.n_overlay):
        u = int(topo.overlay_nodes[i])
        for a, w in enumerate(topo.neighbors(u)):
            edges.append((i, int(topo.overlay_index[w])))
            col.append(int(row[u]) + a)
    return edges, np.asarray(col, dtype=np.int64)


def pack_routing(topo: Topology, routing) -> np.ndarray:
    """routing float64 [NO, NO, T] (reference edge order) -> the device table uint32 [NO, NO, T]
    (class << 24 | weight, columns in the action-history layout).  ValueError on a wrong shape, on
    negative or non-finite entries and on more than 255 classes for one (s, t)."""
    no, row = topo.n_overlay, edge_rows(topo)
    T = int(row[-1])
    p = np.asarray(routing, dtype=np.float64)
    if p.shape != (no, no, T):
        raise ValueError(f"routing must have shape ({no}, {no}, {T}) = (overlay nodes, overlay nodes, overlay "
                         f"edges), got {p.shape}")
    if not np.all(np.isfinite(p)):
        raise ValueError("routing holds NaN or infinite entries")
    if np.any(p < 0):
        raise ValueError("routing holds negative entries")
    _, col = reference_edges(topo)
    q = np.zeros_like(p)
    q[:, :, col] = p                                            # columns in the table's order
    cls = np.zeros((no, no, T), dtype=np.uint32)
    for s in range(no):
        for t in range(no):
            x = q[s, t]
            inner = (x > 0) & (x < 1)
            vals = np.unique(x[inner])                          # ascending, distinct as float64
            if vals.size > MAX_CLASSES:
                raise ValueError(f"routing[{s}][{t}] has {vals.size} distinct values in (0, 1): at most "
                                 f"{MAX_CLASSES} classes fit the table")
            cls[s, t, inner] = 1 + np.searchsorted(vals, x[inner]).astype(np.uint32)
    wt = np.zeros((no, no, T), dtype=np.uint32)
    for v in range(topo.n_nodes):
        r0, r1 = int(row[v]), int(row[v + 1])
        if r1 == r0:
            continue
        seg = q[:, :, r0:r1]
        rowsum = np.cumsum(seg, axis=-1)[..., -1:]              # left to right, as Python's sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.floor(seg / rowsum * float(WT_ONE) + 0.5)
        w = np.where(rowsum == 0, 0.0, np.minimum(w, float(WT_ONE - 1)))
        wt[:, :, r0:r1] = w.astype(np.uint32)
    return (cls << np.uint32(24)) | wt


def stoch_draw(seed, gid, d, episode) -> np.ndarray:
    """The decision's Philox words c [..., 4] (counter word 3 = 3)."""
    d, episode, gid = np.broadcast_arrays(np.asarray(d, dtype=np.uint64), np.asarray(episode, dtype=np.uint64),
                                          np.asarray(gid, dtype=np.uint64))
    ctr = np.stack([d, np.zeros_like(d), episode, np.full_like(d, STOCH_DOMAIN)], axis=-1)
    key = np.stack([np.full_like(d, int(seed) & _MASK), gid], axis=-1)
    return philox4x32_10(ctr, key)


def stoch_pick(c1, wt):
    """The drawn action: c1 the draw's word 1 (scalar or array), wt the node's weights [deg].
    A scalar c1 gives an int, an array an int64 array."""
    c1 = np.asarray(c1, dtype=np.uint64)
    wt = np.asarray(wt, dtype=np.uint64)
    deg = wt.shape[-1]
    W = wt.sum(dtype=np.uint64)                                 # < 2^30: deg <= 55
    if W == 0:
        a = (c1 * np.uint64(deg)) >> np.uint64(32)
    else:
        u = (c1 * W) >> np.uint64(32)                           # c1 * W < 2^62
        a = (np.cumsum(wt, dtype=np.uint64) <= u[..., None]).sum(axis=-1)   # the first i with prefix_i > u
    a = a.astype(np.int64)
    return int(a) if a.ndim == 0 else a


def stoch_action(tab, row, s, t, v, prev, seed, gid, d, episode, with_branch=False):
    """The action the stochastic-routing kernels take.  tab: the packed table [NO, NO, T]; row:
    edge_rows; s, t: overlay indices of the packet's source and destination; v: the deciding node
    (underlay id); prev: None for a fresh packet, else (u, a_u), node and action of its previous
    decision.  with_branch: return (action, followed) instead of the action."""
    st = np.asarray(tab)[int(s), int(t)]
    r0, deg = int(row[v]), int(row[v + 1] - row[v])
    e = st[r0:r0 + deg].astype(np.uint32)
    c_prev = 0
    if prev is not None:
        u, a_u = int(prev[0]), int(prev[1])
        if 0 <= a_u < int(row[u + 1] - row[u]):
            c_prev = int(st[int(row[u]) + a_u]) >> 24
    if c_prev != 0:
        m = np.flatnonzero((e >> np.uint32(24)) == c_prev)
        if m.size:
            return (int(m[0]), True) if with_branch else int(m[0])
    c = stoch_draw(seed, gid, d, episode)
    a = stoch_pick(int(c[1]), e & np.uint32(WT_ONE - 1))
    return (a, False) if with_branch else a


def load_optimal_solution(path: str):
    """The reference's optimal-solution file (argument_parser.py:148, agent.py:136-137): JSON with
    "routing" [N][N][E] and "rejected_flows".  Returns (routing float64, rejected_flows float64);
    the latter is not used by the rule."""
    with open(path, "r") as fh:
        sol = json.load(fh)
    return np.asarray(sol["routing"], dtype=np.float64), np.asarray(sol["rejected_flows"], dtype=np.float64)


def _overlay_graph(topo: Topology):
    adj = (np.asarray(topo.overlay_adj) != 0).astype(np.int32)
    _, dist = route_tables(adj)
    nb = [[int(j) for j in np.flatnonzero(adj[i])] for i in range(adj.shape[0])]
    return adj, dist, nb


def ecmp_routing(topo: Topology) -> np.ndarray:
    """An equal split over the shortest-path next hops: routing[s][t][(v, w)] = 1 / k for each of
    the k overlay neighbours w of v one hop closer to t (for every s), 0 elsewhere."""
    _, dist, nb = _overlay_graph(topo)
    edges, _ = reference_edges(topo)
    no = topo.n_overlay
    out = np.zeros((no, no, len(edges)), dtype=np.float64)
    for t in range(no):
        for v in range(no):
            if v == t:
                continue
            k = sum(1 for w in nb[v] if dist[w, t] == dist[v, t] - 1)
            for e, (a, b) in enumerate(edges):
                if a == v and dist[b, t] == dist[v, t] - 1:
                    out[:, t, e] = 1.0 / k
    return out


def _bfs_path(nb, s, t, banned):
    """The shortest path s -> t avoiding the directed edges in `banned` (lowest ids first), or None."""
    parent = {s: None}
    frontier = [s]
    while frontier and t not in parent:
        nxt = []
        for x in frontier:
            for y in nb[x]:
                if y not in parent and (x, y) not in banned:
                    parent[y] = x
                    nxt.append(y)
        frontier = nxt
    if t not in parent:
        return None
    path = [t]
    while parent[path[-1]] is not None:
        path.append(parent[path[-1]])
    return path[::-1]


def _acyclic(edge_set) -> bool:
    out = {}
    for a, b in edge_set:
        out.setdefault(a, []).append(b)
    state = {}

    def visit(x):
        state[x] = 1
        for y in out.get(x, ()):
            if state.get(y) == 1 or (y not in state and not visit(y)):
                return False
        state[x] = 2
        return True

    return all(visit(x) for x in list(out) if x not in state)


def path_split_routing(topo: Topology, k: int = 3, seed: int = 0) -> np.ndarray:
    """Up to k simple paths per (s, t) with distinct fractions: the shortest path and the shortest
    paths that avoid one of its edges, kept while their union stays acyclic; path j carries the
    fraction w_j / sum(w), w_j = j + 1 + a uniform draw of numpy's default_rng(seed).  An edge's
    entry is the sum of the fractions of the paths that cross it."""
    if k < 1:
        raise ValueError("k must be >= 1")
    _, _, nb = _overlay_graph(topo)
    edges, _ = reference_edges(topo)
    index = {e: i for i, e in enumerate(edges)}
    no = topo.n_overlay
    rng = np.random.default_rng(seed)
    out = np.zeros((no, no, len(edges)), dtype=np.float64)
    for s in range(no):
        for t in range(no):
            if s == t:
                continue
            first = _bfs_path(nb, s, t, set())
            paths, used = [first], set(zip(first[:-1], first[1:]))
            for cut in zip(first[:-1], first[1:]):
                if len(paths) >= k:
                    break
                p = _bfs_path(nb, s, t, {cut})
                if p is None or p in paths:
                    continue
                pe = set(zip(p[:-1], p[1:]))
                if _acyclic(used | pe):
                    paths.append(p)
                    used |= pe
            w = np.arange(1, len(paths) + 1, dtype=np.float64) + rng.random(len(paths))
            f = w / w.sum()
            for p, fj in zip(paths, f):
                for e in zip(p[:-1], p[1:]):
                    out[s, t, index[e]] += fj
    return out
