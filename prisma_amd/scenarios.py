"""Traffic scenarios: the replicas of one env on different traffic matrices and load factors.

An env's replicas run one topology, one parameter set and one set of launches; with a
``ScenarioSet`` each replica reads the flow rates of its own scenario (include/prisma.h
prisma_create_scenarios).  Flow rates are all a scenario may change: the flow LIST decides the state
layout, the kernel instances and the start-event numbering, so every topology of a set must have the
same nodes, links, overlay and (flow_src, flow_dst) -- which holds for all shipped data sets over
their traffic matrices and load factors (tests/test_scenarios.py).

Replica r of a scenario env equals replica r (same global id) of a single-scenario env on
``scenarios.topos[scenario_of[r]]``: the oracle checks it as ``OracleSim(that topology, params, id)``.

Not per scenario: the exploration thresholds and the stochastic routing table of a launch stay one
per env, and QRoutingTrainer.compute_sync_step reads scenario 0's traffic matrix (env.topo).

No torch import here.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .topology import Topology

# what scenarios of one set may differ in; every other array field of Topology must be equal
MAY_DIFFER = ("flow_rate_bps", "flow_base_bps", "load_factor", "name", "tm_strings")
STRUCTURAL = ("n_nodes", "adjacency", "row_ptr", "link_dst", "link_src", "link_rev", "flow_src", "flow_dst",
              "overlay_index", "overlay_nodes", "overlay_adj", "ov_row_ptr", "tun_src", "tun_dst", "tun_link",
              "tun_len", "next_hop", "dist")

# prisma_scenario_stats_t (include/prisma.h): 31 eight-byte fields
STATS_INT_FIELDS = ("events", "hops", "decisions", "hop_deg_sum", "now_ns", "ov_injected", "ov_arrived", "ov_lost",
                    "un_injected", "un_arrived", "un_lost", "bytes_data", "bytes_signaling", "cost_n", "e2e_n",
                    "un_cost_n", "episode", "ping_rounds", "seq", "uid", "dec_count", "ctrl_dropped", "hops_total",
                    "events_total")
STATS_SIGNED = ("now_ns", "ov_injected", "ov_arrived", "ov_lost", "un_injected", "un_arrived", "un_lost",
                "bytes_data", "bytes_signaling", "cost_n", "e2e_n", "un_cost_n")
STATS_F64_FIELDS = ("reward_sum", "cost_sum", "e2e_sum", "un_cost_sum")
STATS_DTYPE = np.dtype([("n_replicas", "<u8"), ("n_error", "<u8"), ("n_over", "<u8")]
                       + [(k, "<i8" if k in STATS_SIGNED else "<u8") for k in STATS_INT_FIELDS]
                       + [(k, "<f8") for k in STATS_F64_FIELDS])
assert STATS_DTYPE.itemsize == 248

MAX_SCENARIOS = 65535            # PRISMA_MAX_SCENARIOS


def stats_sum(x) -> float:
    """The f64 sum of prisma_scenario_stats, restated (include/prisma.h): lane l of 64 adds
    x[l], x[l + 64], ... in turn from +0.0, then the lane sums fold in halves, a[l] += a[l + h] for
    h = 32 .. 1; every addition one IEEE binary64 add.  Bit-equal to the kernel's result."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    pad = np.zeros(-(-max(n, 1) // 64) * 64, dtype=np.float64)
    pad[:n] = x
    rows = pad.reshape(-1, 64)
    a = np.zeros(64, dtype=np.float64)
    for k in range(rows.shape[0]):
        # a lane past the end adds nothing (not even +0.0: -0.0 + 0.0 would lose a sign the kernel keeps)
        live = 64 if (k + 1) * 64 <= n else n - k * 64
        a[:live] = a[:live] + rows[k, :live]
    h = 32
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return float(a[0])


def stats_host(counters: np.ndarray, scenario_of, n_scenarios: int) -> np.ndarray:
    """prisma_scenario_stats on the host, from counters() (COUNTERS_DTYPE [R]) and scenario_of [R]:
    STATS_DTYPE [n_scenarios], the f64 fields in stats_sum's order over ascending replica index."""
    sc = np.asarray(scenario_of)
    out = np.zeros(int(n_scenarios), dtype=STATS_DTYPE)
    for s in range(int(n_scenarios)):
        c = counters[sc == s]
        out[s]["n_replicas"] = len(c)
        out[s]["n_error"] = int((c["error"] != 0).sum())
        out[s]["n_over"] = int((c["episode_over"] != 0).sum())
        for k in STATS_INT_FIELDS:
            out[s][k] = int(c[k].astype(np.int64 if k in STATS_SIGNED else np.uint64).sum())
        for k in STATS_F64_FIELDS:
            out[s][k] = stats_sum(c[k].astype(np.float64))
    return out


def _first_difference(a: Topology, b: Topology):
    for k in STRUCTURAL:
        x, y = getattr(a, k), getattr(b, k)
        if k == "n_nodes":
            same = int(x) == int(y)
        elif x is None or y is None:
            same = x is None and y is None
        else:
            x, y = np.asarray(x), np.asarray(y)
            same = x.shape == y.shape and bool(np.array_equal(x, y))
        if not same:
            return k
    return None


class ScenarioSet:
    """S topologies that differ in their traffic only (MAY_DIFFER); .rates is uint64 [S, F]."""

    def __init__(self, topos: Sequence[Topology]):
        topos = list(topos)
        if not topos:
            raise ValueError("a ScenarioSet needs at least one topology")
        if len(topos) > MAX_SCENARIOS:
            raise ValueError(f"more than {MAX_SCENARIOS} scenarios")
        for s, t in enumerate(topos[1:], 1):
            k = _first_difference(topos[0], t)
            if k is not None:
                raise ValueError(f"scenario {s} ({t.name}, load factor {t.load_factor}) differs from scenario 0 in "
                                 f"{k}: the scenarios of one env share nodes, links, overlay and flow list "
                                 f"(only {', '.join(MAY_DIFFER)} may differ)")
        self.topos: List[Topology] = topos
        self.rates = np.ascontiguousarray(np.stack([np.asarray(t.flow_rate_bps, dtype=np.uint64) for t in topos]))
        if np.any(self.rates == 0):
            s, f = [int(v[0]) for v in np.nonzero(self.rates == 0)]
            raise ValueError(f"flow_rate_bps: zero rate of flow {f} in scenario {s}")

    def __len__(self) -> int:
        return len(self.topos)

    @property
    def n_scenarios(self) -> int:
        return len(self.topos)

    @property
    def labels(self) -> list:
        return [f"{t.name} lf {t.load_factor:g}" for t in self.topos]

    @classmethod
    def grid(cls, name: str, tm_indices: Sequence[int], load_factors: Sequence[float]) -> "ScenarioSet":
        """The traffic-matrix x load-factor grid of a shipped data set, TM-major:
        scenario i * len(load_factors) + j is (tm_indices[i], load_factors[j])."""
        return cls([Topology.example(name, int(tm), float(lf)) for tm in tm_indices for lf in load_factors])

    def assign(self, n_replicas: int, how: str = "round_robin", replica_base: int = 0,
               n_total: int = None) -> np.ndarray:
        """int32 [n_replicas]: the scenario of local replica r, a function of its GLOBAL id
        g = replica_base + r, so a shard's assignment (dist.shard) is the slice of the unsharded one.
        "round_robin": g mod S.  "blocks": S contiguous blocks over the n_total global replicas
        (default replica_base + n_replicas: pass the world's total for a shard), g * S // n_total."""
        g = int(replica_base) + np.arange(int(n_replicas), dtype=np.int64)
        s = self.n_scenarios
        if how == "round_robin":
            out = g % s
        elif how == "blocks":
            total = int(n_total) if n_total is not None else int(replica_base) + int(n_replicas)
            if total < int(replica_base) + int(n_replicas):
                raise ValueError("n_total is smaller than replica_base + n_replicas")
            out = g * s // total
        else:
            raise ValueError("how must be 'round_robin' or 'blocks'")
        return out.astype(np.int32)


def derived_stats(st: np.ndarray) -> dict:
    """ComputeStats' per-scenario figures from the sums (compute-stats-v2.cc:87-266):
    avg_e2e_delay = e2e_sum / e2e_n, loss_ratio = ov_lost / ov_injected, avg_cost = cost_sum / cost_n
    (NaN where the denominator is 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        def ratio(a, b):
            b = b.astype(np.float64)
            return np.where(b != 0, a.astype(np.float64) / np.where(b != 0, b, 1.0), np.nan)
        return {"avg_e2e_delay": ratio(st["e2e_sum"], st["e2e_n"]),
                "loss_ratio": ratio(st["ov_lost"], st["ov_injected"]),
                "avg_cost": ratio(st["cost_sum"], st["cost_n"])}
