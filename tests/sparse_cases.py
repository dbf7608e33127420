"""Sparse traffic over full-length episodes: the case table tests/test_sparse_long.py (CPU: the
oracle's own run of each case) and tests/test_gpu_sparse_long.py (GPU parity) both import.

Two regimes no loaded, short run reaches:

* an idle network -- the next event lies 2^32 - 1 ns (4.29 s) or more ahead, so every 32-bit
  saturated offset of the event selection saturates and the exact 64-bit path decides
  (engine_core.h select_event; prisma_engine_mem.hip wave_min_key_exact), and the offsets between
  2^31 and 2^32 - 2 ns just below it;
* a late clock -- t up to 4.095e12 ns: the device forms of t / 1000 and t / 10^9, the microsecond
  state above 2^31 (after 2147.5 s), the 12-bit packet start second with its top bit set (after
  2048 s), ping rounds up to k = 4094 and the ping delay as a difference of two large doubles.

Every case: sim_time_s = 4095 (the host's limit), seed 105, 3 replicas from replica_base 7, a log
of 65 536 records (a whole episode's, so every record is compared), the shortest-path table.  Load
factors of 0.0002 to 0.002 give flows of 1 to 129 bit/s (ceil(base * load factor)): mean gaps of up
to 4 096 s between a flow's packets, flows that never send within the episode included.

The oracle's run of each case, per replica 7 / 8 / 9 (tests/test_sparse_long.py prints these):
"idle gaps": consecutive events 2^32 - 1 ns or more apart in OracleSim.trace(); "half gaps": those
in [2^31, 2^32 - 1) ns; "late": records with start_s >= 2048; "prev late": records whose previous
record lies at t >= 2^31 us; "ties": records with t_ns % 1000 == 500 (py_micros' tie branch).

  case        hops               events                idle gaps    half gaps    late               prev late       ties      rounds
  idle        1879/1763/1827     6757/6450/6506        339/356/340  182/165/174  1374/1312/1240     911/860/832     0/0/5     4
  idle_geant  5710/5609/5472     61895/61507/61188     206/205/216  479/466/464  3894/3798/3641     2693/2583/2521  4/9/12    136
  idle_ns3    1791/1768/1763     106559/106549/106497  421/419/407  421/417/424  1255/1293/1260     823/879/824     3/0/0     818
  ctrl        8546/8344/8350     145714/144783/144597  25/33/37     385/393/389  6007/5890/5949     4069/3927/3964  30/12/14  818
  pings       1879/1763/1827     509827/509520/509576  0/0/0        0/0/0        1374/1312/1240     911/860/832     0/0/5     4094
  busy        16743/16663/16827  59762/59563/59738     3/1/6        167/169/152  11754/11912/12078  7877/7973/8094  16/8/27   40
  tunnelled   2610/2551/2587     36175/35744/36067     340/328/340  272/287/276  1763/1813/1790     1190/1212/1209  8/10/6    81

Every episode ends between t = 4085 and 4095 s with 2 512 to 23 845 records.  Every case's three
replicas together meet py_micros' tie under seed 105 (`idle` and `pings` on replica 9 alone,
`idle_ns3` on replica 7 alone), so no case needed a seed of its own.  `pings` is `idle` with a ping
round every second (the same flows, so the same hops).  GEANT's
identity overlay has 506 flows here: 8 blocks of 64 on either engine.
"""
from __future__ import annotations

import functools

import numpy as np

from prisma_amd.topology import Topology, sp_next_hop_table

R = 3
REPLICA_BASE = 7
SIM_TIME_S = 4095.0
SEED = 105
LOG = 1 << 16
IDLE_NS = (1 << 32) - 1                # an event gap from here on saturates every 32-bit offset
HALF_NS = 1 << 31
LATE_S = 2048                          # the 12-bit start second's top bit
LATE_US = 1 << 31                      # the microsecond state's top bit (2147.48 s)


def _c(topo, load, ping, hops, idle=0, half=0, **over):
    """Topology and load factor, ping_interval_s, the hop budget (about 1.5 x the episode's hops),
    the idle and half gaps every replica's run must have at the least, the other overrides of
    config.engine_params.  (Under seed 105 every case's three replicas together meet py_micros'
    tie, so no case needed a seed of its own.)"""
    return dict(topo=topo, load=load, hops=hops, idle=idle, half=half, over=dict(over, ping_interval_s=ping))


CASES = {
    # no ping round but four: the flows alone, the longest gaps
    "idle": _c("abilene", 0.0002, 1000, 2799, idle=100, half=1),
    # 506 flows: 8 flow blocks and one group on the memory-resident engine, (8, 2) on the register one
    "idle_geant": _c("geant", 0.0002, 30, 8499, idle=100, half=1),
    # ns-3's MRG32k3a streams: other exponential gaps, a ping round every 5 s
    "idle_ns3": _c("abilene", 0.0002, 5, 2700, idle=100, half=1, rng="ns3"),
    # the ctrl instances: --train echoes and destination notifications at late time
    "ctrl": _c("abilene", 0.001, 5, 12750, idle=10, half=1, train=1, notify_dest=1),
    # a ping round every second: ping_send_s up to k = 4094, no idle gap (and none meant)
    "pings": _c("abilene", 0.0002, 1.0, 2799),
    # ten times idle's load: the most records at late time
    "busy": _c("abilene", 0.002, 100, 25050),
    # the tunnelled kernels, under the SP table (a random table loops its packets: 40 000 hops
    # reach 160 s)
    "tunnelled": _c("abilene_on_geant", 0.0005, 50, 3900, idle=10),
}
IDLE_CASES = [n for n, c in CASES.items() if c["idle"]]
MLP_CASES = ["idle", "idle_geant", "ctrl"]      # the SP-equivalent weights' runs (identity overlays)
# the memory-resident engine's runs (it takes the ctrl paths: param_cases.MEMORY_CASES has --train cases)
MEMORY_RUNS = [("idle_geant", "table"), ("idle_geant", "mlp"), ("idle", "table"), ("pings", "table"), ("ctrl", "table")]
SHAPES = {"abilene": (2, 1), "geant": (8, 2), "abilene_on_geant": (2, 1)}     # (flow_slots, link_slots)


@functools.lru_cache(maxsize=None)
def case_topo(name):
    return Topology.example(CASES[name]["topo"], 0, CASES[name]["load"])


def case_params(name, **kw):
    """engine_params of a case: the common set-up, the case's overrides, the caller's."""
    from prisma_amd.config import engine_params
    args = dict(sim_time_s=SIM_TIME_S, replica_base=REPLICA_BASE, log_capacity=LOG, seed=SEED)
    args.update(CASES[name]["over"])
    args.update(kw)
    return engine_params(case_topo(name), **args)


@functools.lru_cache(maxsize=None)
def table(name):
    return sp_next_hop_table(case_topo(name))


# ---- DQN-buffer weights that decide as the shortest-path table does -------------------------------
# A randomly initialised StackedQNet loops its packets (60 000 hops reach 80 to 160 s), so it cannot
# carry the MLP instances -- other instantiations of the same event loop -- to late time.  These
# weights can: W1[u, dst, a] = 1 at the SP action a, W2 and W3 pass units 0 to 31 through, W4[u, a,
# a] = -1, every bias 0, so without the buffers branch Q = expm1(-1) at the SP action and 0 elsewhere.
# The buffers branch enters through hidden units 32 to 63, which nothing else uses: with |Wb| <= WB
# and the LayerNorm output's sum of magnitudes <= deg, a branch unit stays within WB * deg, the ELUs
# and the pass-through layers shrink it or keep it, and 32 units times |W4| <= w4 move a Q's
# pre-activation by BRANCH_BOUND = 0.08 at the most.  The argmin is then the SP action by
# expm1(-0.92) against expm1(-0.08): 0.52.  This drives the MLP kernels through the two regimes; the
# MLP's arithmetic is other suites' business.
WB = 0.05
BRANCH_BOUND = 0.08


def sp_equivalent_net(topo):
    """StackedQNet(topo, "buffer") on the CPU with the weights above, and its packed weights (numpy)."""
    import torch
    from prisma_amd.policies import StackedQNet
    net = StackedQNet(topo, "buffer", seed=0, device="cpu")
    Bw, Hw, NH = net.dims
    assert (Bw, Hw, NH) == (32, 64, 2) and topo.max_deg <= Bw
    sp = sp_next_hop_table(topo)
    w4 = BRANCH_BOUND / (Bw * WB * topo.max_deg)
    rng = np.random.default_rng(1)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        for u in topo.overlay_nodes:
            deg = int(topo.degrees[u])
            for i, dst in enumerate(topo.overlay_nodes):
                if dst != u:
                    net.W1[u, i, int(sp[u, dst])] = 1.0
            net.Wb[u, :deg, :] = torch.from_numpy(rng.uniform(-WB, WB, (deg, Bw)).astype(np.float32))
            for j in range(2 * Bw):
                net.W2[u, j, j] = 1.0
                net.W3[u, j, j] = 1.0
            for a in range(deg):
                net.W4[u, a, a] = -1.0
            net.W4[u, Bw:2 * Bw, :deg] = torch.from_numpy(rng.uniform(-w4, w4, (Bw, deg)).astype(np.float32))
    return net, net.pack().numpy()


@functools.lru_cache(maxsize=None)
def net(name):
    return sp_equivalent_net(case_topo(name))


def policy(name, kind):
    return ("mlp", net(name)[1]) if kind == "mlp" else ("table", table(name))


# ---- the oracle's own run of a case ---------------------------------------------------------------
def gaps(t_ns):
    """(idle gaps, half gaps) of a sorted series of times that starts from t = 0."""
    d = np.diff(np.asarray(t_ns, dtype=np.int64), prepend=0)
    return int((d >= IDLE_NS).sum()), int(((d >= HALF_NS) & (d < IDLE_NS)).sum())


def summary(recs, trace=None):
    """What the ledger lists of one replica's records (and event trace)."""
    prev = recs["prev"].astype(np.int64)
    has = prev >= 0
    out = dict(records=len(recs), late=int((recs["start_s"] >= LATE_S).sum()),
               max_start_s=int(recs["start_s"].max()),
               prev_late=int((recs["t_ns"][prev[has]] >= LATE_US * 1000).sum()),
               ties=int((recs["t_ns"] % 1000 == 500).sum()), record_gaps=gaps(recs["t_ns"])[0])
    if trace is not None:
        out["idle"], out["half"] = gaps(trace[:, 0])
    return out


@functools.lru_cache(maxsize=None)
def oracle_runs(name, kind="table"):
    """The case's R replicas on the oracle alone under the table (with the event trace) or the
    SP-equivalent weights: (hops run, records, counters, event trace or None) each."""
    import oracle as O
    O.build()
    out = []
    for r in range(R):
        o = O.OracleSim(case_topo(name), case_params(name), replica=REPLICA_BASE + r)
        _, pol = policy(name, kind)
        if kind == "table":
            o.enable_trace()
            got = o.run_table(pol, CASES[name]["hops"])
        else:
            got = o.run_mlp(pol, CASES[name]["hops"])
        out.append((got, o.records(), o.counters(), o.trace() if kind == "table" else None))
        o.close()
    return out
