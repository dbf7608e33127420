"""Link, buffer, packet and ping parameters away from the reference's defaults (500 kbit/s, 1 ms,
16 260 B, 512 B, 0.2 s, a 5-word moving average): the case matrix tests/test_param_matrix.py (CPU:
the plan, the sizing and the oracle's own run) and tests/test_gpu_param_matrix.py (GPU parity)
both import.

The parameters decide how prisma_create lays a replica out: the wire slots per link (WCAP), the
ping-back delay slots per responder (PBK), the ring capacity per switch link (qs), how many data
packets a byte-limited FIFO holds (data_max), the moving-average window.  sizing() restates the
host formulas in plain Python; on identity overlays its ring_entries must equal prisma_plan's.

Every case: 3 replicas from replica_base 7, a 6-s episode, seed 105, 3 000 hops (the 64-B-packet
cases: 9 000) over 2 launches, a log of 8 192 records, on Abilene (load factor 3), GEANT (2) and
Abilene on GEANT (3)."""
from __future__ import annotations

import functools

import numpy as np

from prisma_amd.topology import Topology, sp_next_hop_table

R = 3
REPLICA_BASE = 7
SIM_TIME_S = 6.0
SEED = 105
LOG = 8192
H = 3000                               # hops per case, over 2 launches on the GPU

TOPOS = {"abilene": ("abilene", 0, 3.0), "geant": ("geant", 0, 2.0), "abilene_on_geant": ("abilene_on_geant", 0, 3.0)}
IDENTITY = ("abilene", "geant")
TUNNELLED = "abilene_on_geant"
MEM_MAX_WIRE = 16                      # the memory-resident engine's wire slots (engine_layout.h kMemMaxWire)
Q_WIN = 4                              # LDS FIFO window of the tunnelled kernels (engine_layout.h kQWin)


def _c(wcap, pbk, qs, data_max=30, load=1.0, hops=H, **over):
    """WCAP, PBK and qs (identity overlays: Abilene and GEANT size alike), data_max; a factor on
    the topologies' load; the hops of the fused parity runs; the overrides of config.engine_params."""
    return dict(wcap=wcap, pbk=pbk, qs=qs, data_max=data_max, load=load, hops=hops, over=over)


# 64-B packets: 3 000 hops are 0.3 s and one ping round; 9 000 reach 2 to 4 rounds and fill the
# 172-packet FIFOs until they drop (12 000 would outrun the log of 8 192 records: LOGWRAP).  A run
# then writes more records than the log holds, and the parity runs compare its last 8 192.
H_PKT64 = 9000


# The sizing classes are worked out from the formulas (sizing() below), not read off the library;
# tests/test_param_matrix.py holds both to them.  Replica 7's oracle run under the SP table
# (Abilene on GEANT: random_table(topo, 11)) over the case's hops, as abilene / geant /
# abilene_on_geant (tests/test_param_matrix.py prints these for every replica):
#
#   case                 max_wire  FIFO + wire  drops           ping rounds
#   delay0               2/2/2     34/32/39     369/11/631      5/3/6
#   delay3               4/4/5     35/33/40     369/11/639      5/3/6
#   delay8               4/4/5     35/33/40     366/13/639      5/3/7
#   delay6_pkt64_train   12/12/11  245/160/260  616/0/1445      3/2/4       (9 000 hops)
#   delay8_train         7/6/7     63/52/66     388/15/661      5/3/7
#   cap5M                5/4/5     33/8/33      14/0/176        1/1/1
#   delay35_pkt64        26/26/27  199/124/201  418/0/857       3/2/4       (9 000 hops)
#   delay28_pkt64_train  36/36/35  266/177/293  618/0/1348      3/2/4       (9 000 hops)
#   buf541               2/2/3     2/2/3        3000/3000/3000  8/5/12
#   buf542               3/3/3     4/4/4        957/534/1273    5/3/7
#   buf162600            3/3/3     148/41/145   0/0/0           5/3/6
#   pkt1470              3/3/3     16/15/22     733/285/1120    12/7/16
#   pkt1470_train_nn     3/3/-     26/25/-      771/303/-       12/7/-
#   ping10ms_ma64, _ma1  3/3/3     73/57/150    321/3/794       114/76/150
#   ping50ms_train       4/4/4     67/56/78     395/17/695      22/15/28
#   ping100s             2/2/2     32/31/32     362/9/620       0/0/0
#   penalty0, _12_5      3/3/3     35/32/39     368/11/633      5/3/6
#   sim750ms             3/3/3     32/30/36     5/0/23          3/3/3       (1467/2970/1148 hops)
#
# (FIFO + wire: the most entries one switch link's ring held at once, or_diag's peak_ring.)
CASES = {
    # arrival and tx-complete of a packet at the same instant; 2 wire slots, below the tunnelled
    # kernels' 4-slot FIFO window
    "delay0": _c(2, 4, 42, link_delay_ms=0),
    # LR_WT + 3 * 8 > 32: the memory-resident engine's first 64-word link record
    "delay3": _c(8, 4, 48, link_delay_ms=3),
    "delay8": _c(16, 4, 64, link_delay_ms=8),
    # 30-B echoes 0.48 ms apart on a 6-ms wire: the memory-resident engine's deepest wire
    "delay6_pkt64_train": _c(16, 4, 384, data_max=172, hops=H_PKT64, link_delay_ms=6, packet_size=64, train=1),
    "delay8_train": _c(32, 4, 128, link_delay_ms=8, train=1),                    # register only
    # ten times the load, so that the tenfold links still fill: drops on Abilene (14 / 47 / 44 on
    # replicas 7-9; none at the plain load), none on GEANT
    "cap5M": _c(32, 2, 96, load=10.0, link_cap=5_000_000),
    "delay35_pkt64": _c(64, 4, 256, data_max=172, hops=H_PKT64, link_delay_ms=35, packet_size=64),
    "delay28_pkt64_train": _c(64, 4, 448, data_max=172, hops=H_PKT64, link_delay_ms=28, packet_size=64, train=1),
    "buf541": _c(4, 2, 12, data_max=0, max_buffer=541),             # every hop is a drop
    "buf542": _c(4, 2, 12, data_max=1, max_buffer=542),
    "buf162600": _c(4, 32, 364, data_max=300, max_buffer=162600),
    "pkt1470": _c(4, 4, 24, data_max=10, packet_size=1470),
    # NN echoes: 8 + 8 (degree + 1) B per node, so identity overlays only
    "pkt1470_train_nn": _c(4, 4, 40, data_max=10, packet_size=1470, train=1, signaling_type="NN"),
    # 64 ping rounds and more: the 64-word moving-average window wraps; pings are dropped
    # (seed 108: under 105 GEANT's replica 9 drops no ping; found by an oracle search of 100-139)
    "ping10ms_ma64": _c(4, 64, 148, ping_interval_s=0.01, ma_size=64, seed=108),
    "ping10ms_ma1": _c(4, 64, 148, ping_interval_s=0.01, ma_size=1, seed=108),
    "ping50ms_train": _c(4, 16, 96, ping_interval_s=0.05, train=1),
    "ping100s": _c(4, 2, 40, ping_interval_s=100),                  # no ping round in the episode
    "penalty0": _c(4, 4, 44, loss_penalty=0.0),
    "penalty12_5": _c(4, 4, 44, loss_penalty=12.5),
    # the episode ends inside the run (seed 108: under 105 GEANT's replica 8 is still running
    # after 3 000 hops; the same search)
    "sim750ms": _c(4, 4, 44, sim_time_s=0.75, seed=108),
}
IDENTITY_ONLY = ("pkt1470_train_nn",)                               # refused on abilene_on_geant
# 64 wire slots and rings of 448 entries on GEANT's 74 + 23 links are over 180 KiB of LDS: beyond the
# register-resident engine, and the memory-resident one takes 16 wire slots at the most
NO_ENGINE = (("delay28_pkt64_train", "geant"),)
WCAP64 = ("delay35_pkt64", "delay28_pkt64_train")
MEMORY_CASES = [n for n, c in CASES.items() if c["wcap"] <= MEM_MAX_WIRE]
MEMORY_REFUSED = [n for n, c in CASES.items() if c["wcap"] > MEM_MAX_WIRE]

# ---- what tests/test_gpu_param_matrix.py runs (about 100 tests; GEANT dropped from a variant
# before a case): (case, topology, policy) ---------------------------------------------------------
REGISTER_RUNS = [(n, t, p) for n in CASES for t, p in (("abilene", "table"), ("geant", "table"), ("abilene", "mlp"))
                 if (n, t) not in NO_ENGINE]
MEMORY_RUNS = [(n, t, p) for n in MEMORY_CASES for t, p in (("geant", "table"), ("abilene", "mlp"))]
TUNNELLED_RUNS = ["delay0", "delay8", "delay28_pkt64_train", "buf541", "buf542", "ping10ms_ma64"]
EXPLORE_RUNS = [("delay0", "geant"), ("delay35_pkt64", "abilene"), ("buf542", "abilene")]
STEP_RUNS = [("delay35_pkt64", "abilene", "register"), ("buf541", "geant", "register"),
             ("delay6_pkt64_train", "abilene", "memory")]


@functools.lru_cache(maxsize=None)
def topo(name, load=1.0):
    n, tm, lf = TOPOS[name]
    return Topology.example(n, tm, lf * load)


def case_topo(case, topo_name):
    return topo(topo_name, CASES[case]["load"])


@functools.lru_cache(maxsize=None)
def table(name):
    """The table policy of a topology: shortest paths, on the tunnelled overlay a random table."""
    from parity_util import random_table
    return random_table(topo(name), 11) if name == TUNNELLED else sp_next_hop_table(topo(name))


@functools.lru_cache(maxsize=None)
def net(name):
    """The torch DQN-buffer model of a topology on the CPU and its packed weights (numpy)."""
    from prisma_amd.policies import StackedQNet
    n = StackedQNet(topo(name), "buffer", seed=21, device="cpu")
    return n, n.pack().numpy()


def policy(name, kind):
    return ("mlp", net(name)[1]) if kind == "mlp" else ("table", table(name))


def case_params(case, topo_name, **kw):
    """engine_params of a case on a topology: the common set-up, the case's overrides, the caller's."""
    from prisma_amd.config import engine_params
    args = dict(sim_time_s=SIM_TIME_S, replica_base=REPLICA_BASE, log_capacity=LOG, seed=SEED)
    args.update(CASES[case]["over"])
    args.update(kw)
    return engine_params(case_topo(case, topo_name), **args)


def _ns(s):
    return int(s * 1e9 + 0.5)                                       # numerics.h sec_to_ns


def _pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def sizing(params, tp):
    """The host sizing of prisma_create (prisma_engine.hip build_layout) restated: WCAP, PBK,
    data_max and, on identity overlays, qs and ring_entries = E * qs + N * max(8, WCAP).  Without
    big signalling (no case here has it)."""
    bps, delay, buf = params["link_bps"], params["link_delay_ns"], params["max_buffer_bytes"]
    data_size = params["packet_size"] + 30                          # UDP 8 + IP 20 + PPP 2
    ival = float(np.float32(params["ping_interval_s"]))             # a C float in prisma_params_t
    txd = _ns(data_size * 8 / bps)
    min_tx = _ns(30 * 8 / bps) if params["train"] else _ns(38 * 8 / bps)      # a 0-B echo, an 8-B ping
    wcap = _pow2(max(2, delay // min_tx + 2))
    data_max = buf // data_size
    tx_s = txd * 1e-9
    drain_s = buf * 8.0 / bps + tx_s
    out = dict(WCAP=wcap, data_max=data_max)
    if tp.identity:
        span = 2.0 * (drain_s + delay * 1e-9)
        ctrl = 2 * (int(span / ival) + 3)
        echoes = int(drain_s / tx_s) + 2 if params["train"] else 0
        qs = (data_max + ctrl + echoes + wcap + wcap - 1) // wcap * wcap
        out.update(qs=qs, ring_entries=tp.n_links * qs + tp.n_nodes * max(8, wcap))
    else:
        hop_s = buf * 8.0 / bps + 2.0 * tx_s + delay * 1e-9
        span = 2.0 * int(tp.tun_len.max()) * hop_s
        out.update(ring_multiple=max(wcap, Q_WIN))
    out["PBK"] = _pow2(int(span / ival) + 2)
    return out
