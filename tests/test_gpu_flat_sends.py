"""The lane-resident send as one straight-line body and the link's topology word (engine_core.h
link_send_lane, lane_links_bind, on_arrive) of the fused table instances with one link slot,
prisma_step_kernel_fused_t<1 | 2 | 4, 1, false, false>.  As tests/test_gpu_lane_links.py, whose
drive() runs here: every case goes launch by launch, and after EVERY launch the new records and
every counter of every replica are compared with an OracleChain byte for byte; drive() asserts
through kernel_name that a fused instance with one link slot ran, the cases assert which.

link_send_lane commits under per-lane predicates and takes H.seq, ev_launch and the flags from its
status word; a data arrival takes the far end of its link, that node's row pointer and degree from
one word of the link's lane.  Every case asserts on the ORACLE's side that the run holds what the
case names.  Checked on the CPU when the inputs were chosen (the oracle alone):
  * star(21, 64, 5), replicas 0-2, seed 100, 2 000 hops: the hub takes 940, 897 and 928 of the hops,
    the last leaf 38, 45 and 58, every node 9 or more; 144, 136 and 126 drops, 4 to 5 ping rounds;
  * Abilene, load 3.0, 4 000 hops, replicas 7-9: ctrl_dropped 14, 6 and 7 (pings refused by a full
    FIFO: link_send_lane's drop at the ping sites), 641, 661 and 614 data drops, peak_ring 34 to
    35, no error; each of the four launches holds drops and the start of a ping round;
  * l64_f64 (FS = 1), 1 000 hops, replicas 7-9: link 0 receives 54 to 67 packets, link 63 11 to 27;
    1, 5 and 16 drops.  l64_f129 (FS = 4), 1 200 hops: 23 to 31 and 14 to 19; 6, 2 and 8 drops;
  * Abilene, load 1.0, 300 hops in 76 launches of 1 and 7: 17, 33 and 23 of the 75 launch ends
    fall inside a switch link's transmission for certain (its completion follows within a ping's
    transmission time, the shortest there is); 313, 275 and 317 transmissions are started by a
    send on an idle transmitter (START: H.seq += 2), the rest by a dequeue."""
import numpy as np
import pytest
import torch

import synth_topology as S
from prisma_amd.config import engine_params
from prisma_amd.records import ST_DROPPED, ST_ENQUEUED
from prisma_amd.topology import Topology, sp_next_hop_table

from test_gpu_lane_links import EV_COMPLETE, EV_RECEIVE, R_BASE, drive, link_story, tx_times

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]


def _instance(fs):
    return f"prisma_step_kernel_fused_t<{fs}, 1, false, false>"


def _kernel_of(topo, params):
    from prisma_amd.engine import PrismaEngine
    eng = PrismaEngine(topo, params, 1)
    try:
        return eng.kernel_name
    finally:
        eng.close()


def _hops_of(rec, node=None):
    hop = (rec["status"] == ST_ENQUEUED) | (rec["status"] == ST_DROPPED)
    return int(hop.sum()) if node is None else int((hop & (rec["node"] == node)).sum())


def test_topology_word_at_the_instance_limits(oracle_mod):
    """A star of 21 leaves: 42 switch links and 22 access links fill the 64 lanes, the hub has the
    largest degree an LS = 1 instance can meet (21) and the last leaf the largest row pointer (41)."""
    topo = S.star(21, 64, 5)
    assert (topo.n_nodes, topo.n_links, topo.n_links + topo.n_nodes) == (22, 42, 64)
    assert int(topo.max_deg) == 21
    params = engine_params(topo, sim_time_s=30.0, seed=100, ping_as_obs=1, replica_base=0)
    assert _kernel_of(topo, params) == _instance(1)
    _, out = drive(oracle_mod, topo, params, sp_next_hop_table(topo), [500] * 4, "star21")
    for r, o in enumerate(out):
        rec = o["rec"]
        hub, last = _hops_of(rec, 0), _hops_of(rec, 21)
        every = min(_hops_of(rec, v) for v in range(topo.n_nodes))
        drops = int((rec["status"] == ST_DROPPED).sum())
        rounds = int(o["counters"]["ping_rounds"])
        print(f"star21 replica {r}: hub decides {hub}, node 21 {last}, least {every}, drops {drops}, ping rounds {rounds}")
        assert _hops_of(rec) == 2000
        assert hub >= 800 and last >= 25 and every >= 5 and drops >= 100 and rounds >= 3, (r, hub, last, every, drops, rounds)


def test_ping_sends_that_drop(oracle_mod):
    """Abilene at load factor 3.0: pings find full FIFOs and are refused (ctrl_dropped), at the ping
    round's, the ping-back's or the ping forward's send; data drops and ping rounds in one launch."""
    topo = Topology.example("abilene", 0, 3.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE)
    assert _kernel_of(topo, params) == _instance(2)
    budgets = [1000] * 4
    _, out = drive(oracle_mod, topo, params, sp_next_hop_table(topo), budgets, "abilene lf 3")
    for r, o in enumerate(out):
        rec, c = o["rec"], o["counters"]
        drops = int((rec["status"] == ST_DROPPED).sum())
        print(f"abilene lf 3 replica {R_BASE + r}: ctrl_dropped {int(c['ctrl_dropped'])}, data drops {drops}, "
              f"ping rounds {int(c['ping_rounds'])}, diag {o['diag']}")
        assert int(c["ctrl_dropped"]) >= 1 and int(c["error"]) == 0, (r, c)
        assert drops >= 300, (r, drops)
        # one launch with both: the hops of launch k are records' hops [1000 k, 1000 (k + 1)), and a
        # ping round starts every 0.2 s of the records' clock
        hop = np.flatnonzero((rec["status"] == ST_ENQUEUED) | (rec["status"] == ST_DROPPED))
        both = 0
        for k in range(len(budgets)):
            part = rec[hop[1000 * k]:hop[1000 * (k + 1) - 1] + 1]
            t0, t1 = int(part["t_ns"][0]), int(part["t_ns"][-1])
            both += int((part["status"] == ST_DROPPED).any() and t1 // 200_000_000 > t0 // 200_000_000)
        assert both >= 1, r


@pytest.mark.parametrize("case,fs,hops", [("l64_f64", 1, 1000), ("l64_f129", 4, 1200)])
def test_other_flow_slot_counts(oracle_mod, case, fs, hops):
    """The FS = 1 and FS = 4 gated instances (their own register allocations), links on lanes 0 and 63."""
    topo = S.build(case)
    assert topo.n_links + topo.n_nodes == 64
    params = S.case_params(case)
    assert _kernel_of(topo, params) == _instance(fs)
    _, out = drive(oracle_mod, topo, params, S.case_table(case), [hops // 2] * 2, case)
    for r, o in enumerate(out):
        tr = o["traces"][0]
        rx0 = int(((tr[:, 2] == EV_RECEIVE) & (tr[:, 3] == 0)).sum())
        rx63 = int(((tr[:, 2] == EV_RECEIVE) & (tr[:, 3] == 63)).sum())
        drops = int((o["rec"]["status"] == ST_DROPPED).sum())
        print(f"{case} replica {r}: link 0 receives {rx0}, link 63 {rx63}, drops {drops}")
        assert rx0 >= 5 and rx63 >= 3, (r, rx0, rx63)
        assert drops >= 1, (r, drops)


def test_launch_ends_between_a_send_and_its_elided_completion(oracle_mod):
    """Launches of 1 and 7 hops: most launches end with transmissions under way whose completions
    were elided, and the next launch's sends find them due.  H.seq and ev_launch (the counters' seq
    and events) are compared after every launch."""
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE)
    assert _kernel_of(topo, params) == _instance(2)
    budgets = []
    while sum(budgets) < 300:
        budgets.append((1, 7)[len(budgets) % 2])
    budgets[-1] -= sum(budgets) - 300
    assert sum(budgets) == 300 and len(budgets) >= 70
    _, out = drive(oracle_mod, topo, params, sp_next_hop_table(topo), budgets, "budgets 1 / 7")
    _, txp = tx_times(params)
    for r, o in enumerate(out):
        rec, tr = o["rec"], o["traces"][0]
        # a launch ends with its last hop: that record's time.  A switch link whose transmission
        # completes within a ping's transmission time after it was transmitting then
        hop = np.flatnonzero((rec["status"] == ST_ENQUEUED) | (rec["status"] == ST_DROPPED))
        ends = rec["t_ns"][hop[np.cumsum(budgets)[:-1] - 1]]
        tc = tr[(tr[:, 2] == EV_COMPLETE) & (tr[:, 3] < topo.n_links), 0]
        inside = sum(int(((tc > t) & (tc <= t + txp)).any()) for t in ends)
        st = link_story(tr, params, topo.n_links, topo.n_nodes)
        idle = sum(s["due"] for s in st[:topo.n_links])
        print(f"budgets 1 / 7 replica {r}: launch ends inside a transmission {inside} of {len(ends)}, "
              f"transmissions started by a send {idle}")
        assert inside >= 10 and idle >= 200, (r, inside, idle)
