"""The lane-resident link handlers (engine_core.h link_send_lane / on_complete_lane) of the fused
table instances with one link slot: the FIFO and transmitter updates run in the link's own lane and
only the owner lane commits.  Every case drives the engine launch by launch and compares, after
EVERY launch, the new records and every counter of every replica with an OracleChain byte for byte,
and asserts through kernel_name that the gated instance ran.

Every case also asserts on the ORACLE's side (its event trace, diag() and records) that the run
holds what the case names.  link_story() reads a link's history off the trace: transmission i of a
link ends at its EV_COMPLETE, and it started inside the previous EV_COMPLETE of that link (a dequeue
behind the transmitter: on_complete) exactly when the two lie one transmission time apart;
otherwise a send started it on an idle transmitter (link_send's START path, hx = e).  In the
engine's terms:
  * a transmission started by a send, not the link's first: the send found the completion before it
    elided and DUE (unless a launch ended in between: lazy_resolve settles those; the cases count
    far more such sends than launches x links);
  * the first dequeue of a busy period: its packet was sent while the transmitter was busy with an
    empty queue -- a send that found an elided completion NOT yet due;
  * two dequeues in a row: the second packet waited behind an older head.

Checked on the CPU when the inputs were chosen (the oracle alone; the figures are replica 7's):
  * l64_f64, 2 400 hops: links 0 and 63 receive 105 and 72 packets (replicas 8, 9: 105 / 50, 119 / 54);
  * Abilene, load 1.0, 3 600 hops: the busiest switch link carries 243 packets (capacity 44), the
    busiest access link 196 (capacity 8); 1 539 sends find an idle transmitter after an earlier
    transmission (launches x links = 123), 520 busy periods go on with a dequeue, 1 915 dequeues
    follow a dequeue;
  * Abilene, load 2.0, 6 000 hops: 865 drops, peak_ring 35 (30 data packets, pings, the wire), 11
    ping rounds, no previous decision more than 1 186 records old (the log holds 8 192);
  * Abilene, load 4.0, 3 000 hops: 1 787 flow sends, 1 787 access-link receives, 500 drops;
  * delay0 / delay3 / buf542 on Abilene at load 3, 3 000 hops: WCAP 2 / 8 / 4, data_max 30 / 30 / 1,
    369 / 369 / 957 drops, max_wire 2 / 4 / 3;
  * 2-s episodes: the first ends after 2 859 / 2 790 / 2 552 hops, the second holds 2 494 or more
    sends on an idle transmitter.

Admission by packet count on an access link: the case the issue names -- a load at which the oracle
DROPS on an access link -- does not exist.  An access link admits 1 000 packets and transmits at
10^6 x degree times the switch links' rate (a 542-B packet in 2 to 4 ns), so its queue never holds
two packets at any load the switch links survive, and its ring of 8 entries would fail the replica
(PRISMA_EBIT_RING) long before 1 000 queued.  What exists is the packet-count SIDE of the admission
select, which every flow send takes on its access-link lane: the access-link case asserts from the
trace that every flow send was admitted and received (no drop) while the switch links next to them
drop by bytes at load factor 4."""
import functools

import numpy as np
import pytest
import torch

import param_cases as PC
import synth_topology as S
from prisma_amd.config import engine_params
from prisma_amd.engine import PrismaEngine
from prisma_amd.records import ST_DROPPED
from prisma_amd.topology import Topology, sp_next_hop_table

from parity_util import OracleChain, assert_counters_equal, first_difference

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

R = 3
R_BASE = 7
FUSED = "prisma_step_kernel_fused_t<"
EV_SEND, EV_COMPLETE, EV_RECEIVE = 2, 3, 4             # oracle/prisma_oracle.c event kinds


def tx_times(params):
    """Transmission times (ns) of a data packet and of a ping on a switch link."""
    bps = params["link_bps"]
    return PC._ns((params["packet_size"] + 30) * 8 / bps), PC._ns(38 * 8 / bps)


def link_story(trace, params, n_links, n_nodes):
    """Per link (switch links, then the access link of every node), from an oracle trace: packets
    received, transmissions started by a send on an idle transmitter after an earlier transmission
    (`due`), busy periods that went on with a dequeue (`not_due`), dequeues that followed a
    dequeue (`older`)."""
    txs = tx_times(params)
    out = []
    for l in range(n_links + n_nodes):
        tc = trace[(trace[:, 2] == EV_COMPLETE) & (trace[:, 3] == l), 0]
        gaps = np.diff(tc)
        deq = np.isin(gaps, txs) if l < n_links else np.zeros(len(gaps), dtype=bool)
        first_deq = deq & ~np.concatenate(([False], deq[:-1]))
        out.append(dict(received=int(((trace[:, 2] == EV_RECEIVE) & (trace[:, 3] == l)).sum()),
                        due=int((~deq).sum()), not_due=int(first_deq.sum()),
                        older=int((deq[1:] & deq[:-1]).sum())))
    return out


def drive(oracle_mod, topo, params, table, budgets, label, replicas=R):
    """One fused launch per budget; after EVERY launch the new records and the counters of every
    replica against an OracleChain.  Returns (counters, per replica: records, oracle traces of the
    episodes, oracle diag of the last episode)."""
    eng = PrismaEngine(topo, params, replicas)
    chains = [OracleChain(oracle_mod, topo, params, params["replica_base"] + r, ("table", table))
              for r in range(replicas)]
    traced = []

    def trace_on(ch):
        ch.o.enable_trace(True)
        traced.append(ch.o)

    try:
        assert eng.kernel_name.startswith(FUSED), (label, eng.kernel_name)
        ki = eng.kernel_info()
        assert (ki["link_slots"], ki["tunnels"], ki["ctrl"]) == (1, 0, 0), (label, ki)
        for ch in chains:
            trace_on(ch)
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        checked = [0] * replicas
        prev_hops = np.zeros(replicas, dtype=np.uint64)
        recs = [[] for _ in range(replicas)]
        for k, hops in enumerate(budgets):
            eng.run(dev, hops)
            torch.cuda.synchronize()
            cnt = eng.counters()
            log = eng.log_tensor().cpu().numpy()
            delta = cnt["hops_total"] - prev_hops
            prev_hops = cnt["hops_total"].copy()
            for r, ch in enumerate(chains):
                c = cnt[r]
                assert int(c["error"]) == 0, (label, k, r, int(c["error"]))
                assert int(delta[r]) == hops, (label, k, r, int(delta[r]))
                left = hops
                while left > 0:                        # (advance(), with the trace on in every episode)
                    got = ch._run(left)
                    left -= got
                    ch.hops_total += got
                    if left > 0:
                        assert params["auto_reset"] and int(ch.o.counters()["episode_over"]) == 1, (label, k, r)
                        ch._next_episode()
                        trace_on(ch)
                while ch.ep < int(c["episode"]):
                    assert ch._run(1) == 0, (label, k, r)
                    ch._next_episode()
                    trace_on(ch)
                new = int(c["dec_count"]) - checked[r]
                assert 0 < new <= eng.log_capacity, (label, k, r, new)
                ref = ch.records(checked[r], new)
                assert len(ref) == new, (label, k, r, len(ref), new)
                got = eng.records(r, checked[r], new, log_host=log)
                bad = first_difference(got, ref)
                assert bad is None, (f"{label} launch {k} replica {r}: record {checked[r] + bad} differs\n"
                                     f" engine {got[bad]}\n oracle {ref[bad]}")
                assert_counters_equal(c, ch.counters(), r, f" ({label}, launch {k})")
                checked[r] += new
                recs[r].append(got.copy())
        out = []
        for r, ch in enumerate(chains):
            eps = [o for _, o, _ in ch.done] + [ch.o]
            out.append(dict(rec=np.concatenate(recs[r]), traces=[o.trace() for o in eps], diag=ch.o.diag(),
                            counters=ch.o.counters().copy()))
        return cnt, out
    finally:
        eng.close()
        for ch in chains:
            for _, o, _ in ch.done:
                o.close()
            ch.o.close()


@functools.lru_cache(maxsize=None)
def _abilene(lf):
    topo = Topology.example("abilene", 0, lf)
    return topo, sp_next_hop_table(topo)


def test_links_at_both_ends_of_the_lane_range(oracle_mod):
    """l64_f64 (22 nodes, 21 edges): 42 switch links + 22 access links = 64, one per lane; link 0
    and link 63 (node 21's access link) both carry traffic."""
    topo = S.build("l64_f64")
    assert topo.n_links + topo.n_nodes == 64
    params = S.case_params("l64_f64")
    _, out = drive(oracle_mod, topo, params, sp_next_hop_table(topo), [800] * 3, "l64_f64")
    for r, o in enumerate(out):
        st = link_story(o["traces"][0], params, topo.n_links, topo.n_nodes)
        print(f"l64_f64 replica {r}: link 0 {st[0]}, link 63 {st[63]}")
        assert st[0]["received"] >= 10 and st[63]["received"] >= 5, (r, st[0], st[63])


@pytest.fixture(scope="module")
def light(oracle_mod):
    """Abilene at load factor 1.0, 3 replicas x 3 launches of 1 200 hops."""
    topo, table = _abilene(1.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE)
    _, out = drive(oracle_mod, topo, params, table, [1200] * 3, "abilene lf 1")
    return topo, params, [link_story(o["traces"][0], params, topo.n_links, topo.n_nodes) for o in out], out


def test_ring_indices_wrap_on_switch_and_access_links(light):
    """More packets through one link than its ring holds: tail, txp and head all wrap."""
    topo, params, stories, _ = light
    size = PC.sizing(params, topo)
    assert size["qs"] == 44 and max(8, size["WCAP"]) == 8
    for r, st in enumerate(stories):
        sw = max(s["received"] for s in st[:topo.n_links])
        acc = max(s["received"] for s in st[topo.n_links:])
        print(f"abilene lf 1 replica {r}: busiest switch link {sw} packets, busiest access link {acc}")
        assert sw > 3 * 44 and acc > 3 * 8, (r, sw, acc)


def test_elided_completions_found_due_and_not_due(light):
    topo, params, stories, _ = light
    launches, links = 3, topo.n_links + topo.n_nodes
    for r, st in enumerate(stories):
        due = sum(s["due"] for s in st[:topo.n_links])
        not_due = sum(s["not_due"] for s in st[:topo.n_links])
        print(f"abilene lf 1 replica {r}: sends that found a completion due {due}, not yet due {not_due}")
        # (a launch's end settles at most one elided completion per link before a send finds it)
        assert due - launches * links >= 500 and not_due >= 200, (r, due, not_due)


def test_idle_transmitter_and_older_head(light):
    """A send on an idle transmitter with an empty queue (it transmits its own packet: no ring read)
    and a completion that dequeues a packet which itself waited behind an older head."""
    topo, params, stories, out = light
    for r, st in enumerate(stories):
        idle = sum(s["due"] for s in st) + sum(1 for s in st if s["received"])
        older = sum(s["older"] for s in st[:topo.n_links])
        print(f"abilene lf 1 replica {r}: sends on an idle transmitter {idle}, dequeues behind a dequeue {older}")
        assert idle >= 1000 and older >= 50, (r, idle, older)


def test_byte_limit_with_pings_queued(oracle_mod):
    """Abilene at load factor 2.0: the 16 260-B FIFOs (30 data packets) fill and drop, with the
    pings of several rounds queued among the data."""
    topo, table = _abilene(2.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE)
    data_max = PC.sizing(params, topo)["data_max"]
    assert data_max == 30
    _, out = drive(oracle_mod, topo, params, table, [1500] * 4, "abilene lf 2")
    for r, o in enumerate(out):
        drops = int((o["rec"]["status"] == ST_DROPPED).sum())
        print(f"abilene lf 2 replica {r}: drops {drops}, diag {o['diag']}, ping rounds {int(o['counters']['ping_rounds'])}")
        assert drops >= 100 and o["diag"]["peak_ring"] >= data_max + 1, (r, drops, o["diag"])
        assert int(o["counters"]["ping_rounds"]) >= 3, r


def test_access_links_admit_by_packet_count(oracle_mod):
    """The packet-count side of the admission (see the module docstring: no load drops on an access
    link): at load factor 4 every flow send is admitted on its access link while the switch links
    drop by bytes."""
    topo, table = _abilene(4.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE)
    _, out = drive(oracle_mod, topo, params, table, [1500] * 2, "abilene lf 4")
    for r, o in enumerate(out):
        tr = o["traces"][0]
        sends = int((tr[:, 2] == EV_SEND).sum())
        acc_rx = int(((tr[:, 2] == EV_RECEIVE) & (tr[:, 3] >= topo.n_links)).sum())
        drops = int((o["rec"]["status"] == ST_DROPPED).sum())
        print(f"abilene lf 4 replica {r}: flow sends {sends}, access-link receives {acc_rx}, drops {drops}")
        # (a packet sent in the last nanoseconds may still be on its access link)
        assert sends >= 1000 and sends - acc_rx <= topo.n_nodes and drops >= 100, (r, sends, acc_rx, drops)


@pytest.mark.parametrize("case,wcap,data_max", [("delay0", 2, 30), ("delay3", 8, 30), ("buf542", 4, 1)])
def test_wire_shapes(oracle_mod, case, wcap, data_max):
    """0-ms links (2 wire slots; arrival and completion at the same instant), 3-ms links (8 wire
    slots), a buffer of one data packet."""
    topo = PC.case_topo(case, "abilene")
    params = PC.case_params(case, "abilene")
    size = PC.sizing(params, topo)
    assert (size["WCAP"], size["data_max"]) == (wcap, data_max), size
    _, out = drive(oracle_mod, topo, params, PC.table("abilene"), [1500] * 2, case)
    for r, o in enumerate(out):
        drops = int((o["rec"]["status"] == ST_DROPPED).sum())
        print(f"{case} replica {r}: drops {drops}, diag {o['diag']}")
        assert drops >= 100 and o["diag"]["max_wire"] >= 2, (r, drops, o["diag"])


def test_episode_end_inside_a_launch(oracle_mod):
    """2-s episodes with auto_reset: the launch's budget ends in episode 1, so the second event-loop
    copy and lazy_resolve run on link state the new handlers wrote."""
    topo, table = _abilene(1.0)
    params = engine_params(topo, sim_time_s=2.0, ping_as_obs=1, auto_reset=1, replica_base=R_BASE)
    e = []
    for r in range(R):
        ch = OracleChain(oracle_mod, topo, params, R_BASE + r, ("table", table))
        e0 = ch._run(1 << 30)
        ch._next_episode()
        e.append((e0, ch._run(1 << 30)))
        ch.o.close()
        ch.done[0][1].close()
    e = np.array(e)
    budget = int(e[:, 0].max() + e[:, 1].min() // 2)
    assert e[:, 0].max() < budget < e.sum(axis=1).min()
    cnt, out = drive(oracle_mod, topo, params, table, [budget, 300], "episode end")
    for r, o in enumerate(out):
        assert int(cnt[r]["episode"]) == 1 and len(o["traces"]) == 2, r
        ep1 = o["rec"][o["rec"]["episode"] == 1]
        st = link_story(o["traces"][1], params, topo.n_links, topo.n_nodes)
        assert len(ep1) > 300 and sum(s["due"] for s in st) >= 100 and sum(s["not_due"] for s in st) >= 10, r


def test_step_and_run_alternate(oracle_mod):
    """prisma_step's general instance keeps the uniform handlers, prisma_run's fused one has the
    lane-resident ones: the state image goes back and forth between the two forms."""
    from test_gpu_fused_instances import Pair
    topo, table = _abilene(2.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, max_buffer=4096)
    p = Pair(oracle_mod, topo, params, R, table, "alternating")
    try:
        assert p.eng.kernel_name.startswith(FUSED)
        assert p.eng.kernel_name_step.startswith("prisma_step_kernel_t<")
        p.steps(30, "first external")
        for hops in (1, 150, 400):
            p.run(hops, f"fused {hops}")
            p.steps(30, f"external after fused {hops}")
        p.run(400, "last fused")
        for r, o in enumerate(p.orcs):
            rec = o.records()
            assert int((rec["status"] == ST_DROPPED).sum()) >= 10 and len(rec) >= 1000, r
    finally:
        p.close()
