"""A fresh data arrival (a packet off an access link: no previous decision) issues no load of a
previous decision record and waits for none (engine_core.h on_arrive); a relayed one still does.
Bit-exact against the CPU oracle at the smallest shapes where that path can go wrong: an empty log,
one-hop launches that open and end on fresh arrivals, a 1 024-record log that wraps while fresh
and relayed arrivals interleave, fresh packets next to their destination and dropped at their first
decision, the fused and the general kernel alternating on one env, an episode end inside a launch,
and one case for each other instance set (DQN-buffer MLP, tunnelled overlay, --train, stochastic
routing, memory-resident engine).

Every case asserts on the records themselves that it holds what it names (fresh arrivals, relays
after a wrap, the drop): premises() below, checked on the CPU oracle when the cases were chosen."""
import functools

import numpy as np
import pytest
import torch

import synth_topology as S
from prisma_amd import optrouting
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaEngine
from prisma_amd.records import ST_DESTINATION, ST_DROPPED
from prisma_amd.topology import Topology, sp_next_hop_table

from parity_util import OracleChain, assert_counters_equal, first_difference, random_table, run_fused_both

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

R_BASE = 7
CAP = 1024                               # the smallest log the validator accepts
# Abilene at load factor 2.0 with 4 096-byte buffers (8 packets): queues drop fresh packets, and no
# packet's previous decision gets CAP records old (with the default 16 260 bytes one does after
# about 1 900 hops, and the episode stops on PRISMA_EBIT_LOGWRAP)
MIXED = dict(sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=CAP, max_buffer=4096)


def premises(rec, cap):
    """What a run's records hold, from the records alone (prev < 0: a fresh arrival)."""
    prev = rec["prev"].astype(np.int64)
    idx = np.arange(len(rec))
    fresh = prev < 0
    relay = ~fresh
    # the slot a fresh packet's ring entry names: dst | start parity << 8 | uid << 9 (f_make)
    named = (rec["dst"].astype(np.int64) | ((rec["start_s"].astype(np.int64) & 1) << 8)
             | (rec["uid"].astype(np.int64) << 9)) & (cap - 1)
    named_slots = np.zeros(cap, dtype=bool)
    named_slots[named[fresh]] = True
    dest_of_relay = idx[(rec["status"] == ST_DESTINATION) & relay]
    # A fresh entry travels on its node's access link, which carries nothing else, so "the same
    # link's next packet" is never a relay; the nearest thing the records name is the same NODE's
    # next arrival: a fresh arrival at a node whose next arrival, on a switch link, is a relay
    order = np.lexsort((idx, rec["node"]))
    node_s, fresh_s = rec["node"][order], fresh[order]
    same_node = node_s[:-1] == node_s[1:]
    return dict(
        records=len(rec), fresh=int(fresh.sum()), relays=int(relay.sum()),
        relays_after_wrap=int((relay & (idx >= cap)).sum()),
        max_age=int((idx - prev)[relay].max()) if relay.any() else 0,
        fresh_then_relay=int((fresh[:-1] & relay[1:]).sum()), relay_then_fresh=int((relay[:-1] & fresh[1:]).sum()),
        fresh_then_fresh=int((fresh[:-1] & fresh[1:]).sum()),
        node_fresh_then_relay=int((same_node & fresh_s[:-1] & ~fresh_s[1:]).sum()),
        # a relayed packet whose previous record lies in a slot that some fresh entry's bits name
        relay_in_named_slot=int(named_slots[prev[relay] & (cap - 1)].sum()),
        fresh_dropped=int((fresh & (rec["status"] == ST_DROPPED)).sum()),
        # a packet that reaches its destination one hop after its fresh arrival
        fresh_next_to_dst=int(fresh[prev[dest_of_relay]].sum()))


def assert_fresh_fields(rec):
    """A fresh arrival's record: no previous decision, no reward."""
    fresh = rec[rec["prev"] < 0]
    assert len(fresh) and np.all(fresh["prev"] == -1) and np.all(fresh["reward"] == 0.0)
    assert np.all(fresh["reward"].view(np.uint64) == 0)                      # (+0.0 bit for bit)
    relay = rec[rec["prev"] >= 0]
    assert np.all(relay["reward"] > 0.0)


def drive(oracle_mod, topo, params, policy, R, budgets, label, kernel_prefix=None):
    """One launch per budget on the engine; after EVERY launch the new records and the counters of
    every replica against an OracleChain.  Returns (counters, per replica: the engine's records of
    each launch)."""
    kind, pol = policy
    eng = PrismaEngine(topo, params, R)
    chains = [OracleChain(oracle_mod, topo, params, params["replica_base"] + r, policy) for r in range(R)]
    try:
        if kernel_prefix is not None:
            name = eng.kernel_name if kind == "table" else eng.kernel_name_mlp
            assert name.startswith(kernel_prefix), (label, name)
        eng.reset(0)
        dev = torch.from_numpy(np.ascontiguousarray(pol)).cuda()
        checked = [0] * R
        prev_hops = np.zeros(R, dtype=np.uint64)
        out = [[] for _ in range(R)]
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
                assert ch.advance(hops) == hops, (label, k, r)
                ch.sync_episode(int(c["episode"]))
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
                out[r].append(got.copy())
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


def test_first_decisions_one_hop_per_launch(oracle_mod):
    """dec_count 0, an empty log: the first arrivals are all fresh.  16 launches of one hop each."""
    topo, table = _abilene(1.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=CAP)
    _, out = drive(oracle_mod, topo, params, ("table", table), 3, [1] * 16, "first decisions",
                   kernel_prefix="prisma_step_kernel_fused_t<")
    for r, launches in enumerate(out):
        rec = np.concatenate(launches)
        assert rec[0]["prev"] == -1 and rec[0]["reward"] == 0.0, (r, rec[0])
        assert_fresh_fields(rec)
        p = premises(rec, CAP)
        assert p["fresh"] >= 4 and p["relays"] >= 1 and p["fresh_then_relay"] >= 1, (r, p)
        # a launch whose records are all fresh arrivals: it opens and ends on one
        assert any(np.all(x["prev"] < 0) for x in launches), r


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    """3 replicas x 10 launches of 600 hops on Abilene at load factor 2.0 with a 1 024-record log."""
    topo, table = _abilene(2.0)
    params = engine_params(topo, **MIXED)
    _, out = drive(oracle_mod, topo, params, ("table", table), 3, [600] * 10, "mixed",
                   kernel_prefix="prisma_step_kernel_fused_t<")
    return [np.concatenate(x) for x in out]


def test_mixed_stream_on_a_wrapping_log(mixed):
    for r, rec in enumerate(mixed):
        p = premises(rec, CAP)
        print(f"mixed replica {r}: {p}")
        assert p["records"] >= 6 * CAP and p["max_age"] < CAP, (r, p)         # the log wrapped 6 times
        assert p["fresh"] >= 1000 and p["relays_after_wrap"] >= 1000, (r, p)
        # after a fresh arrival: a relay next, and a relay whose record lies where a fresh entry points
        assert p["fresh_then_relay"] >= 100 and p["relay_then_fresh"] >= 100 and p["fresh_then_fresh"] >= 100, (r, p)
        assert p["relay_in_named_slot"] >= 10 and p["node_fresh_then_relay"] >= 100, (r, p)


def test_fresh_next_to_its_destination_and_fresh_dropped(mixed):
    for r, rec in enumerate(mixed):
        p = premises(rec, CAP)
        assert p["fresh_next_to_dst"] >= 10 and p["fresh_dropped"] >= 10, (r, p)
        assert_fresh_fields(rec)
        drop = rec[(rec["prev"] < 0) & (rec["status"] == ST_DROPPED)]
        assert np.all(drop["prev"] == -1) and np.all(drop["reward"] == 0.0)
        dest = rec[(rec["status"] == ST_DESTINATION) & (rec["prev"] >= 0)]
        first = rec[dest["prev"]]                  # (the run's records from 0: prev indexes them)
        near = first[first["prev"] < 0]
        assert len(near) >= 10 and np.all(near["prev"] == -1) and np.all(near["reward"] == 0.0)
        # and the destination's own record has the one-hop reward of that decision
        assert np.all(dest["reward"] > 0.0)


def test_fused_and_general_kernels_alternate(oracle_mod):
    """prisma_run's fused instance and prisma_step's general one on one env, at load factor 2.0."""
    from test_gpu_fused_instances import Pair
    topo, table = _abilene(2.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=8192,
                           max_buffer=4096)
    p = Pair(oracle_mod, topo, params, 2, table, "alternating")
    try:
        assert p.eng.kernel_name.startswith("prisma_step_kernel_fused_t<")
        assert p.eng.kernel_name_step.startswith("prisma_step_kernel_t<")
        p.steps(30, "first external")
        for hops in (1, 150, 400):
            p.run(hops, f"fused {hops}")
            p.steps(30, f"external after fused {hops}")
        p.run(400, "last fused")
        for r, o in enumerate(p.orcs):
            rec = o.records()
            pr = premises(rec, 8192)
            assert pr["fresh"] >= 100 and pr["relays"] >= 100 and pr["fresh_then_relay"] >= 30, (r, pr)
            assert_fresh_fields(rec)
    finally:
        p.close()


def test_episode_end_inside_a_launch(oracle_mod):
    """auto_reset: the launch's budget ends in episode 1, whose arrivals the restart loop (the second
    event-loop copy) takes -- the first of them fresh again."""
    topo, table = _abilene(1.0)
    R = 2
    params = engine_params(topo, sim_time_s=0.75, ping_as_obs=1, auto_reset=1, replica_base=R_BASE,
                           log_capacity=4096)
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
    cnt, out = drive(oracle_mod, topo, params, ("table", table), R, [budget], "episode end",
                     kernel_prefix="prisma_step_kernel_fused_t<")
    for r in range(R):
        rec = out[r][0]
        assert int(cnt[r]["episode"]) == 1
        ep1 = rec[rec["episode"] == 1]
        assert len(ep1) > 50 and ep1[0]["prev"] == -1 and ep1[0]["reward"] == 0.0, (r, ep1[:1])
        assert np.any(ep1["prev"] >= 0) and np.all(ep1["prev"][ep1["prev"] >= 0] >= len(rec) - len(ep1))
        assert_fresh_fields(rec)


# ---- one case for each other instance set ---------------------------------------------------------

def _check_refs(refs, cap, label, fresh=100, relays=100, wrap=False, dropped=0):
    for r, rec in enumerate(refs):
        p = premises(rec, cap)
        print(f"{label} replica {r}: {p}")
        assert p["fresh"] >= fresh and p["relays"] >= relays and p["fresh_dropped"] >= dropped, (label, r, p)
        assert p["fresh_then_relay"] >= 10 and p["relay_then_fresh"] >= 10, (label, r, p)
        if wrap:
            assert p["relays_after_wrap"] >= 100 and p["max_age"] < cap, (label, r, p)
        assert_fresh_fields(rec)


def test_mlp_instance(oracle_mod):
    """The in-kernel DQN-buffer MLP on Abilene (the register engine's MLP instance)."""
    from prisma_amd.policies import StackedQNet
    topo, _ = _abilene(2.0)
    params = engine_params(topo, **dict(MIXED, log_capacity=2048))
    net = StackedQNet(topo, "buffer", seed=7, device="cpu")
    cnt, refs = run_fused_both(oracle_mod, topo, params, 2, 2400, ("mlp", net.pack().numpy()), launches=3,
                               kernel=dict(ctrl=0), net_cpu=net, label="mlp")
    _check_refs(refs, 2048, "mlp", wrap=True)


def test_tunnelled_overlay(oracle_mod):
    """The 3-node overlay mesh on Abilene at load factor 20: the tunnelled (relay_ip) instance; most
    fresh packets are dropped at their first decision."""
    topo = Topology.example("overlay_full_mesh_3n_abilene", 0, 20.0)
    params = engine_params(topo, sim_time_s=30.0, ping_as_obs=1, replica_base=R_BASE, log_capacity=2048)
    cnt, refs = run_fused_both(oracle_mod, topo, params, 3, 3000, ("table", random_table(topo, 11)), launches=3,
                               kernel=dict(tunnels=1, ctrl=0, relay_ip=1), label="mesh3 lf 20")
    _check_refs(refs, 2048, "mesh3 lf 20", wrap=True, dropped=100)


def test_train_instance(oracle_mod):
    """--train (the CTRL instance): a relayed arrival echoes to its last hop, a fresh one does not
    (the node is the packet's source), so the echoes' bytes are the oracle's."""
    topo, table = _abilene(2.0)
    params = engine_params(topo, train=1, **MIXED)
    cnt, refs = run_fused_both(oracle_mod, topo, params, 3, 3000, ("table", table), launches=5,
                               kernel=dict(ctrl=1), label="train")
    assert np.all(cnt["bytes_signaling"] > 0)
    _check_refs(refs, CAP, "train", wrap=True, dropped=1)


def test_stochastic_instance(oracle_mod):
    """prisma_run_stochastic: the rule reads the previous record's action only for a relayed packet."""
    import test_gpu_opt_routing as OPT
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=5.0, replica_base=R_BASE, log_capacity=OPT.LOG)
    _, all_refs = OPT._run_and_compare(oracle_mod, topo, params, optrouting.path_split_routing(topo, 3, seed=1),
                                       "stochastic", hops=1500, launches=3, replicas=2, floors=(50, 50, 5))
    for per in all_refs:
        assert len(per) == 1
        _check_refs([per[0].records(0, per[0].n_records())], OPT.LOG, "stochastic")


@pytest.mark.parametrize("mlp", [0, 1], ids=["table", "mlp"])
def test_memory_resident_engine(oracle_mod, mlp):
    """l40_f100 of MEMORY_CASES forced onto the memory-resident engine."""
    from prisma_amd.policies import StackedQNet
    name = "l40_f100"
    topo = S.build_mem(name)
    params = S.mem_params(name)
    net = StackedQNet(topo, "buffer", seed=S.MLP_SEED, device="cpu") if mlp else None
    policy = ("mlp", net.pack().numpy()) if mlp else ("table", S.mem_table(name))
    cnt, refs = run_fused_both(oracle_mod, topo, params, S.R, 1500, policy, launches=3,
                               kernel=dict(engine=PRISMA_ENGINE_MEMORY, ctrl=0), net_cpu=net,
                               label=f"{name} memory engine mlp {mlp}")
    _check_refs(refs, params["log_capacity"], f"{name} mlp {mlp}")
