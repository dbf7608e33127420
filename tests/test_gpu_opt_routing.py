"""In-kernel stochastic multipath routing (prisma_run_stochastic, the reference's "opt" agent)
against the CPU oracle stepped under the host rule (opt_routing_util.OptSteppedOracle: the packet's
source and previous decision from the oracle's own records, nothing read from the GPU): records
byte for byte and the counters a stopped launch determines; a one-hot matrix against
prisma_run's table policy on the same env; the refusals.  Every case asserts on its own reference
that both branches of the rule are exercised, so a kernel that only draws, or only follows, cannot
pass unnoticed."""
import functools

import numpy as np
import pytest
import torch

from prisma_amd import engine as E
from prisma_amd import optrouting
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaEngine, PrismaError
from prisma_amd.env import VecRoutingEnv
from prisma_amd.topology import Topology, sp_next_hop_table

import synth_topology
from opt_routing_util import OptSteppedOracle
from parity_util import assert_counters_equal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

LOG = 16384
HUGE = 1 << 30
R, HOPS, LAUNCHES = 3, 3000, 2


@functools.lru_cache(maxsize=None)
def _topo(name):
    return Topology.example(name, 0, 1.0)


def _device_table(eng, routing):
    tab = eng.stochastic_table(routing)
    assert tab.dtype == torch.int32 and tab.is_cuda and tab.is_contiguous()
    assert np.array_equal(tab.cpu().numpy().view(np.uint32), optrouting.pack_routing(eng.topo, routing))
    return tab


def _reference(oracle_mod, topo, params, r, routing, total):
    """The first `total` records of replica r's log, over as many episodes as they span, and the
    oracles that produced them."""
    out, refs, base, ep = [], [], 0, 0
    while base < total:
        ref = OptSteppedOracle(oracle_mod, topo, params, params["replica_base"] + r, routing, episode=ep, base=base)
        ref.run(until_records=total - base)
        n = min(ref.n_records(), total - base)
        assert n > 0
        out.append(ref.records(0, n))
        refs.append(ref)
        base += n
        ep += 1
    return np.concatenate(out), refs


def _run_and_compare(oracle_mod, topo, params, routing, label, hops=HOPS, launches=LAUNCHES, replicas=R, pre=None,
                     floors=(1, 1, 0)):
    """`launches` launches of hops / launches hops each on `replicas` replicas; the records up to
    dec_count byte for byte against the stepped oracle.  floors: the least follows, draws and
    follows at an index other than 0 a replica's reference must hold."""
    eng = PrismaEngine(topo, params, replicas)
    assert eng.kernel_info()["ctrl"] == 0
    tab = _device_table(eng, routing)
    eng.reset(0)
    if pre:
        pre(eng)
    for _ in range(launches):
        eng.run_stochastic(tab, hops // launches)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    all_refs = []
    for r in range(replicas):
        c = cnt[r]
        assert int(c["error"]) == 0, (label, r, int(c["error"]))
        total = int(c["dec_count"])
        assert 0 < total <= LOG, (label, r, total)
        want, refs = _reference(oracle_mod, topo, params, r, routing, total)
        got = eng.records(r, 0, total, log_host=log)
        if got.tobytes() != want.tobytes():
            bad = next(i for i in range(total) if got[i].tobytes() != want[i].tobytes())
            raise AssertionError(f"{label} replica {r}: record {bad} of {total} differs\n engine {got[bad]}\n"
                                 f" oracle {want[bad]}")
        follows = sum(x.follows for x in refs)
        draws = sum(x.draws for x in refs)
        nonzero = sum(x.follows_nonzero for x in refs)
        print(f"{label} replica {r}: {total} records over {len(refs)} episode(s), {follows} followed ({nonzero} at an "
              f"index other than 0), {draws} drawn")
        assert follows >= floors[0] and draws >= floors[1] and nonzero >= floors[2], (label, r, follows, draws, nonzero)
        # the counters a launch stopped by its hop budget determines: every record but a
        # destination's is a hop, and within one episode they are the episode's own counters too
        hop_rec = want[want["status"] != 3]
        assert int(c["hops_total"]) == len(hop_rec), (label, r, int(c["hops_total"]), len(hop_rec))
        if len(refs) == 1:
            # (a pending decision's hop counts towards the launch's budget)
            assert int(c["episode_over"]) == 0 and int(c["hops_total"]) == (hops // launches) * launches
            assert int(c["hops"]) == len(hop_rec) and int(c["hop_deg_sum"]) == int(topo.degrees[hop_rec["node"]].sum())
        all_refs.append(refs)
    eng.close()
    return cnt, all_refs


@pytest.mark.parametrize("gen", ["path_split", "ecmp"])
def test_abilene(oracle_mod, gen):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=5.0, replica_base=5, log_capacity=LOG)
    routing = optrouting.path_split_routing(topo, 3, seed=1) if gen == "path_split" else optrouting.ecmp_routing(topo)
    # (the equal split's classes are shared by every edge of a node: it follows at index 0 or 1)
    _run_and_compare(oracle_mod, topo, params, routing, f"abilene {gen}",
                     floors=(200, 200, 20) if gen == "path_split" else (5, 200, 1))


def test_geant(oracle_mod):
    topo = _topo("geant")
    assert topo.obs_width == 8
    params = engine_params(topo, sim_time_s=5.0, log_capacity=LOG)
    _run_and_compare(oracle_mod, topo, params, optrouting.path_split_routing(topo, 3, seed=2), "geant",
                     floors=(200, 200, 20))


def test_tunnelled_overlay(oracle_mod):
    """Abilene on GEANT: the tunnelled instances, whose relay entries carry no source (the kernel
    walks the records' prev chain), and a table whose columns are not in the matrix's order."""
    topo = _topo("abilene_on_geant")
    params = engine_params(topo, sim_time_s=5.0, log_capacity=LOG)
    eng = PrismaEngine(topo, params, 1)
    ki = eng.kernel_info()
    eng.close()
    assert ki["tunnels"] == 1 and ki["ctrl"] == 0 and ki["relay_ip"] == 1
    _run_and_compare(oracle_mod, topo, params, optrouting.path_split_routing(topo, 3, seed=1), "abilene on geant",
                     floors=(200, 200, 20))


def _star_routing(topo, seed):
    """Random weights at the hub, the destination's edge boosted so packets arrive.  For pairs
    with s + t even the source leaf's edge carries the fraction of the hub's edge to t, so the hub
    follows to it (any index up to d - 1); for the others the leaves' edges carry 1.0 and the hub
    draws, also when a packet comes back from a wrong leaf."""
    rng = np.random.default_rng(seed)
    row = optrouting.edge_rows(topo)
    hub = int(np.argmax(topo.degrees))
    d = int(topo.degrees[hub])
    nb = topo.neighbors(hub)
    n = topo.n_nodes
    rt = np.zeros((n, n, int(row[-1])))
    for s in range(n):
        for t in range(n):
            if s == t or s == hub or t == hub:
                continue
            w = rng.random(d) * 0.9 / d + 1e-3             # distinct, each below 0.06
            w[nb.index(t)] = 0.5 + 0.01 * rng.random()
            rt[s, t, row[hub]: row[hub] + d] = w
            for leaf in nb:
                rt[s, t, row[leaf]] = 1.0
            if (s + t) % 2 == 0:
                rt[s, t, row[s]] = w[nb.index(t)]
    return rt, hub


@pytest.mark.parametrize("d", [17, 33, 55])
def test_wide_star(oracle_mod, d):
    """A hub of degree d: the entries' load, the scan and both ballots cross a 16-lane row (17),
    the 32-lane half (33) and reach lane 54 (55)."""
    topo = synth_topology.star(d, 64, 7)
    params = engine_params(topo, sim_time_s=5.0, log_capacity=LOG)
    routing, hub = _star_routing(topo, d)
    assert int(topo.degrees[hub]) == d and np.all(np.delete(topo.degrees, hub) == 1)
    _, refs = _run_and_compare(oracle_mod, topo, params, routing, f"star {d}", replicas=2, floors=(100, 100, 50))
    for per in refs:
        tr = [e for x in per for e in x.trace if e["v"] == hub]
        drawn = {e["action"] for e in tr if not e["followed"]}
        followed = {e["action"] for e in tr if e["followed"]}
        print(f"star {d}: {len(drawn)} distinct drawn hub actions (max {max(drawn)}), {len(followed)} followed "
              f"(max {max(followed)})")
        assert len(drawn) >= min(d, 16) and max(drawn) >= d // 2 and max(followed) >= d // 2
        if d > 16:
            assert any(a >= 16 for a in drawn) and any(a >= 16 for a in followed)
        if d > 32:
            assert any(a >= 32 for a in drawn) and any(a >= 32 for a in followed)


def test_257_hops_after_a_pending_decision(oracle_mod):
    """step(None) leaves every replica at a pending decision: the launch answers it by the rule
    (the first decision site, from the pending entry) and goes on for 257 hops."""
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=5.0, log_capacity=LOG)

    def pre(eng):
        _, mask, _ = eng.step(None)
        assert bool(mask.all())

    cnt, _ = _run_and_compare(oracle_mod, topo, params, optrouting.path_split_routing(topo, 3, seed=1),
                              "abilene after step()", hops=257, launches=1, pre=pre, floors=(10, 10, 1))
    assert np.all(cnt["hops_total"] == 257)


def test_pending_relay_decision_through_the_env(oracle_mod):
    """The same with pending decisions of relayed packets, so the first site reads the previous
    record: 40 steps under SP actions first.  Through VecRoutingEnv.run(model="opt")."""
    topo = _topo("abilene")
    routing = optrouting.path_split_routing(topo, 3, seed=1)
    sp = sp_next_hop_table(topo)
    table = torch.from_numpy(sp.astype(np.int64)).cuda()
    env = VecRoutingEnv(topo=topo, n_replicas=R, sim_time_s=5.0, log_capacity=LOG)
    eng = env.engine
    tab = _device_table(eng, routing)
    eng.reset(0)
    obs, mask, node = eng.step(None)
    for _ in range(40):
        obs, mask, node = eng.step(table[node.long(), obs[:, 0].long()].to(torch.int32))
    assert bool(mask.all())
    env.run(tab, 257, model="opt")
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    relayed = 0
    for r in range(R):
        total = int(cnt[r]["dec_count"])
        # the oracle: SP answers for the 40 stepped decisions, the rule from the pending one on
        ref = OptSteppedOracle(oracle_mod, topo, env.params, r, routing)
        for _ in range(40):
            k = ref.n_records() - 1
            rec = ref.o.records(k, 1)[0]
            v = int(rec["node"])
            a = int(sp[v, int(rec["dst"])])
            ref.src[k] = v if int(rec["prev"]) < 0 else ref.src[int(rec["prev"])]
            ref.dec[k] = (v, a)
            ref.obs = ref.o.step(a)
        relayed += int(ref.o.records(ref.n_records() - 1, 1)[0]["prev"] >= 0)
        ref.run(until_records=total)
        want = ref.records(0, total)
        got = eng.records(r, 0, total, log_host=log)
        assert int(cnt[r]["error"]) == 0 and int(cnt[r]["hops_total"]) == 40 + 257
        if got.tobytes() != want.tobytes():
            bad = next(i for i in range(total) if got[i].tobytes() != want[i].tobytes())
            raise AssertionError(f"replica {r}: record {bad} of {total} differs\n engine {got[bad]}\n oracle {want[bad]}")
        assert ref.follows > 5 and ref.draws > 5
    assert relayed > 0                                     # (some replica's pending packet had a previous hop)
    env.close()


def test_episode_end_inside_a_launch(oracle_mod):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=0.75, auto_reset=1, log_capacity=LOG)
    cnt, refs = _run_and_compare(oracle_mod, topo, params, optrouting.path_split_routing(topo, 3, seed=1),
                                 "abilene 0.75-s episodes", floors=(100, 100, 10))
    for r, per in enumerate(refs):
        assert len(per) >= 2 and int(cnt[r]["episode"]) >= 1, (r, len(per))     # the second event loop ran
        assert per[1].decisions > 50 and per[1].episode == 1 and per[1].base > 0


def test_all_zero_row(oracle_mod):
    """A node whose row is zero for every pair takes the uniform pick (W == 0); a whole episode,
    so every counter is compared."""
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=0.75, log_capacity=LOG)
    routing = optrouting.ecmp_routing(topo)
    row = optrouting.edge_rows(topo)
    v = int(np.argmax(topo.degrees))
    routing[:, :, row[v]: row[v + 1]] = 0.0
    eng = PrismaEngine(topo, params, R)
    tab = _device_table(eng, routing)
    eng.reset(0)
    eng.run_stochastic(tab, HUGE)
    torch.cuda.synchronize()
    cnt = eng.counters()
    log = eng.log_tensor().cpu().numpy()
    for r in range(R):
        ref = OptSteppedOracle(oracle_mod, topo, params, r, routing).run()
        want = ref.records()
        c = cnt[r]
        assert int(c["error"]) == 0 and int(c["episode_over"]) == 1 and int(c["dec_count"]) == len(want) <= LOG
        assert eng.records(r, 0, len(want), log_host=log).tobytes() == want.tobytes(), r
        assert_counters_equal(c, ref.counters(), r, " (all-zero row)")
        zero = [e for e in ref.trace if e["v"] == v]
        assert len(zero) > 50 and all(e["W"] == 0 and not e["followed"] for e in zero)
        assert {e["action"] for e in zero} == set(range(int(topo.degrees[v])))
    eng.close()


def test_one_hot_matrix_equals_the_table_policy():
    """routing = the SP table one-hot: every weight row is one-hot and every class 0, so each
    decision draws and lands on the SP action.  Against prisma_run(PRISMA_POLICY_TABLE) on the same
    env: log and counters byte for byte.  Independent of the host restatement of the rule."""
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=5.0, log_capacity=LOG)
    sp = sp_next_hop_table(topo)
    edges, _ = optrouting.reference_edges(topo)
    routing = np.zeros((topo.n_overlay, topo.n_overlay, len(edges)))
    row = optrouting.edge_rows(topo)
    for t in range(topo.n_nodes):
        for v in range(topo.n_nodes):
            if v != t:
                routing[:, t, row[v] + int(sp[v, t])] = 1.0
    eng = PrismaEngine(topo, params, R)
    dev = torch.from_numpy(sp).cuda()
    tab = _device_table(eng, routing)
    eng.reset(0)
    for _ in range(LAUNCHES):
        eng.run(dev, HOPS // LAUNCHES)
    torch.cuda.synchronize()
    want_log, want_cnt = eng.log_tensor().cpu().numpy().copy(), eng.counters().copy()
    eng.reset(0)
    for _ in range(LAUNCHES):
        eng.run_stochastic(tab, HOPS // LAUNCHES)
    torch.cuda.synchronize()
    got_log, got_cnt = eng.log_tensor().cpu().numpy(), eng.counters()
    assert np.all(got_cnt["error"] == 0) and np.all(got_cnt["hops_total"] == HOPS)
    assert got_cnt.tobytes() == want_cnt.tobytes()
    for r in range(R):
        n = int(got_cnt[r]["dec_count"])
        assert n > HOPS and got_log[r, :n].tobytes() == want_log[r, :n].tobytes(), r
    eng.close()


def _raw(eng, tab_ptr, words, hops=100):
    return E._lib.prisma_run_stochastic(eng.h, tab_ptr, words, hops, None)


# the library's refusals, whole: status PRISMA_ERR_CONFIG (-1) and the text
REFUSAL_MEMORY = ("prisma error -1: prisma_run_stochastic: the memory-resident engine has no instances with stochastic "
                  "routing")
REFUSAL_CTRL = ("prisma error -1: prisma_run_stochastic: this env runs the step kernels with the ctrl paths (train, "
                "notify_dest, ns-3 streams, or a tunnelled overlay with log_capacity >= 2^18), which have no instances "
                "with stochastic routing")


@pytest.mark.parametrize("kw", [dict(train=1), dict(engine=PRISMA_ENGINE_MEMORY)], ids=["train", "memory-engine"])
def test_refuses_by_config(kw):
    topo = _topo("abilene")
    params = engine_params(topo, sim_time_s=1.0, **kw)
    eng = PrismaEngine(topo, params, 2)
    assert eng.kernel_info()["ctrl"] == 1 or eng.engine_kind == PRISMA_ENGINE_MEMORY
    eng.reset(0)
    tab = _device_table(eng, optrouting.ecmp_routing(topo))
    assert _raw(eng, tab.data_ptr(), tab.numel()) == -1                        # PRISMA_ERR_CONFIG
    with pytest.raises(PrismaError) as err:
        eng.run_stochastic(tab, 100)
    assert str(err.value) == (REFUSAL_MEMORY if "engine" in kw else REFUSAL_CTRL)
    eng.run(torch.from_numpy(sp_next_hop_table(topo)).cuda(), 100)         # the engine still runs
    torch.cuda.synchronize()
    cnt = eng.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 100)
    eng.close()


def test_refuses_a_wrong_table():
    topo = _topo("abilene")
    eng = PrismaEngine(topo, engine_params(topo, sim_time_s=1.0), 2)
    eng.reset(0)
    good = _device_table(eng, optrouting.ecmp_routing(topo))
    no, T = topo.n_overlay, int(optrouting.edge_rows(topo)[-1])
    assert good.numel() == no * no * T
    assert _raw(eng, None, good.numel()) == -5                                 # null table: PRISMA_ERR_ARG
    assert _raw(eng, good.data_ptr(), good.numel() - 1) == -5                  # wrong tab_words
    assert _raw(eng, good.data_ptr(), good.numel() + T) == -5
    assert _raw(eng, good.data_ptr(), good.numel(), hops=0) == -5
    bad = [torch.zeros((no, no, T + 1), dtype=torch.int32, device="cuda"),     # shape
           torch.zeros(no * no * T, dtype=torch.int32, device="cuda"),
           torch.zeros((no, no, T), dtype=torch.int64, device="cuda"),         # dtype
           torch.zeros((no, no, T), dtype=torch.float32, device="cuda"),
           torch.zeros((no, no, T), dtype=torch.int32),                        # device
           torch.zeros((no, T, no), dtype=torch.int32, device="cuda").transpose(1, 2),   # contiguity
           np.zeros((no, no, T), dtype=np.uint32)]
    for t in bad:
        with pytest.raises(PrismaError, match="prisma_run_stochastic"):
            eng.run_stochastic(t, 100)
    torch.cuda.synchronize()
    assert int(eng.counters()["hops_total"].sum()) == 0
    eng.run_stochastic(good, 100)                                              # the engine still runs
    torch.cuda.synchronize()
    cnt = eng.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["hops_total"] == 100)
    eng.close()
