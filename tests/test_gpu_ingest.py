"""prisma_ingest_transitions against the torch path of the same tree: every case runs
``buffers.add(env.transitions())`` into buffers A and the kernel path into buffers B from the same
log, the same progress mark and the same ring state, and requires them bit-identical (_both)."""
import functools

import numpy as np
import pytest
import torch

from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PrismaError
from prisma_amd.env import VecRoutingEnv
from prisma_amd.records import ST_PENDING
from prisma_amd.topology import DATA_DIR, Topology, sp_next_hop_table
from prisma_amd.trainer import QRoutingTrainer, ReplayBuffers, train_fused

import synth_topology as ST

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

FIELDS = ("obs", "next_obs", "action", "reward", "done", "replica", "next_idx", "count", "total")


def _buffers(env, size):
    return ReplayBuffers(env.topo.n_nodes, size, env.W, env.device)


def _clone(b):
    c = ReplayBuffers(b.N, b.size, b.W, b.device)
    for f in FIELDS:
        setattr(c, f, getattr(b, f).clone())
    return c


def _snapshot(b, env):
    return [getattr(b, f).cpu().numpy().tobytes() for f in FIELDS] + [env._consumed.cpu().numpy().tobytes()]


def _both(env, A, torch_path=None):
    """The torch path into A, the kernel path into a clone of A's earlier state, from the same
    progress mark; both must agree on every ring tensor and on the mark.  -> (transitions, B)."""
    c0 = env._consumed.clone()
    B = _clone(A)
    tr = env.transitions() if torch_path is None else torch_path()
    A.add(tr)
    cA = env._consumed.clone()
    env._consumed = c0
    env.ingest_transitions(B)
    torch.cuda.synchronize()
    for f in FIELDS:
        a, b = getattr(A, f), getattr(B, f)
        assert torch.equal(a, b), (f, int((a != b).sum()), int(a.numel()))
    assert torch.equal(env._consumed, cA), (env._consumed.tolist()[:8], cA.tolist()[:8])
    return tr, B


@functools.lru_cache(maxsize=None)
def _table(name):
    return sp_next_hop_table(Topology.example(name, 0, 1.0))


def _abilene_rollout(size, launches=4, hops=257, **kw):
    """Abilene at load factor 2.0, SP table with eps 0.3: `launches` launches of `hops` hops,
    compared after each.  -> (env, A, the launches' transitions, the rings' next_idx before each)."""
    env = VecRoutingEnv("abilene", load_factor=2.0, n_replicas=3, **kw)
    table = torch.from_numpy(_table("abilene")).to(env.device)
    A = _buffers(env, size)
    env.reset()
    trs, nexts = [], []
    for _ in range(launches):
        env.run(table, hops, explore=0.3)
        nexts.append(A.next_idx.clone())
        trs.append(_both(env, A)[0])
    assert np.all(env.counters()["error"] == 0)
    return env, A, trs, nexts


def test_drops_and_several_nodes():
    env, A, trs, _ = _abilene_rollout(4096)
    hop = torch.cat([t["hop"] for t in trs])
    node = torch.cat([t["node"] for t in trs]).long()
    rep = torch.cat([t["replica"] for t in trs]).long()
    assert int(hop.sum()) > 0 and int((~hop).sum()) > 0, (int(hop.sum()), int((~hop).sum()))
    seen = torch.zeros((env.topo.n_nodes, env.R), dtype=torch.bool, device=env.device)
    seen[node, rep] = True
    assert int((seen.sum(1) >= 2).sum()) >= 2
    assert int(A.total.sum()) == int(node.numel())
    # nothing new: a second ingest straight after the first changes nothing
    before = _snapshot(A, env)
    env.ingest_transitions(A)
    torch.cuda.synchronize()
    assert _snapshot(A, env) == before
    env.close()


def test_ring_overflow():
    env, A, trs, nexts = _abilene_rollout(64)
    over = wrapped = False
    for t, nx in zip(trs, nexts):
        cnt = torch.bincount(t["node"].long(), minlength=env.topo.n_nodes)
        over |= bool((cnt > 64).any())
        wrapped |= bool(((nx + cnt >= 64) & (cnt > 0)).any())
    assert over and wrapped
    assert torch.all(A.count == 64)
    env.close()


def test_log_ring_wrap():
    env, A, _, _ = _abilene_rollout(4096, launches=5, hops=300, log_capacity=1024)
    assert int(env.counters()["dec_count"].min()) > 1024
    env.close()


def test_trailing_pending_record():
    """The external path: every step leaves each live replica's newest record pending, which the
    ingest must neither emit nor pass."""
    env = VecRoutingEnv("abilene", n_replicas=5, sim_time_s=30.0)
    A = _buffers(env, 256)
    gen = torch.Generator().manual_seed(3)
    deg = torch.from_numpy(env.topo.degrees.astype(np.int64)).to(env.device)
    obs, info = env.reset()
    held = 0
    for _ in range(8):
        node = info["node"].long().clamp_min(0)
        a = (torch.randint(0, 1 << 20, (env.R,), generator=gen).to(env.device) % deg[node].clamp_min(1)).to(torch.int32)
        step = {}

        def torch_path():
            step["out"] = env.step(a)
            return step["out"][3]["transitions"]

        _both(env, A, torch_path)
        obs, _, _, info = step["out"]
        dec = env._dec_counts()
        last = env.engine.gather_records(torch.arange(env.R, device=env.device, dtype=torch.int32),
                                         ((dec - 1).clamp_min(0) % env.engine.log_capacity).to(torch.int32))
        pending = ((last.view(torch.int32)[:, 7] >> 8) & 0xFF) == ST_PENDING
        assert torch.equal(env._consumed[pending], dec[pending] - 1)       # held back at the pending record
        held += int(pending.sum())
    assert held > 0 and int(A.total.sum()) > 0
    env.close()


def test_scan_chunk_boundary():
    """1 025 replicas: the scan's second chunk of replicas holds one."""
    env = VecRoutingEnv("abilene", n_replicas=1025, sim_time_s=30.0)
    A = _buffers(env, 4096)
    env.reset()
    env.run(torch.from_numpy(_table("abilene")).to(env.device), 64, explore=0.3)
    tr, _ = _both(env, A)
    assert int((tr["replica"] == 1024).sum()) > 0
    env.close()


def _er256():
    return Topology.example("er256"), np.load(f"{DATA_DIR}/er256/sp_next_hop_table.npy")


@pytest.mark.parametrize("case", ["geant", "star55", "er256-memory"])
def test_widths_and_node_ids(case):
    kw = dict(n_replicas=2, sim_time_s=30.0)
    explore = 0.3
    if case == "geant":
        topo = Topology.example("geant", 0, 1.0)
        table = sp_next_hop_table(topo)
        want_w = 8
    elif case == "star55":
        topo = ST.build("star55")
        table = sp_next_hop_table(topo)
        want_w = 56
    else:
        topo, table = _er256()
        kw.update(n_replicas=1, engine=PRISMA_ENGINE_MEMORY)
        explore = None                                         # (exploration is refused on that engine)
        want_w = None
    env = VecRoutingEnv(topo=topo, **kw)
    if want_w is not None:
        assert env.W == want_w and env.engine.rec_bytes == 32 + 4 * want_w
    else:
        assert env.engine.engine_kind == PRISMA_ENGINE_MEMORY
    A = _buffers(env, 1024)
    env.reset()
    env.run(torch.from_numpy(table).to(env.device), 512, explore=explore)
    tr, _ = _both(env, A)
    assert int(tr["node"].numel()) > 100
    if case == "er256-memory":
        assert int(tr["node"].max()) > 127
    env.close()


def test_episode_end_inside_a_launch():
    env = VecRoutingEnv("abilene", n_replicas=2, sim_time_s=1.0, auto_reset=1, log_capacity=16384)
    A = _buffers(env, 8192)
    table = torch.from_numpy(_table("abilene")).to(env.device)
    env.reset()
    for _ in range(3):
        env.run(table, 2000, explore=0.3)
        _both(env, A)
    cnt = env.counters()
    assert np.all(cnt["error"] == 0) and np.all(cnt["episode"] >= 2)
    env.close()


def test_train_fused_end_to_end():
    out = []
    for fused in (False, True):
        env = VecRoutingEnv("abilene", n_replicas=64, sim_time_s=30.0)
        tr = QRoutingTrainer(env.topo, "routing", batch_size=32, buffer_size=1 << 15, seed=0, n_replicas=64)
        losses = train_fused(env, tr, 6, 256, fused_ingest=fused)
        torch.cuda.synchronize()
        out.append((tr, losses, env._consumed.clone()))
        env.close()
    (ta, la, ca), (tb, lb, cb) = out
    for f in FIELDS:
        assert torch.equal(getattr(ta.buffers, f), getattr(tb.buffers, f)), f
    assert int(ta.buffers.total.sum()) > 0 and torch.equal(ca, cb)
    assert torch.equal(ta.transitions_seen, tb.transitions_seen)
    assert len(la) == 6 and la == lb


def test_refusals():
    env = VecRoutingEnv("abilene", n_replicas=2, sim_time_s=30.0)
    env.reset()
    env.run(torch.from_numpy(_table("abilene")).to(env.device), 200, explore=0.3)
    N, W = env.topo.n_nodes, env.W

    def wrong_w():
        return ReplayBuffers(N, 64, W + 4, env.device)

    def wrong_n():
        return ReplayBuffers(N + 1, 64, W, env.device)

    def non_contiguous():
        b = _buffers(env, 64)
        b.action = torch.zeros((64, N), dtype=torch.int64, device=env.device).t()
        return b

    def cpu_tensor():
        b = _buffers(env, 64)
        b.count = b.count.cpu()
        return b

    def size_zero():
        return ReplayBuffers(N, 0, W, env.device)

    for make in (wrong_w, wrong_n, non_contiguous, cpu_tensor, size_zero):
        b = make()
        before = [getattr(b, f).cpu().numpy().tobytes() for f in FIELDS]
        c0 = env._consumed.clone()
        with pytest.raises((PrismaError, ValueError)):
            env.ingest_transitions(b)
        torch.cuda.synchronize()
        assert [getattr(b, f).cpu().numpy().tobytes() for f in FIELDS] == before, make.__name__
        assert torch.equal(env._consumed, c0), make.__name__
    pr = QRoutingTrainer(env.topo, "routing", batch_size=32, buffer_size=64, n_replicas=2, prioritized_replay=True)
    with pytest.raises(ValueError, match="prioritized"):
        env.ingest_transitions(pr.buffers)
    # and the call still works afterwards
    _both(env, _buffers(env, 64))
    env.close()
