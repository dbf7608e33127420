"""The reduced DQN-buffer models (buffer_lite, buffer_lighter, buffer_lighter_2, buffer_lighter_3)
off the device: StackedQNet, pack(), the SavedModel importer, the trainer and the C-ABI's argument
checks for the new kinds, against the host restatement of tests/lightq_util.py (itself pinned to the
oracle in tests/test_lightq_restatement.py)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from prisma_amd import engine, savedmodel as sm
from prisma_amd.config import AGENT_MODEL_KINDS, AGENT_TYPES
from prisma_amd.policies import BUFFER_DIMS, StackedQNet, buffer_floats, buffer_layer_names
from prisma_amd.topology import Topology
from prisma_amd.trainer import QRoutingTrainer, nn_param_count

import lightq_util as LQ

NEW_KINDS = ["buffer_lite", "buffer_lighter", "buffer_lighter_2", "buffer_lighter_3"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stackedqnet_init_hashes.json")


def _topo(name):
    return Topology.example(name, 0, 1.0)


# ---- 3. each new kind ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NEW_KINDS)
def test_pack_layout(kind):
    topo = _topo("abilene")
    N, D = topo.n_nodes, topo.max_deg
    B, H, NH = BUFFER_DIMS[kind]
    net = StackedQNet(topo, kind, seed=2, device="cpu").requires_grad_(False)
    w = net.pack()
    want = N * N * B + N * B + N * D * B + N * B + N * 2 * B * H + N * H + (NH - 1) * (N * H * H + N * H) + N * H * D + N * D
    assert w.dtype == torch.float32 and w.numel() == want == buffer_floats(kind, N, D) == engine.model_floats(kind, N, D)
    assert engine.model_floats("buffer", N, D) == engine.dqn_buffer_floats(N, D) == buffer_floats("buffer", N, D)
    assert ("W3" in dict(net.named_parameters())) == (NH == 2)
    o = 0
    for wn in buffer_layer_names(kind):
        for p in (getattr(net, wn), getattr(net, "b" + wn[1:])):
            assert torch.equal(w[o:o + p.numel()], p.detach().flatten()), wn
            o += p.numel()
    assert o == w.numel()
    assert tuple(net.W1.shape) == (N, N, B) and tuple(net.Wb.shape) == (N, D, B)
    assert tuple(net.W2.shape) == (N, 2 * B, H) and tuple(net.W4.shape) == (N, H, D)
    # he_uniform: a kernel within sqrt(6 / fan_in), a bias within sqrt(6 / its length)
    u = int(np.argmax(topo.degrees))
    assert float(net.W2[u].abs().max()) <= np.sqrt(6.0 / (2 * B)) and float(net.b2[u].abs().max()) <= np.sqrt(6.0 / H)
    assert float(net.W2[u].abs().max()) > 0.5 * np.sqrt(6.0 / (2 * B))
    offs = LQ.HostMLP.__new__(LQ.HostMLP)
    offs.B, offs.H, offs.NH, offs.N, offs.D = B, H, NH, N, D
    assert offs.offsets()["_total"][0] == want


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_q_values_against_per_node_sequential(kind):
    """q_values against one literal torch model per node, built from the packed slices."""
    topo = _topo("geant")
    N, D = topo.n_nodes, topo.max_deg
    B, H, NH = BUFFER_DIMS[kind]
    net = StackedQNet(topo, kind, seed=4, device="cpu")
    w = net.pack().numpy()
    host = LQ.HostMLP.__new__(LQ.HostMLP)
    host.B, host.H, host.NH, host.N, host.D = B, H, NH, N, D
    offs = host.offsets()
    P = {k: torch.from_numpy(w[o:o + int(np.prod(s))].reshape(s).copy()) for k, (o, s) in offs.items() if k != "_total"}
    rng = np.random.default_rng(9)
    for v in [int(x) for x in np.nonzero(topo.degrees > 0)[0][::3]]:
        deg = int(topo.degrees[v])

        def lin(W, b):
            m = torch.nn.Linear(W.shape[0], W.shape[1])
            with torch.no_grad():
                m.weight.copy_(W.T)
                m.bias.copy_(b)
            return m
        one_hot = torch.nn.Sequential(lin(P["W1"][v][:topo.n_overlay], P["b1"][v]), torch.nn.ELU())
        buffers = torch.nn.Sequential(torch.nn.LayerNorm(deg, eps=1e-3, elementwise_affine=False),
                                      lin(P["Wb"][v][:deg], P["bb"][v]), torch.nn.ELU())
        layers = [lin(P["W2"][v], P["b2"][v]), torch.nn.ELU()]
        if NH == 2:
            layers += [lin(P["W3"][v], P["b3"][v]), torch.nn.ELU()]
        layers += [lin(P["W4"][v][:, :deg], P["b4"][v][:deg]), torch.nn.ELU()]
        trunk = torch.nn.Sequential(*layers)
        obs = LQ.random_obs(topo, v, 64, rng)
        with torch.no_grad():
            oh = torch.nn.functional.one_hot(torch.from_numpy(obs[:, 0].astype(np.int64)), topo.n_overlay).float()
            x = torch.from_numpy(obs[:, 1:1 + deg].astype(np.float32))
            want = trunk(torch.cat([one_hot(oh), buffers(x)], dim=1))
            got = net.q_values(torch.from_numpy(obs.astype(np.int32)), torch.full((64,), v))
        assert torch.all(torch.isinf(got[:, deg:])) and got.shape == (64, D)
        assert torch.allclose(got[:, :deg], want, rtol=1e-5, atol=1e-5), (kind, v)
        assert torch.equal(net.act(torch.from_numpy(obs.astype(np.int32)), torch.full((64,), v)).long(),
                           torch.argmin(got, dim=1))


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_near_ties_against_host_restatement(oracle_mod, kind):
    """The restatement's actions against torch fp32 under the project's near-tie rule."""
    from parity_util import check_near_ties
    from prisma_amd.records import ST_ENQUEUED, record_dtype
    topo = _topo("geant")
    net = StackedQNet(topo, kind, seed=6, device="cpu")
    w = net.pack().numpy()
    host = LQ.HostMLP(oracle_mod, topo, kind)
    rng = np.random.default_rng(10)
    nodes = np.nonzero(topo.degrees > 0)[0]
    recs = np.zeros(40 * len(nodes), dtype=record_dtype(topo.obs_width))
    for i, v in enumerate(nodes):
        sl = slice(40 * i, 40 * i + 40)
        recs["obs"][sl] = LQ.random_obs(topo, int(v), 40, rng)
        recs["node"][sl] = v
    recs["status"] = ST_ENQUEUED
    _, a = host.mlp_q_batch(w, recs["node"].astype(np.int32), recs["obs"].astype(np.uint32))
    recs["action"] = a
    n, dis, dq, gap = check_near_ties(net, w, host, recs, rel_tol=1e-5)
    assert n == len(recs) and dq < 1e-4, (n, dis, dq, gap)


def _net_hash(net):
    h = hashlib.sha256()
    for name, p in sorted(net.named_parameters()):
        h.update(name.encode() + b"\0" + p.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def test_existing_kinds_draw_the_same_tensors():
    """kind="buffer" and "routing": the same tensors for the same seed as before the family was
    added (hashes recorded from the commit before it)."""
    golden = json.load(open(GOLDEN))
    assert len(golden) == 8
    for key, want in golden.items():
        name, kind, seed = key.split("/")
        assert _net_hash(StackedQNet(_topo(name), kind, seed=int(seed), device="cpu")) == want, key


def test_agent_type_map():
    assert set(AGENT_MODEL_KINDS) <= set(AGENT_TYPES)
    assert [AGENT_MODEL_KINDS["dqn_" + k] for k in NEW_KINDS] == NEW_KINDS
    assert AGENT_MODEL_KINDS["dqn_buffer"] == "buffer" and AGENT_MODEL_KINDS["dqn_routing"] == "routing"
    assert all(k == "routing" or k in BUFFER_DIMS for k in AGENT_MODEL_KINDS.values())
    assert not {"dqn_buffer_ff", "dqn_buffer_fp", "dqn_buffer_with_throughputs"} & set(AGENT_MODEL_KINDS)
    assert {k: v[1] for k, v in engine.MODEL_POLICIES.items()} == BUFFER_DIMS
    with pytest.raises(ValueError):
        StackedQNet(_topo("abilene"), "buffer_ff", device="cpu")


# ---- 4. SavedModel bundles ----------------------------------------------------------------
@pytest.mark.parametrize("kind", NEW_KINDS)
def test_savedmodel_round_trip(tmp_path, kind):
    topo = _topo("abilene_on_geant")
    net = StackedQNet(topo, kind, seed=8, device="cpu")
    nodes = [int(u) for u in topo.overlay_nodes]
    sm.save_q_networks(net, str(tmp_path), nodes)
    layers = sm.dense_layers(sm.read_tensor_bundle(str(tmp_path / f"node{nodes[0]}" / "variables" / "variables")))
    # the two first-layer branches, NH hidden layers and the output: the Dense layers of models.py:39-227
    assert len(layers) == 3 + BUFFER_DIMS[kind][2] == len(buffer_layer_names(kind))
    back = sm.load_q_networks(str(tmp_path), topo, kind)
    assert sorted(back.loaded_nodes) == sorted(nodes)
    assert torch.equal(back.pack(), net.pack())
    # a bundle of another member of the family does not fit
    other = "buffer_lighter" if kind == "buffer_lite" else "buffer_lite"
    with pytest.raises(sm.BundleError):
        sm.load_q_networks(str(tmp_path), topo, other if BUFFER_DIMS[other] != BUFFER_DIMS[kind] else "buffer")


# ---- 5. parameter counts ----------------------------------------------------------------------
def test_nn_param_count_hand_counts():
    """Abilene: 11 overlay nodes; node 0 has 2 neighbours, so per model: one-hot Dense (11 B + B),
    buffers Dense (2 B + B), Dense(2B -> H), NH - 1 times Dense(H -> H), Dense(H -> 2)."""
    topo = _topo("abilene")
    u = int(np.nonzero(topo.degrees == 2)[0][0])
    assert topo.n_overlay == 11
    hand = {
        "buffer": (11 * 32 + 32) + (2 * 32 + 32) + (64 * 64 + 64) + (64 * 64 + 64) + (64 * 2 + 2),          # 8930
        "buffer_lite": (11 * 16 + 16) + (2 * 16 + 16) + (32 * 32 + 32) + (32 * 32 + 32) + (32 * 2 + 2),     # 2418
        "buffer_lighter": (11 * 16 + 16) + (2 * 16 + 16) + (32 * 32 + 32) + (32 * 2 + 2),                   # 1362
        "buffer_lighter_2": (11 * 8 + 8) + (2 * 8 + 8) + (16 * 16 + 16) + (16 * 2 + 2),                     # 426
        "buffer_lighter_3": (11 * 4 + 4) + (2 * 4 + 4) + (8 * 8 + 8) + (8 * 2 + 2),                         # 150
        "routing": (11 * 32 + 32) + (32 * 64 + 64) + (64 * 64 + 64) + (64 * 2 + 2),
    }
    assert [hand[k] for k in ("buffer", "buffer_lite", "buffer_lighter", "buffer_lighter_2", "buffer_lighter_3")] == \
        [8930, 2418, 1362, 426, 150]
    for kind, want in hand.items():
        assert nn_param_count(topo, u, kind) == want, kind
        if kind != "routing":
            net = StackedQNet(topo, kind, seed=0, device="cpu")
            used = sum(int((getattr(net, n)[u] != 0).sum()) for n, _ in net.named_parameters())
            assert used == want, kind                       # the draws fill exactly the model's parameters


# ---- 6. the trainer on the CPU ------------------------------------------------------------
def test_trainer_step_on_cpu():
    topo = _topo("abilene")
    tr = QRoutingTrainer(topo, kind="buffer_lighter", device="cpu", batch_size=16, buffer_size=256, seed=1)
    assert tr.kind == "buffer_lighter" and tr.q.dims == (16, 32, 1)
    assert tr.nn_size[0] == nn_param_count(topo, 0, "buffer_lighter") * 32
    rng = np.random.default_rng(3)
    n = 400
    node = rng.choice(np.nonzero(topo.degrees > 0)[0], n)
    obs = np.zeros((n, topo.obs_width), dtype=np.int32)
    nxt = np.zeros_like(obs)
    for i, v in enumerate(node):
        obs[i] = LQ.random_obs(topo, int(v), 1, rng)[0]
        nxt[i] = LQ.random_obs(topo, int(v), 1, rng)[0]
    act = np.array([rng.integers(0, topo.degrees[v]) for v in node], dtype=np.int32)
    tr.observe({"obs": torch.from_numpy(obs), "action": torch.from_numpy(act),
                "reward": torch.from_numpy(rng.uniform(0.001, 0.05, n)), "next_obs": torch.from_numpy(nxt),
                "done": torch.from_numpy(rng.random(n) < 0.2), "node": torch.from_numpy(node.astype(np.int32)),
                "replica": torch.zeros(n, dtype=torch.int32), "uid": torch.arange(n, dtype=torch.int64),
                "hop": torch.ones(n, dtype=torch.bool), "t_ns": torch.zeros(n, dtype=torch.int64),
                "episode": torch.zeros(n, dtype=torch.int64)})
    before = tr.q.pack().clone()
    per = tr.train_step()
    assert per is not None and bool(torch.isfinite(per[~torch.isnan(per)]).all()) and bool((~torch.isnan(per)).any())
    after = tr.q.pack()
    assert after.numel() == buffer_floats("buffer_lighter", topo.n_nodes, topo.max_deg)
    assert not torch.equal(before, after)


# ---- 7. the C-ABI without a device -----------------------------------------------------------
def test_new_policy_ids_with_null_env():
    lib = engine.load_library()
    assert (engine.PRISMA_POLICY_DQN_LITE, engine.PRISMA_POLICY_DQN_LIGHTER, engine.PRISMA_POLICY_DQN_LIGHTER_2,
            engine.PRISMA_POLICY_DQN_LIGHTER_3) == (3, 4, 5, 6)
    hdr = open(os.path.join(os.path.dirname(engine.LIB_PATH), "..", "include", "prisma.h")).read()
    for name, val in (("LITE", 3), ("LIGHTER", 4), ("LIGHTER_2", 5), ("LIGHTER_3", 6)):
        assert f"#define PRISMA_POLICY_DQN_{name} " in hdr.replace("  ", " ").replace("  ", " ") and \
            engine.MODEL_POLICIES["buffer_" + name.lower()][0] == val
    buf = (C.c_float * 4)()
    for pid in (3, 4, 5, 6):
        assert lib.prisma_run(None, pid, buf, 10, None) == -5                  # PRISMA_ERR_ARG
        assert lib.prisma_run_explore(None, pid, buf, 10, buf, None) == -5
    assert lib.prisma_abi_version() == 10
