"""ctypes binding of libprisma_amd.so (include/prisma.h) on torch HIP memory.

The library is the product: every simulation step runs in its gfx950
kernels.  There is no CPU fallback — if the shared library is missing or no
gfx950 device is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import buildid
from .records import COUNTERS_DTYPE, record_dtype
from .topology import Topology

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libprisma_amd.so")

ABI_VERSION = 10
PRISMA_POLICY_TABLE = 1
PRISMA_POLICY_DQN_BUFFER = 2
PRISMA_POLICY_DQN_LITE, PRISMA_POLICY_DQN_LIGHTER, PRISMA_POLICY_DQN_LIGHTER_2, PRISMA_POLICY_DQN_LIGHTER_3 = 3, 4, 5, 6
PRISMA_ENGINE_AUTO, PRISMA_ENGINE_REGISTER, PRISMA_ENGINE_MEMORY = 0, 1, 2

# run(..., model=): the kind of a packed fp32 policy (StackedQNet kinds) -> (policy id, (B, H, NH)),
# the widths of include/prisma.h's table (restated here: this module imports no torch)
MODEL_POLICIES = {
    "buffer": (PRISMA_POLICY_DQN_BUFFER, (32, 64, 2)),
    "buffer_lite": (PRISMA_POLICY_DQN_LITE, (16, 32, 2)),
    "buffer_lighter": (PRISMA_POLICY_DQN_LIGHTER, (16, 32, 1)),
    "buffer_lighter_2": (PRISMA_POLICY_DQN_LIGHTER_2, (8, 16, 1)),
    "buffer_lighter_3": (PRISMA_POLICY_DQN_LIGHTER_3, (4, 8, 1)),
}


def dqn_buffer_floats(n: int, d: int) -> int:
    """Length of the packed DQN-buffer weights (include/prisma.h PRISMA_POLICY_DQN_BUFFER)."""
    return n * n * 32 + n * 32 + n * d * 32 + n * 32 + 2 * (n * 64 * 64 + n * 64) + n * 64 * d + n * d


def model_floats(model: str, n: int, d: int) -> int:
    """Length of the packed weights of a DQN-buffer family kind (StackedQNet(kind=model).pack());
    dqn_buffer_floats for "buffer"."""
    b, h, nh = MODEL_POLICIES[model][1]
    return n * (n * b + b + d * b + b + 2 * b * h + h + (nh - 1) * (h * h + h) + h * d + d)


class PrismaError(RuntimeError):
    pass


class _Topo(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32), ("n_links", C.c_int32), ("n_flows", C.c_int32), ("max_deg", C.c_int32),
        ("row_ptr", C.c_void_p), ("link_dst", C.c_void_p), ("link_rev", C.c_void_p),
        ("flow_src", C.c_void_p), ("flow_dst", C.c_void_p), ("flow_rate_bps", C.c_void_p),
        ("n_overlay", C.c_int32), ("overlay_nodes", C.c_void_p), ("overlay_adj", C.c_void_p),
    ]


class _Params(C.Structure):
    _fields_ = [
        ("link_bps", C.c_uint64), ("link_delay_ns", C.c_int64), ("max_buffer_bytes", C.c_uint32),
        ("packet_size", C.c_uint32), ("sim_time_s", C.c_double), ("ping_interval_s", C.c_float),
        ("ma_size", C.c_uint32), ("ping_as_obs", C.c_uint32), ("auto_reset", C.c_uint32),
        ("loss_penalty", C.c_double), ("seed", C.c_uint64), ("replica_base", C.c_uint32),
        ("log_capacity", C.c_uint32), ("notify_dest", C.c_uint32), ("train", C.c_uint32),
        ("engine", C.c_uint32), ("signaling_type", C.c_uint32), ("big_signaling", C.c_uint32),
        ("sync_step_s", C.c_float), ("big_signaling_bytes", C.c_uint32),
        ("rng_mode", C.c_uint32), ("rng_stream_offset", C.c_uint32),
    ]


# the defaults of config.engine_params (argument_parser.py:72-74, 86; bigSignalingSize 512)
_PARAM_DEFAULTS = dict(engine=0, signaling_type=0, big_signaling=0, sync_step_s=1.0, big_signaling_bytes=512,
                       rng_mode=0, rng_stream_offset=0)


class _LogView(C.Structure):
    _fields_ = [("records", C.c_void_p), ("record_bytes", C.c_uint32), ("log_capacity", C.c_uint32),
                ("obs_width", C.c_int32), ("n_replicas", C.c_int32)]


class _KernelInfo(C.Structure):
    _fields_ = [("engine", C.c_uint32), ("flow_slots", C.c_int32), ("link_slots", C.c_int32),
                ("tunnels", C.c_uint32), ("ctrl", C.c_uint32), ("relay_ip", C.c_uint32),
                ("relay_dec_bits", C.c_uint32)]


class _Replay(C.Structure):
    """prisma_replay_t: the per-node replay rings prisma_ingest_transitions writes."""
    _fields_ = [("obs", C.c_void_p), ("next_obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p),
                ("done", C.c_void_p), ("replica", C.c_void_p), ("next_idx", C.c_void_p), ("count", C.c_void_p),
                ("total", C.c_void_p), ("size", C.c_int64), ("n_nodes", C.c_int32), ("obs_width", C.c_int32)]


class _QNets(C.Structure):
    """prisma_qnets_t: the stored weight generations prisma_replay_targets evaluates."""
    _fields_ = [("weights", C.c_void_p), ("n_gen", C.c_int32), ("model", C.c_int32), ("gen_of", C.c_void_p)]


# replay_targets(..., model=): MODEL_POLICIES' kinds and the routing model (include/prisma.h)
PRISMA_QMODEL_ROUTING = 0
TARGET_MODELS = dict({"routing": PRISMA_QMODEL_ROUTING}, **{k: v[0] for k, v in MODEL_POLICIES.items()})


def routing_floats(n: int, d: int) -> int:
    """Length of the packed DQ-routing weights (include/prisma.h PRISMA_QMODEL_ROUTING)."""
    return n * (n * 32 + 32 + 32 * 64 + 64 + 64 * 64 + 64 + 64 * d + d)


class _Plan(C.Structure):
    _fields_ = [("state_bytes", C.c_uint32), ("lds_bytes", C.c_uint32), ("lds_state_bytes", C.c_uint32),
                ("ring_entries", C.c_uint32), ("record_bytes", C.c_uint32), ("obs_width", C.c_int32),
                ("flow_slots", C.c_int32), ("link_slots", C.c_int32), ("engine", C.c_uint32)]


class _Scenarios(C.Structure):
    """prisma_scenarios_t: the flow rates of S scenarios and each replica's scenario (host arrays)."""
    _fields_ = [("n_scenarios", C.c_int32), ("flow_rate_bps", C.c_void_p), ("scenario_of", C.c_void_p)]


class _ScenarioPlan(C.Structure):
    _fields_ = [("topo_bytes", C.c_uint64), ("image_bytes", C.c_uint32), ("n_scenarios", C.c_int32)]


EXPORTS = [
    "prisma_abi_version", "prisma_last_error", "prisma_build_id", "prisma_create", "prisma_reset", "prisma_step", "prisma_run",
    "prisma_run_explore", "prisma_action_history_layout", "prisma_run_explore_smart", "prisma_run_stochastic",
    "prisma_read_counters", "prisma_counters_device", "prisma_log_view", "prisma_copy_log",
    "prisma_copy_counters", "prisma_gather_records", "prisma_state_bytes", "prisma_plan", "prisma_destroy",
    "prisma_compact_pending", "prisma_expand_actions", "prisma_kernel_info", "prisma_ingest_transitions",
    "prisma_replay_targets", "prisma_create_scenarios", "prisma_plan_scenarios", "prisma_plan_scenario_images",
    "prisma_scenario_info", "prisma_scenario_stats",
]

_lib = None


def load_library(path: str = None):
    """Load libprisma_amd.so and declare its C-ABI (raises if absent).

    PRISMA_LIB overrides the path (diagnostic builds, e.g. scripts/build_variant.sh).  The default
    library must carry the build id of the sources beside it (prisma_amd/buildid.py): a stale
    binary raises instead of running."""
    global _lib
    if _lib is not None:
        return _lib
    override = path or os.environ.get("PRISMA_LIB")
    path = override or LIB_PATH
    if not os.path.exists(path):
        raise PrismaError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    # torch first: its wheel carries its own HIP runtime, and the library works on torch's device
    # memory, so it must bind to that runtime.  Loaded before torch it would pull in the system's
    # libamdhip64 as a second runtime in the process, which then finds no device (build() followed
    # by smoke() in one process).
    import torch  # noqa: F401
    L = C.CDLL(path)
    L.prisma_abi_version.restype = C.c_int
    L.prisma_last_error.restype = C.c_char_p
    L.prisma_build_id.restype = C.c_char_p
    if not override and buildid.sources_present():
        want, got = buildid.source_hash(), L.prisma_build_id().decode()
        if got != want:
            raise PrismaError(f"{path} was built from other sources (build id {got}, sources {want}): "
                              f"rebuild with `python -c 'import __graft_entry__ as g; g.build()'`")
    L.prisma_create.restype = C.c_int
    L.prisma_create.argtypes = [C.POINTER(_Topo), C.POINTER(_Params), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.prisma_reset.restype = C.c_int
    L.prisma_reset.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.prisma_step.restype = C.c_int
    L.prisma_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.prisma_run.restype = C.c_int
    L.prisma_run.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.prisma_run_explore.restype = C.c_int
    L.prisma_run_explore.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.prisma_action_history_layout.restype = C.c_int
    L.prisma_action_history_layout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.prisma_run_explore_smart.restype = C.c_int
    L.prisma_run_explore_smart.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.c_void_p]
    L.prisma_run_stochastic.restype = C.c_int
    L.prisma_run_stochastic.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p]
    L.prisma_read_counters.restype = C.c_int
    L.prisma_read_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.prisma_counters_device.restype = C.c_int
    L.prisma_counters_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.prisma_log_view.restype = C.c_int
    L.prisma_log_view.argtypes = [C.c_void_p, C.POINTER(_LogView)]
    L.prisma_copy_log.restype = C.c_int
    L.prisma_copy_log.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.prisma_copy_counters.restype = C.c_int
    L.prisma_copy_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.prisma_gather_records.restype = C.c_int
    L.prisma_gather_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.prisma_compact_pending.restype = C.c_int
    L.prisma_compact_pending.argtypes = [C.c_void_p] + [C.c_void_p] * 7 + [C.c_void_p]
    L.prisma_expand_actions.restype = C.c_int
    L.prisma_expand_actions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p]
    L.prisma_ingest_transitions.restype = C.c_int
    L.prisma_ingest_transitions.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Replay), C.c_void_p]
    L.prisma_replay_targets.restype = C.c_int
    L.prisma_replay_targets.argtypes = [C.c_void_p, C.POINTER(_Replay), C.c_void_p, C.c_int32, C.POINTER(_QNets),
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.prisma_kernel_info.restype = C.c_int
    L.prisma_kernel_info.argtypes = [C.c_void_p, C.POINTER(_KernelInfo)]
    L.prisma_state_bytes.restype = C.c_int
    L.prisma_state_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.prisma_plan.restype = C.c_int
    L.prisma_plan.argtypes = [C.POINTER(_Topo), C.POINTER(_Params), C.POINTER(_Plan)]
    L.prisma_create_scenarios.restype = C.c_int
    L.prisma_create_scenarios.argtypes = [C.POINTER(_Topo), C.POINTER(_Params), C.POINTER(_Scenarios), C.c_int32,
                                          C.c_int32, C.POINTER(C.c_void_p)]
    L.prisma_plan_scenarios.restype = C.c_int
    L.prisma_plan_scenarios.argtypes = [C.POINTER(_Topo), C.POINTER(_Params), C.POINTER(_Scenarios), C.c_int32,
                                        C.POINTER(_Plan)]
    L.prisma_plan_scenario_images.restype = C.c_int
    L.prisma_plan_scenario_images.argtypes = [C.POINTER(_Topo), C.POINTER(_Params), C.POINTER(_Scenarios), C.c_int32,
                                              C.POINTER(_ScenarioPlan)]
    L.prisma_scenario_info.restype = C.c_int
    L.prisma_scenario_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    L.prisma_scenario_stats.restype = C.c_int
    L.prisma_scenario_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.prisma_destroy.restype = None
    L.prisma_destroy.argtypes = [C.c_void_p]
    if L.prisma_abi_version() != ABI_VERSION:
        raise PrismaError("libprisma_amd ABI version mismatch")
    _lib = L
    return L


def build_id() -> str:
    """Build id of the loaded library (prisma_build_id())."""
    return load_library().prisma_build_id().decode()


def _check(rc: int):
    if rc != 0:
        msg = _lib.prisma_last_error().decode(errors="replace")
        raise PrismaError(f"prisma error {rc}: {msg}")


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


def _topo_struct(topo: Topology):
    keep = [np.ascontiguousarray(topo.row_ptr, dtype=np.int32),
            np.ascontiguousarray(topo.link_dst, dtype=np.int32),
            np.ascontiguousarray(topo.link_rev, dtype=np.int32),
            np.ascontiguousarray(topo.flow_src, dtype=np.int32),
            np.ascontiguousarray(topo.flow_dst, dtype=np.int32),
            np.ascontiguousarray(topo.flow_rate_bps, dtype=np.uint64)]
    t = _Topo(topo.n_nodes, topo.n_links, topo.n_flows, topo.max_deg, *[a.ctypes.data for a in keep])
    if not topo.identity:                      # identity overlays pass n_overlay = 0
        ov = [np.ascontiguousarray(topo.overlay_nodes, dtype=np.int32),
              np.ascontiguousarray(topo.overlay_adj, dtype=np.int32)]
        keep += ov
        t.n_overlay = topo.n_overlay
        t.overlay_nodes = ov[0].ctypes.data
        t.overlay_adj = ov[1].ctypes.data
    return t, keep


def _params_struct(params: dict) -> _Params:
    """prisma_params_t from an engine_params() dict (engine defaults to auto)."""
    return _Params(**{k: params.get(k, _PARAM_DEFAULTS[k]) if k in _PARAM_DEFAULTS else params[k]
                      for k, _ in _Params._fields_})


def _scenarios_struct(scenarios, scenario_of, n_replicas: int, n_flows: int, replica_base: int = 0):
    """prisma_scenarios_t from a scenarios.ScenarioSet (or a uint64 [S, F] array of rates) and an
    int32 [n_replicas] assignment (default: ScenarioSet.assign's round robin by GLOBAL replica id,
    (replica_base + r) mod S, so a shard agrees with the unsharded env)."""
    rates = np.ascontiguousarray(getattr(scenarios, "rates", scenarios), dtype=np.uint64)
    if rates.ndim != 2 or rates.shape[1] != n_flows:
        raise PrismaError(f"scenarios: rates must be a uint64 [S, {n_flows}] array")
    if scenario_of is None:
        scenario_of = (int(replica_base) + np.arange(n_replicas)) % max(rates.shape[0], 1)
    sc = np.ascontiguousarray(scenario_of, dtype=np.int32)
    if sc.shape != (n_replicas,):
        raise PrismaError(f"scenario_of must have n_replicas = {n_replicas} entries")
    return _Scenarios(rates.shape[0], rates.ctypes.data, sc.ctypes.data), [rates, sc]


def plan(topo: Topology, params: dict, scenarios=None, scenario_of=None, n_replicas: int = 1) -> dict:
    """prisma_plan: validate a scenario and report its per-replica footprint (no device needed).
    scenarios (a scenarios.ScenarioSet or uint64 [S, F] rates; scenario_of int32 [n_replicas]):
    prisma_plan_scenarios, with the set's validation, plus topo_bytes -- the device bytes of all
    scenarios' topology images --, image_bytes and n_scenarios (prisma_plan_scenario_images)."""
    L = load_library()
    t, keep = _topo_struct(topo)
    p = _params_struct(params)
    out = _Plan()
    if scenarios is None:
        _check(L.prisma_plan(C.byref(t), C.byref(p), C.byref(out)))
        return {k: int(getattr(out, k)) for k, _ in _Plan._fields_}
    sc, keep2 = _scenarios_struct(scenarios, scenario_of, int(n_replicas), topo.n_flows,
                                  params.get("replica_base", 0))
    _check(L.prisma_plan_scenarios(C.byref(t), C.byref(p), C.byref(sc), int(n_replicas), C.byref(out)))
    sp = _ScenarioPlan()
    _check(L.prisma_plan_scenario_images(C.byref(t), C.byref(p), C.byref(sc), int(n_replicas), C.byref(sp)))
    res = {k: int(getattr(out, k)) for k, _ in _Plan._fields_}
    res.update({k: int(getattr(sp, k)) for k, _ in _ScenarioPlan._fields_})
    return res


def step_kernel_names(ki: dict, pl: dict) -> dict:
    """Demangled names of the step-kernel instances an env launches, from prisma_kernel_info's
    and prisma_plan's answers (the library's own choice, prisma_create and run_fused, restated):
    `step` by prisma_step, `table` by prisma_run with a table, `mlp` by prisma_run with DQN-buffer
    weights.  Fused table runs have instances of their own (prisma_step_kernel_fused_t) on the
    register-resident engine where the env is an identity overlay without the ctrl paths and its
    table sits in LDS (the plan's LDS per replica then exceeds the state image's part); elsewhere
    `table` is `step`."""
    ctrl = "true" if ki["ctrl"] else "false"
    if ki["engine"] == PRISMA_ENGINE_MEMORY:
        step = f"prisma_mem_step_kernel<false, {ctrl}>"
        return {"step": step, "table": step, "mlp": f"prisma_mem_step_kernel<true, {ctrl}>"}
    fs, ls = ki["flow_slots"], ki["link_slots"]
    tun = "true" if ki["tunnels"] else "false"
    # template arguments: slots, in-kernel MLP, tunnels, --train/notify_dest paths (the
    # greedy instances; the sixth, EXPL, is true for the ones run(..., explore=) launches)
    step = f"prisma_step_kernel_t<{fs}, {ls}, false, {tun}, {ctrl}>"
    fused = not ki["ctrl"] and not ki["tunnels"] and pl["lds_bytes"] > pl["lds_state_bytes"]
    return {"step": step,
            "table": f"prisma_step_kernel_fused_t<{fs}, {ls}, false, false>" if fused else step,
            "mlp": f"prisma_step_kernel_t<{fs}, {ls}, true, {tun}, {ctrl}>"}


class PrismaEngine:
    """R replicas of one scenario on one MI355X (device memory owned by the library).

    scenarios (a scenarios.ScenarioSet, or uint64 [S, F] rates) with scenario_of (int32
    [n_replicas], each in [0, S); default round robin by global id, (replica_base + r) mod S): replica r reads the flow rates of scenario
    scenario_of[r] instead of topo's (prisma_create_scenarios); `topo` is then the set's structure,
    by convention scenario 0's topology."""

    def __init__(self, topo: Topology, params: dict, n_replicas: int, device: int = 0, scenarios=None,
                 scenario_of=None):
        import torch
        if not torch.cuda.is_available():
            raise PrismaError("PrismaEngine needs a HIP device (no CPU fallback)")
        L = load_library()
        self.topo = topo
        self.params = dict(params)
        self.R = int(n_replicas)
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        t, self._keep = _topo_struct(topo)
        p = _params_struct(params)
        h = C.c_void_p()
        if scenarios is None and scenario_of is not None:
            raise PrismaError("scenario_of needs scenarios")
        with torch.cuda.device(self.device):
            if scenarios is None:
                _check(L.prisma_create(C.byref(t), C.byref(p), self.R, self.device, C.byref(h)))
            else:
                sc, _keep = _scenarios_struct(scenarios, scenario_of, self.R, topo.n_flows,
                                              params.get("replica_base", 0))
                _check(L.prisma_create_scenarios(C.byref(t), C.byref(p), C.byref(sc), self.R, self.device,
                                                 C.byref(h)))
        self.h = h
        ns = C.c_int32()
        so = np.zeros(self.R, dtype=np.int32)
        _check(L.prisma_scenario_info(self.h, C.byref(ns), so.ctypes.data))
        self.n_scenarios = int(ns.value)
        self.scenario_of_host = so
        self.scenario_of = torch.from_numpy(so).to(self.torch_device)
        lv = _LogView()
        _check(L.prisma_log_view(self.h, C.byref(lv)))
        self.W = int(lv.obs_width)
        self.rec_bytes = int(lv.record_bytes)
        self.log_capacity = int(lv.log_capacity)
        self.rec_dtype = record_dtype(self.W)
        sb, lb = C.c_uint32(), C.c_uint32()
        _check(L.prisma_state_bytes(self.h, C.byref(sb), C.byref(lb)))
        self.state_bytes, self.lds_bytes = int(sb.value), int(lb.value)
        # step-kernel instances the library picked (prisma_kernel_info: the choice prisma_create
        # made, reported by the library; the demangled names are for profiles)
        ki = self.kernel_info()
        self.engine_kind = ki["engine"]
        # kernel_name: what run() with a table launches (bench.py's roofline.kernel, the
        # profiles' filter); kernel_name_step: what step() launches; kernel_name_mlp: run() with
        # DQN-buffer weights
        names = step_kernel_names(ki, plan(topo, params))
        self.kernel_name = names["table"]
        self.kernel_name_step = names["step"]
        self.kernel_name_mlp = names["mlp"]
        self.obs = torch.zeros((self.R, self.W), dtype=torch.int32, device=self.torch_device)
        self.mask = torch.zeros(self.R, dtype=torch.uint8, device=self.torch_device)
        self.node = torch.zeros(self.R, dtype=torch.int32, device=self.torch_device)

    def kernel_info(self) -> dict:
        """prisma_kernel_info: the step-kernel instances this engine launches (engine, template
        slots, tunnels, ctrl paths, relay entries with LDS FIFO windows, relay index bits)."""
        ki = _KernelInfo()
        _check(_lib.prisma_kernel_info(self.h, C.byref(ki)))
        return {k: int(getattr(ki, k)) for k, _ in _KernelInfo._fields_}

    # -- lifecycle --------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            _lib.prisma_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, episode: int = 0, stream=None):
        _check(_lib.prisma_reset(self.h, int(episode), _stream_handle(stream)))

    # -- hot path ---------------------------------------------------------
    def step(self, actions=None, stream=None):
        """Apply actions [R] (int32 on device) to pending decisions, advance to the next ones."""
        a = 0
        if actions is not None:
            if actions.dtype != self.obs.dtype or actions.numel() != self.R or not actions.is_cuda:
                raise PrismaError("actions must be a device int32 tensor of n_replicas elements")
            a = actions.contiguous().data_ptr()
        _check(_lib.prisma_step(self.h, a or None, self.obs.data_ptr(), self.mask.data_ptr(), self.node.data_ptr(),
                                _stream_handle(stream)))
        return self.obs, self.mask, self.node

    def compact_pending(self, stream=None):
        """The pending replicas of the last step() as a dense batch (prisma_compact_pending):
        (ids int32 [n], obs int32 [n, W], node int32 [n]) for a policy that evaluates only the
        notified replicas (ns3env.py:417-423). One host read of the count. The tensors are views
        of buffers the next call reuses: valid until then (clone them to keep them longer)."""
        import torch
        if not hasattr(self, "_cids"):
            self._cids = torch.empty(self.R, dtype=torch.int32, device=self.torch_device)
            self._cobs = torch.empty((self.R, self.W), dtype=torch.int32, device=self.torch_device)
            self._cnode = torch.empty(self.R, dtype=torch.int32, device=self.torch_device)
            self._ccount = torch.zeros(1, dtype=torch.int32, device=self.torch_device)
        _check(_lib.prisma_compact_pending(self.h, self.mask.data_ptr(), self.obs.data_ptr(), self.node.data_ptr(),
                                           self._cids.data_ptr(), self._cobs.data_ptr(), self._cnode.data_ptr(),
                                           self._ccount.data_ptr(), _stream_handle(stream)))
        n = int(self._ccount.item())
        self._cn = n
        return self._cids[:n], self._cobs[:n], self._cnode[:n]

    def expand_actions(self, ids, packed_actions, fill: int = 0, stream=None):
        """Actions of a compacted batch back to one per replica (prisma_expand_actions), ready
        for step(); replicas without a pending decision get `fill`."""
        import torch
        out = torch.empty(self.R, dtype=torch.int32, device=self.torch_device)
        n = int(ids.numel())
        # the count on the device without a host-to-device copy (a pageable copy synchronises the
        # stream): compact_pending's own count when ids is its batch, else a device-side fill
        if (hasattr(self, "_ccount") and n and n == self._cn and ids.data_ptr() == self._cids.data_ptr()
                and ids.dtype == torch.int32):
            cnt = self._ccount
        else:
            # a fresh count per call, filled on the launch's own stream: a reused buffer could be
            # refilled while an earlier expand still reads it, or read before a fill on another stream
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                cnt = torch.full((1,), n, dtype=torch.int32, device=self.torch_device)
        # (an empty batch still passes valid device pointers: the count says there is nothing)
        ids_c = ids.to(torch.int32).contiguous() if n else torch.zeros(1, dtype=torch.int32, device=self.torch_device)
        act = (packed_actions.to(torch.int32).contiguous() if n
               else torch.zeros(1, dtype=torch.int32, device=self.torch_device))
        _check(_lib.prisma_expand_actions(self.h, ids_c.data_ptr(), cnt.data_ptr(), act.data_ptr(), int(fill),
                                          out.data_ptr(), _stream_handle(stream)))
        return out

    def action_history_layout(self):
        """prisma_action_history_layout: (row int32 [n_nodes + 1], T) -- node v's actions are
        columns row[v] .. row[v + 1] of an action history, by underlay id (empty for a node outside
        the overlay); T = row[n_nodes] is the sum of the overlay degrees."""
        row = np.zeros(self.topo.n_nodes + 1, dtype=np.int32)
        total = C.c_int32()
        _check(_lib.prisma_action_history_layout(self.h, row.ctypes.data, C.byref(total)))
        return row, int(total.value)

    def new_action_history(self, fill: int = 1):
        """A device int32 [n_replicas, T] action history for run(..., action_history=), every count
        `fill` (the reference starts at ones).  The kernels read its bits as uint32."""
        import torch
        _, total = self.action_history_layout()
        return torch.full((self.R, total), int(fill), dtype=torch.int32, device=self.torch_device)

    def run(self, policy, max_hops: int, stream=None, explore=None, model: str = "buffer", action_history=None):
        """Fused in-kernel policy: every replica executes up to max_hops hops.

        policy: a device uint8 [N, N] action table (SP, DQ-routing argmin), or the device fp32
        packed weights of StackedQNet(kind=model).pack().

        model: the kind of a packed fp32 policy, "buffer" (the default) or one of the reduced
        DQN-buffer models "buffer_lite", "buffer_lighter", "buffer_lighter_2", "buffer_lighter_3"
        (MODEL_POLICIES; the register-resident engine without the ctrl paths only).  The policy must
        have model_floats(model, n_nodes, max_deg) elements.  Ignored for a table.

        explore: None (greedy), or the epsilons of an epsilon-greedy rollout (prisma_run_explore;
        prisma_amd/explore.py restates its draw rule): a scalar, or a float tensor / array
        [n_nodes] indexed by underlay node id. Constant over the launch; a device tensor is
        converted on the device without a host sync.

        action_history: None, or with `explore` the history-weighted ("smart") exploration of
        prisma_run_explore_smart: a contiguous int32 [n_replicas, T] tensor on this engine's device
        (new_action_history), which the launch reads and updates in place -- an exploring decision
        picks by its node's counts instead of uniformly, and every data decision counts its action
        (explore.py restates the rule).  The caller owns it and carries it between launches."""
        import torch
        n, d = self.topo.n_nodes, self.topo.max_deg
        if action_history is not None:
            if explore is None:
                raise PrismaError("prisma_run_explore_smart: action_history needs explore (the epsilons)")
            total = self.action_history_layout()[1]
            if (not torch.is_tensor(action_history) or action_history.device != self.torch_device
                    or action_history.dtype != torch.int32 or tuple(action_history.shape) != (self.R, total)
                    or not action_history.is_contiguous()):
                raise PrismaError(f"prisma_run_explore_smart: action_history must be a contiguous int32 "
                                  f"[{self.R}, {total}] tensor on {self.torch_device} (new_action_history)")
        if not policy.is_cuda:
            raise PrismaError("policy data must live on the device")
        if model not in MODEL_POLICIES:
            raise PrismaError(f"model must be one of {', '.join(MODEL_POLICIES)}")
        if policy.dtype == torch.uint8 and tuple(policy.shape) == (n, n):
            kind = PRISMA_POLICY_TABLE
        elif policy.dtype == torch.float32 and policy.dim() == 1 and policy.numel() == model_floats(model, n, d):
            kind = MODEL_POLICIES[model][0]
        elif model != "buffer":
            raise PrismaError(f"policy must be a uint8 [n_nodes, n_nodes] table or the packed fp32 weights of model "
                              f"{model!r}: {model_floats(model, n, d)} elements")
        else:
            raise PrismaError("policy must be a uint8 [n_nodes, n_nodes] table or packed fp32 DQN-buffer weights")
        self._policy_keep = policy.contiguous()
        if explore is None:
            _check(_lib.prisma_run(self.h, kind, self._policy_keep.data_ptr(), int(max_hops), _stream_handle(stream)))
            return
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            self._thr_keep = self._explore_thr(explore)
        if action_history is not None:
            _check(_lib.prisma_run_explore_smart(self.h, kind, self._policy_keep.data_ptr(), int(max_hops),
                                                 self._thr_keep.data_ptr(), action_history.data_ptr(),
                                                 action_history.numel(), _stream_handle(stream)))
            return
        _check(_lib.prisma_run_explore(self.h, kind, self._policy_keep.data_ptr(), int(max_hops),
                                       self._thr_keep.data_ptr(), _stream_handle(stream)))

    def run_stochastic(self, tab, max_hops: int, stream=None):
        """Fused stochastic multipath routing, the reference's "opt" agent (prisma_run_stochastic;
        prisma_amd/optrouting.py restates its rule): every replica executes up to max_hops hops.

        tab: a contiguous int32 or uint32 [n_overlay, n_overlay, T] tensor on this engine's device,
        the table optrouting.pack_routing builds (T = action_history_layout()[1]); the kernels read
        its bits as uint32.  It is read during the launch: keep it unchanged until the launch is done
        (the engine holds a reference).  The register-resident engine without the ctrl paths only."""
        import torch
        no, total = self.topo.n_overlay, self.action_history_layout()[1]
        if (not torch.is_tensor(tab) or tab.device != self.torch_device
                or tab.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                or tuple(tab.shape) != (no, no, total) or not tab.is_contiguous()):
            raise PrismaError(f"prisma_run_stochastic: tab must be a contiguous int32 / uint32 [{no}, {no}, {total}] "
                              f"tensor on {self.torch_device} (optrouting.pack_routing)")
        self._policy_keep = tab
        _check(_lib.prisma_run_stochastic(self.h, tab.data_ptr(), tab.numel(), int(max_hops), _stream_handle(stream)))

    def stochastic_table(self, routing):
        """optrouting.pack_routing(topo, routing) as a device tensor for run_stochastic (int32 storage
        of the uint32 words)."""
        import torch
        from . import optrouting
        tab = optrouting.pack_routing(self.topo, routing)
        return torch.from_numpy(tab.view(np.int32)).to(self.torch_device)

    def _explore_thr(self, explore):
        """Epsilons -> the device thresholds of prisma_run_explore (explore.thresholds' rule:
        floor(eps * 2^24 + 0.5) clamped to [0, 2^24]), in double precision as on the host.  A fresh
        tensor per call: an earlier launch may still read the last one."""
        import torch
        n = self.topo.n_nodes
        if torch.is_tensor(explore):
            eps = explore.to(device=self.torch_device, dtype=torch.float64)
        else:
            eps = torch.from_numpy(np.asarray(explore, dtype=np.float64)).to(self.torch_device, non_blocking=True)
        if eps.dim() == 0:
            eps = eps.expand(n)
        if eps.dim() != 1 or eps.numel() != n:
            raise PrismaError("explore must be a scalar or one epsilon per node [n_nodes]")
        thr = torch.floor(torch.nan_to_num(eps, nan=0.0) * float(1 << 24) + 0.5).clamp(0.0, float(1 << 24))
        # (int32 storage: values <= 2^24, read as uint32 by the kernel)
        return thr.to(torch.int32).contiguous()

    # -- outputs ----------------------------------------------------------
    def counters(self, stream=None) -> np.ndarray:
        out = np.zeros(self.R, dtype=COUNTERS_DTYPE)
        _check(_lib.prisma_read_counters(self.h, out.ctypes.data, _stream_handle(stream)))
        return out

    def scenario_stats(self, stream=None):
        """prisma_scenario_stats: per-scenario sums of the replicas' counters, one launch on torch's
        current stream (or `stream`), no host read.  A device uint8 tensor [n_scenarios, 248]:
        rows of scenarios.STATS_DTYPE (``.cpu().numpy().view(STATS_DTYPE)``); the f64 sums are in
        the fixed order scenarios.stats_sum restates."""
        import torch
        from .scenarios import STATS_DTYPE
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            buf = torch.empty((self.n_scenarios, STATS_DTYPE.itemsize), dtype=torch.uint8, device=self.torch_device)
        _check(_lib.prisma_scenario_stats(self.h, buf.data_ptr(), _stream_handle(stream)))
        return buf

    def counters_tensor(self, stream=None):
        """Device copy of the counters as a torch uint8 tensor [R, 144] (for device-side use / collectives)."""
        import torch
        buf = torch.empty((self.R, COUNTERS_DTYPE.itemsize), dtype=torch.uint8, device=self.torch_device)
        _check(_lib.prisma_copy_counters(self.h, buf.data_ptr(), _stream_handle(stream)))
        return buf

    def gather_records(self, replica, dec, stream=None):
        """Device gather of records -> torch uint8 [n, rec_bytes] (replica int32, dec int32/uint32 on device)."""
        import torch
        n = int(replica.numel())
        out = torch.empty((max(n, 1), self.rec_bytes), dtype=torch.uint8, device=self.torch_device)
        if n:
            rep = replica.to(torch.int32).contiguous()
            d = dec.to(torch.int32).contiguous()
            _check(_lib.prisma_gather_records(self.h, rep.data_ptr(), d.data_ptr(), n, out.data_ptr(),
                                              _stream_handle(stream)))
        return out[:n]

    def ingest_transitions(self, consumed, buffers, stream=None):
        """prisma_ingest_transitions: the transitions completed since `consumed` (device int64
        [n_replicas], each replica's first record not yet ingested; advanced in place) from the
        decision log straight into `buffers` (a non-prioritized trainer.ReplayBuffers on this
        engine's device), exactly as ``buffers.add(env.transitions())`` would -- the order rule is
        in include/prisma.h.  Three launches on torch's current stream (or `stream`), no host read."""
        import torch
        if getattr(buffers, "prioritized", False):
            raise ValueError("prisma_ingest_transitions fills a non-prioritized ReplayBuffers (priorities are "
                             "kept by ReplayBuffers.add)")
        want = [("consumed", consumed, torch.int64, (self.R,))]
        n, size, w = int(buffers.N), int(buffers.size), int(buffers.W)
        for name, dt, shape in (("obs", torch.int32, (n, size, w)), ("next_obs", torch.int32, (n, size, w)),
                                ("action", torch.int64, (n, size)), ("reward", torch.float32, (n, size)),
                                ("done", torch.bool, (n, size)), ("replica", torch.int64, (n, size)),
                                ("next_idx", torch.int64, (n,)), ("count", torch.int64, (n,)),
                                ("total", torch.int64, (n,))):
            want.append((name, getattr(buffers, name), dt, shape))
        for name, t, dt, shape in want:
            if (not torch.is_tensor(t) or t.device != self.torch_device or t.dtype != dt or tuple(t.shape) != shape
                    or not t.is_contiguous()):
                raise ValueError(f"prisma_ingest_transitions: {name} must be a contiguous {dt} tensor of shape "
                                 f"{shape} on {self.torch_device}")
        rings = _Replay(*[getattr(buffers, k).data_ptr() for k in ("obs", "next_obs", "action", "reward", "done",
                                                                   "replica", "next_idx", "count", "total")],
                        size, n, w)
        _check(_lib.prisma_ingest_transitions(self.h, consumed.data_ptr(), C.byref(rings), _stream_handle(stream)))

    def replay_targets(self, buffers, idx, weights, model: str, gamma: float = 1.0, gen_of=None, stream=None) -> dict:
        """prisma_replay_targets: the batch ``buffers.sample_full(batch, idx=idx)`` selects and its
        bootstrap targets against every stored weight generation, in one launch on torch's current
        stream (or `stream`) with no host read -- the rule is in include/prisma.h.

        idx: device int64 [N, batch] ring slots.  weights: a list of packed device float32 tensors,
        one per generation (StackedQNet.pack_targets()); model: "routing" or a MODEL_POLICIES kind.
        gen_of: device int32 [n_replicas, T] (action_history_layout), the generation each (replica,
        node, action) reads, or None for generation 0 everywhere.  Returns device tensors with row
        i = u * batch + b: obs int32 [N * batch, W], action int64, target float32 and status uint8
        (0 evaluated, 1 done, 2 not evaluable).  The pointer array lives on the device and is
        rebuilt only when the list's addresses change; the tensors are kept alive until the next call."""
        import torch
        if model not in TARGET_MODELS:
            raise PrismaError(f"model must be one of {', '.join(TARGET_MODELS)}")
        n, size, w = int(buffers.N), int(buffers.size), int(buffers.W)
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[0] != n or idx.shape[1] < 1:
            raise ValueError(f"prisma_replay_targets: idx must be an int64 tensor of shape ({n}, batch >= 1)")
        batch = int(idx.shape[1])
        want = [("idx", idx, torch.int64, (n, batch))]
        for name, dt, shape in (("obs", torch.int32, (n, size, w)), ("next_obs", torch.int32, (n, size, w)),
                                ("action", torch.int64, (n, size)), ("reward", torch.float32, (n, size)),
                                ("done", torch.bool, (n, size)), ("replica", torch.int64, (n, size))):
            want.append((name, getattr(buffers, name), dt, shape))
        weights = list(weights)
        if not weights:
            raise ValueError("prisma_replay_targets: weights must hold at least one packed generation")
        d = self.topo.max_deg
        floats = routing_floats(n, d) if model == "routing" else model_floats(model, n, d)
        for g, t in enumerate(weights):
            want.append((f"weights[{g}]", t, torch.float32, (floats,)))
        if gen_of is not None:
            want.append(("gen_of", gen_of, torch.int32, (self.R, int(self.action_history_layout()[1]))))
        for name, t, dt, shape in want:
            if (not torch.is_tensor(t) or t.device != self.torch_device or t.dtype != dt or tuple(t.shape) != shape
                    or not t.is_contiguous()):
                raise ValueError(f"prisma_replay_targets: {name} must be a contiguous {dt} tensor of shape "
                                 f"{shape} on {self.torch_device}")
        ptrs = tuple(t.data_ptr() for t in weights)
        if getattr(self, "_targets_ptrs", None) != ptrs:
            self._targets_ptr_dev = torch.tensor(ptrs, dtype=torch.int64, device=self.torch_device)
            self._targets_ptrs = ptrs
        self._targets_keep = (weights, gen_of)
        rows = n * batch
        out = {"obs": torch.empty((rows, w), dtype=torch.int32, device=self.torch_device),
               "action": torch.empty(rows, dtype=torch.int64, device=self.torch_device),
               "target": torch.empty(rows, dtype=torch.float32, device=self.torch_device),
               "status": torch.empty(rows, dtype=torch.uint8, device=self.torch_device)}
        rings = _Replay(*[getattr(buffers, k).data_ptr() for k in ("obs", "next_obs", "action", "reward", "done",
                                                                   "replica")], None, None, None, size, n, w)
        nets = _QNets(self._targets_ptr_dev.data_ptr(), len(weights), TARGET_MODELS[model],
                      gen_of.data_ptr() if gen_of is not None else None)
        _check(_lib.prisma_replay_targets(self.h, C.byref(rings), idx.data_ptr(), batch, C.byref(nets), float(gamma),
                                          out["obs"].data_ptr(), out["action"].data_ptr(), out["target"].data_ptr(),
                                          out["status"].data_ptr(), _stream_handle(stream)))
        return out

    def log_tensor(self, stream=None):
        import torch
        nbytes = self.R * self.log_capacity * self.rec_bytes
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.torch_device)
        _check(_lib.prisma_copy_log(self.h, buf.data_ptr(), nbytes, _stream_handle(stream)))
        return buf.view(self.R, self.log_capacity, self.rec_bytes)

    def records(self, replica: int, first: int, count: int, log_host: Optional[np.ndarray] = None) -> np.ndarray:
        """Records [first, first+count) of one replica in decision order (host numpy)."""
        if log_host is None:
            import torch
            torch.cuda.synchronize(self.device)
            log_host = self.log_tensor().cpu().numpy()
        if count > self.log_capacity:
            raise PrismaError("requested more records than the log ring holds")
        cap = self.log_capacity
        idx = (np.arange(first, first + count) % cap)
        raw = log_host[replica][idx]
        return raw.reshape(-1).view(self.rec_dtype)
