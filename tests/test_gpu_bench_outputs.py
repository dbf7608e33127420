"""bench.py on the device at a small launch shape: a plain run times exactly --steps steps and leaves
the CPU baseline to --full, and --dump-outputs writes the last step's outputs identically run to run."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from prisma_amd.records import COUNTERS_DTYPE, record_dtype  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

R, HOPS, STEPS, WARMUP = 64, 256, 3, 1
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--replicas", str(R), "--hops", str(HOPS)]


def _run(capsys, *extra):
    bench.main([*ARGS, *extra])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _run(capsys, "--dump-outputs", a)
    _run(capsys, "--dump-outputs", b)
    assert "cpu_baseline" not in d                          # behind --full
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["errors"] == 0
    assert d["ms_per_step"] > 0 and d["unit"] == "hops/s" and d["dtype"] == "int64" and d["higher_is_better"]
    assert abs(d["value"] - R * HOPS * STEPS / (d["ms_per_step"] * 1e-3 * STEPS)) <= 1e-9 * d["value"]
    names = sorted(os.listdir(a))
    assert names == ["counters.npy", "log.npy", "log_replicas.npy", "policy.npy"] == sorted(os.listdir(b))
    got = {n: np.load(os.path.join(a, n)) for n in names}
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for n, v in got.items():
        assert v.dtype in (np.float32, np.float64), n
        assert np.array_equal(v, np.load(os.path.join(b, n)), equal_nan=True), n
    cnt = got["counters.npy"]
    assert cnt.shape == (R, len(COUNTERS_DTYPE.names))
    # every replica executed exactly --hops hops in each of the warm-up and the timed steps
    assert np.all(cnt[:, COUNTERS_DTYPE.names.index("hops_total")] == (WARMUP + STEPS) * HOPS)
    assert np.all(cnt[:, COUNTERS_DTYPE.names.index("error")] == 0)
    assert got["policy.npy"].shape == (11, 11)              # Abilene's DQ-routing action table
    pick, log = got["log_replicas.npy"], got["log.npy"]
    assert pick.shape == (16,) and len(set(pick.tolist())) == 16 and pick.min() >= 0 and pick.max() < R
    scalars = [f for f in record_dtype(4).names if f != "obs"]
    assert log.shape == (16, 8192, len(scalars) + 4)
    dec = cnt[pick.astype(int), COUNTERS_DTYPE.names.index("dec_count")].astype(int)
    assert dec.min() > 0
    for k, n_dec in enumerate(dec):                         # the ring holds each replica's decisions, then zeros
        assert np.all(log[k, :n_dec, scalars.index("t_ns")] > 0) and not log[k, n_dec:].any()


def test_full_run_adds_the_cpu_baseline(capsys):
    d = _run(capsys, "--full", "--cpu-hops", "4000")
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert "cpu_baseline" not in _run(capsys, "--full", "--cpu-baseline", "0")
