"""prisma_ingest_transitions without a device: the declaration, the export, the ABI version, the
null-argument refusal, and train_fused(fused_ingest=True) refusing what keeps the torch path
before it uses the env.  The parity with the torch path is tests/test_gpu_ingest.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from prisma_amd import buildid, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "prisma.h")


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_engine()
    return engine.load_library()


def test_header_declares_and_library_exports():
    txt = open(HEADER).read()
    assert re.search(r"^int\s+prisma_ingest_transitions\s*\(\s*prisma_env_t\*\s*env,\s*int64_t\*\s*consumed,\s*"
                     r"const\s+prisma_replay_t\*\s*rings,\s*void\*\s*stream\s*\)\s*;", txt, re.M)
    assert re.search(r"\}\s*prisma_replay_t;", txt)
    assert "prisma_ingest_transitions" in engine.EXPORTS
    assert "prisma_engine_ingest.hip" in buildid.ENGINE_SOURCES
    lib = _lib()
    assert hasattr(lib, "prisma_ingest_transitions")
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T prisma_ingest_transitions\b", out)


def test_abi_version_unchanged():
    assert re.search(r"#define\s+PRISMA_ABI_VERSION\s+10\b", open(HEADER).read())
    assert _lib().prisma_abi_version() == engine.ABI_VERSION == 10


def test_replay_struct_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "prisma.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(prisma_replay_t), '
                   'offsetof(prisma_replay_t, done), offsetof(prisma_replay_t, size), '
                   'offsetof(prisma_replay_t, n_nodes), offsetof(prisma_replay_t, obs_width)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    R = engine._Replay
    assert got == [C.sizeof(R), R.done.offset, R.size.offset, R.n_nodes.offset, R.obs_width.offset]


def test_null_arguments_are_status_codes():
    lib = _lib()
    rings = engine._Replay()
    assert lib.prisma_ingest_transitions(None, None, C.byref(rings), None) == -5          # PRISMA_ERR_ARG
    assert b"null" in lib.prisma_last_error()
    assert lib.prisma_ingest_transitions(None, None, None, None) == -5
    assert re.search(r"#define\s+PRISMA_ERR_ARG\s+-5\b", open(HEADER).read())


@pytest.mark.parametrize("kw", [dict(prioritized_replay=True), dict(signaling_type="NN")], ids=["prioritized", "NN"])
def test_train_fused_refuses_before_using_the_env(kw):
    from prisma_amd.topology import Topology
    from prisma_amd.trainer import QRoutingTrainer, train_fused
    topo = Topology.example("abilene")
    tr = QRoutingTrainer(topo, "routing", batch_size=32, buffer_size=64, n_replicas=4, device="cpu", **kw)
    with pytest.raises(ValueError, match="prioritized|ideal"):
        train_fused(None, tr, 1, 256, fused_ingest=True)
    with pytest.raises(ValueError, match="prioritized|ideal"):
        tr.observe_env(None)
