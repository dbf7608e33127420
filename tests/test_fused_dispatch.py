"""The rule by which PrismaEngine names the step-kernel instances an env launches
(engine.step_kernel_names, the library's own choice restated), on the CPU: fused table runs have
instances of their own exactly where the env is an identity overlay without the ctrl paths and
prisma_plan puts its table in LDS; prisma_step's instance, the MLP's and the memory engine's names never change."""
import pytest

import synth_topology as S
from prisma_amd import engine
from prisma_amd.engine import PRISMA_ENGINE_MEMORY, PRISMA_ENGINE_REGISTER


def _ki(name, ctrl, eng=PRISMA_ENGINE_REGISTER):
    c = S.CASES[name]
    return dict(engine=eng, flow_slots=c["shape"][0], link_slots=c["shape"][1],
                tunnels=int(c["kind"] == "tunnelled"), ctrl=ctrl)


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("name", list(S.CASES))
def test_table_name_follows_ctrl_and_table_place(name, train):
    c = S.CASES[name]
    pl = engine.plan(S.build(name), S.case_params(name, train=train))
    names = engine.step_kernel_names(_ki(name, train), pl)
    fs, ls = c["shape"]
    tun = "true" if c["kind"] == "tunnelled" else "false"
    ctrl = "true" if train else "false"
    assert names["step"] == f"prisma_step_kernel_t<{fs}, {ls}, false, {tun}, {ctrl}>"
    assert names["mlp"] == f"prisma_step_kernel_t<{fs}, {ls}, true, {tun}, {ctrl}>"
    if not train and c["kind"] != "tunnelled" and c["table_in_lds"][0]:
        assert names["table"] == f"prisma_step_kernel_fused_t<{fs}, {ls}, false, false>"
    else:
        assert names["table"] == names["step"]
    # (tests/test_gpu_parity.py reads TUN, CTRL off the end of the label)
    assert names["table"].endswith(f"{tun}, {ctrl}>")


def test_both_places_of_the_table_and_both_overlay_kinds_occur_without_ctrl():
    assert {c["table_in_lds"][0] for c in S.IDENTITY.values()} == {0, 1}
    assert any(c["table_in_lds"][0] for c in S.TUNNELLED.values())


def test_memory_engine_names():
    pl = dict(lds_bytes=4096, lds_state_bytes=1024)
    names = engine.step_kernel_names(dict(engine=PRISMA_ENGINE_MEMORY, flow_slots=0, link_slots=0, tunnels=0, ctrl=0), pl)
    assert names == {"step": "prisma_mem_step_kernel<false, false>", "table": "prisma_mem_step_kernel<false, false>",
                     "mlp": "prisma_mem_step_kernel<true, false>"}
