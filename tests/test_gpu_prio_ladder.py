"""The issue-priority ladder (engine_core.h prio_update, prio_ladder.h) changes when a wave issues,
never what it computes: every replica is its own wave.  The 4-wave instances against the CPU
oracle, byte for byte, at hop budgets that put the ladder's boundaries everywhere its bookkeeping
can go wrong -- around the shipped chunk size C (the chunk of the bench's 32 768-hop launch: at a
budget of C hops the chunks are a hop or two long, so every hop is a boundary), below the chunk
count (the degenerate one-level ladder), as one launch and as two (the second starts with a
pending decision, so finish_pending's hop precedes the loop and can step over a boundary), through
an episode end inside a launch (spare_restart and the second event-loop copy, which continues on
the ladder at prio_base = the hops done), and on a tunnelled instance (config 3's kernels)."""
import os
import re

import pytest
import torch

from parity_util import compare_steady, random_table, run_fused_both
from prisma_amd.config import engine_params
from prisma_amd.engine import PRISMA_ENGINE_REGISTER, PrismaEngine
from prisma_amd.topology import Topology, sp_next_hop_table

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "prisma_amd", "csrc",
                         "prio_ladder.h")).read()
CHUNKS = int(re.search(r"^#define PRISMA_PRIO_CHUNKS (\d+)", _HDR, re.M).group(1))
C = 32768 // CHUNKS                            # the shipped chunk at the bench's launch size
R = 8
FOUR_WAVE = dict(engine=PRISMA_ENGINE_REGISTER, flow_slots=2, link_slots=1, ctrl=0)
# (CHUNKS - 1: below the chunk count, the ladder is one level)
BUDGETS = list(dict.fromkeys([1, 2, C - 1, C, C + 1, 4 * C + 3, CHUNKS - 1]))


@pytest.mark.parametrize("launches", [1, 2])
@pytest.mark.parametrize("budget", BUDGETS)
def test_headline_instance_around_the_chunk(oracle_mod, budget, launches):
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=60.0, ping_as_obs=1, seed=100, replica_base=4088, log_capacity=8192)
    run_fused_both(oracle_mod, topo, params, R, budget * launches, ("table", random_table(topo, 5)),
                   launches=launches, kernel=dict(FOUR_WAVE, tunnels=0), label=f"abilene budget {budget} x {launches}")


def test_episode_end_inside_a_launch(oracle_mod):
    """1-s episodes with auto_reset at 4 C + 3 hops per launch: an episode (about two thousand hops)
    ends inside a launch with budget left, and the replica continues on the ladder in the second
    event-loop copy; through two episode ends per replica."""
    topo = Topology.example("abilene", 0, 1.0)
    params = engine_params(topo, sim_time_s=1.0, ping_as_obs=1, auto_reset=1, seed=100, replica_base=4088,
                           log_capacity=8192)
    eng = PrismaEngine(topo, params, R)
    try:
        ki = eng.kernel_info()
        assert {k: ki[k] for k in FOUR_WAVE} == FOUR_WAVE, ki
        eng.reset(0)
        out = compare_steady(oracle_mod, eng, topo, params, ("table", random_table(topo, 5)), t_target_s=2.1,
                             hops_per_launch=4 * C + 3, min_episode=2, label="abilene 1-s episodes")
    finally:
        eng.close()
    assert min(out["episodes"]) >= 2 and out["short_launches"] == 0


def test_tunnelled_four_wave_instance(oracle_mod):
    topo = Topology.example("abilene_on_geant", 0, 1.0)
    params = engine_params(topo, sim_time_s=60.0, ping_as_obs=1, seed=100, replica_base=4088, log_capacity=8192)
    run_fused_both(oracle_mod, topo, params, R, 2 * (4 * C + 3), ("table", sp_next_hop_table(topo)), launches=2,
                   kernel=dict(FOUR_WAVE, tunnels=1), label="abilene_on_geant sp")
