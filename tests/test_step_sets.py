"""The step-kernel instance table (step_kernel.h PRISMA_STEP_SETS) and its one picker: a stand-alone
C++ program linked against libprisma_amd.so calls prisma_pick_step for every set, shape and overlay
kind.  No GPU: the picker returns the kernels' host addresses."""
import os
import re
import subprocess
import tempfile

from prisma_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_KERNEL_H = os.path.join(ROOT, "prisma_amd", "csrc", "step_kernel.h")

# the sets that exist, in the table's order, and the shapes every set is instantiated for
SETS = ["ctrl", "ctrl_mlp", "lite", "lite_mlp", "fused", "explore", "explore_mlp", "lightq", "explore_lightq",
        "smart", "smart_mlp", "smart_lightq", "stoch"]
SHAPES = [(fs, ls) for fs in (1, 2, 4, 8) for ls in (1, 2, 4)]
OUTSIDE = [(3, 1), (2, 3), (16, 1), (1, 8), (0, 0)]

PROBE = r'''
#include <stdio.h>
enum StepSet { %(ids)s kNumStepSets };
const void* prisma_pick_step(StepSet set, int fs, int ls, bool tun);
int main() {
  static const int shapes[][2] = { %(shapes)s };
  for (int s = 0; s < kNumStepSets; ++s)
    for (const auto& sh : shapes)
      for (int tun = 0; tun < 2; ++tun) {
        const void* k = prisma_pick_step((StepSet)s, sh[0], sh[1], tun != 0);
        printf("%%d %%d %%d %%d %%d %%p\n", s, sh[0], sh[1], tun, k == nullptr, k);
      }
  return 0;
}
'''


def table_rows():
    """(id, name) of every row of PRISMA_STEP_SETS."""
    txt = open(STEP_KERNEL_H).read()
    body = txt[txt.index("#define PRISMA_STEP_SETS(X)"):txt.index("#define PRISMA_SET_ID_")]
    return re.findall(r'\bX\((\w+),\s*"(\w+)"', body)


def test_table_lists_the_thirteen_sets():
    assert [name for _, name in table_rows()] == SETS


def test_picker_is_complete():
    lib_dir = os.path.dirname(engine.LIB_PATH)
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_engine()
    src = PROBE % dict(ids=" ".join(f"kSet{i}," for i, _ in table_rows()),
                       shapes=", ".join("{%d, %d}" % s for s in SHAPES + OUTSIDE))
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        open(cpp, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", cpp, "-o", exe, "-L", lib_dir, "-lprisma_amd",
                               "-Wl,-rpath," + lib_dir, "-Wl,--allow-shlib-undefined"])
        out = subprocess.check_output([exe], text=True)
    got = {}
    for line in out.splitlines():
        s, fs, ls, tun, null, ptr = line.split()
        got[(SETS[int(s)], (int(fs), int(ls)), int(tun))] = (int(null), ptr)
    assert len(got) == len(SETS) * (len(SHAPES) + len(OUTSIDE)) * 2
    inside = {k: v for k, v in got.items() if k[1] in SHAPES}
    assert len(inside) == 13 * 12 * 2
    # null for exactly the twelve (fused, tunnelled) combinations
    assert sorted(k for k, (null, _) in inside.items() if null) == sorted(("fused", sh, 1) for sh in SHAPES)
    # the other 300 are 300 different kernels
    ptrs = [ptr for null, ptr in inside.values() if not null]
    assert len(ptrs) == 300 and len(set(ptrs)) == 300
    # a shape outside the twelve has no instance in any set
    assert all(null for k, (null, _) in got.items() if k[1] in OUTSIDE)
