#!/bin/bash
# Assembly of the headline step kernel alone (-DPRISMA_DEV_HEADLINE), with instruction-class
# counts: a quick static check of what a change does to the hot kernel (spills show up as
# scratch_* and v_writelane/v_readlane pairs).  The fused-only instance that prisma_run launches,
# or with --general the general instance that prisma_step launches.
# Usage: bash scripts/asm_headline.sh [--general] [out.s] [-D...]
cd "$(dirname "$0")/.."
SRC=prisma_engine_fused.hip; SYM=_Z26prisma_step_kernel_fused_tILi2ELi1ELb0ELb0EEv7KParams; DEV=
if [ "$1" == "--general" ]; then
  SRC=prisma_engine_lite.hip; SYM=_Z20prisma_step_kernel_tILi2ELi1ELb0ELb0ELb0ELb0ELb0EEv7KParams; DEV=-DPRISMA_DEV_GENERAL; shift
fi
OUT=${1:-/tmp/headline.s}; shift
FLAGS=$(python -c "from prisma_amd import buildid; print(' '.join(buildid.HIPCC_FLAGS))")
/opt/rocm/bin/hipcc $FLAGS -DPRISMA_DEV_HEADLINE $DEV "$@" --cuda-device-only -S -o $OUT prisma_amd/csrc/$SRC || exit 1
python - "$OUT" "$SYM" <<'PY'
import re, sys
txt = open(sys.argv[1]).read()
m = re.search(rf"^{sys.argv[2]}:[^\n]*\n(.*?)^\.Lfunc_end", txt, re.S | re.M)
if not m:
    sys.exit(f"{sys.argv[2]} not found in {sys.argv[1]}")
body = m.group(1)
ins = [l.strip().split()[0] for l in body.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
cnt = lambda p: sum(1 for i in ins if i.startswith(p))
print(f"instructions {len(ins)}  scratch {cnt('scratch_')}  v_writelane {cnt('v_writelane')}  "
      f"v_readlane {cnt('v_readlane')}  s_swappc/call {cnt('s_swappc')+cnt('s_call')}  "
      f"s_ {cnt('s_')}  v_ {cnt('v_')}  ds_ {cnt('ds_')}  global_ {cnt('global_')}  flat_ {cnt('flat_')}  "
      f"s_cbranch {cnt('s_cbranch')}")
# the event-loop copies: the unions of the backward branches that span more than 1500 lines
lines = body.splitlines()
lab = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
spans = []
for i, l in enumerate(lines):
    m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in lab and i - lab[m.group(1)] > 1500:
        a = lab[m.group(1)]
        if spans and a <= spans[-1][1]:
            spans[-1] = (min(a, spans[-1][0]), i)
        else:
            spans.append((a, i))
for n, (a, b) in enumerate(spans):
    li = [l.strip().split()[0] for l in lines[a:b + 1] if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c = lambda p: sum(1 for i in li if i.startswith(p))
    print(f"event-loop copy {n}: instructions {len(li)}  flat_ {c('flat_')}  ds_read_u8 {c('ds_read_u8')}  "
          f"v_readlane {c('v_readlane')}  s_ {c('s_')}  v_ {c('v_')}")
for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
    mm = re.findall(rf"\.{k}:\s+(\d+)", txt)
    print(k, mm[:4])
PY
