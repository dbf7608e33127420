// prisma_engine_explore.hip -- the register-resident engine's table-policy step kernels with
// epsilon-greedy exploration (engine_core.h explore_action) and without the --train echo and
// notify_dest code paths (step_kernel.h): prisma_run_explore with PRISMA_POLICY_TABLE.
#include "step_kernel.h"

const void* prisma_pick_step_explore(int fs, int ls, bool tun) { return pick_step<false, false, true>(fs, ls, tun); }

PRISMA_TU_TIMING(prisma_debug_timing_explore)
