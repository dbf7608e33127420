// prisma_engine_explore.hip -- the register-resident engine's table-policy step kernels with
// epsilon-greedy exploration (engine_core.h explore_action) and without the --train echo and
// notify_dest code paths (step_kernel.h): prisma_run_explore with PRISMA_POLICY_TABLE.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetExplore)

PRISMA_TU_TIMING(prisma_debug_timing_explore)
