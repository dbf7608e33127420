// prisma_engine_smart.hip -- the register-resident engine's table-policy step kernels with
// history-weighted exploration (engine_core.h smart_explore_action) and without the --train echo
// and notify_dest code paths (step_kernel.h): prisma_run_explore_smart with PRISMA_POLICY_TABLE.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetSmart)

PRISMA_TU_TIMING(prisma_debug_timing_smart)
