// prisma_engine_explore_lightq.hip -- the register-resident engine's step kernels with the
// in-kernel reduced DQN-buffer models (engine_core.h lightq_action_reg) and epsilon-greedy
// exploration (explore_action), without the --train echo / notify_dest code paths
// (step_kernel.h): prisma_run_explore with PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetExploreLightq)

PRISMA_TU_TIMING(prisma_debug_timing_explore_lightq)
