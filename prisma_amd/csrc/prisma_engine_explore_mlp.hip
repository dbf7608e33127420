// prisma_engine_explore_mlp.hip -- the register-resident engine's step kernels with the
// in-kernel DQN-buffer policy and epsilon-greedy exploration (engine_core.h explore_action),
// without the --train echo / notify_dest code paths (step_kernel.h): prisma_run_explore with
// PRISMA_POLICY_DQN_BUFFER.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetExploreMlp)

PRISMA_TU_TIMING(prisma_debug_timing_explore_mlp)
