// prisma_engine_smart_mlp.hip -- the register-resident engine's step kernels with the in-kernel
// DQN-buffer policy and history-weighted exploration (engine_core.h smart_explore_action),
// without the --train echo / notify_dest code paths (step_kernel.h): prisma_run_explore_smart
// with PRISMA_POLICY_DQN_BUFFER.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetSmartMlp)

PRISMA_TU_TIMING(prisma_debug_timing_smart_mlp)
