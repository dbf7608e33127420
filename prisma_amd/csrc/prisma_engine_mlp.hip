// prisma_engine_mlp.hip -- the register-resident engine's step kernels with the in-kernel
// DQN-buffer policy and the --train echo / notify_dest code paths (step_kernel.h).
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetCtrlMlp)

PRISMA_TU_TIMING(prisma_debug_timing_mlp)
