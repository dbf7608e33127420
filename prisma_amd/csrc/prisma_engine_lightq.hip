// prisma_engine_lightq.hip -- the register-resident engine's step kernels with the in-kernel
// reduced DQN-buffer models (engine_core.h lightq_action_reg: DQN_buffer_lite / lighter /
// lighter_2 / lighter_3, widths as run-time values) and without the --train echo / notify_dest
// code paths (step_kernel.h): prisma_run with PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetLightq)

PRISMA_TU_TIMING(prisma_debug_timing_lightq)
