// prisma_engine_stoch.hip -- the register-resident engine's step kernels with in-kernel stochastic
// multipath routing (engine_core.h stoch_action; the reference's "opt" agent) and without the
// --train echo and notify_dest code paths (step_kernel.h): prisma_run_stochastic.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetStoch)

PRISMA_TU_TIMING(prisma_debug_timing_stoch)
