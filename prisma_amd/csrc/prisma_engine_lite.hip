// prisma_engine_lite.hip -- the register-resident engine's table-policy step kernels without
// the --train echo and notify_dest code paths (step_kernel.h), picked by prisma_create when
// neither is set (every table-policy benchmark configuration, the headline among them).
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetLite)

PRISMA_TU_TIMING(prisma_debug_timing_lite)
PRISMA_TU_WAVE_TIMES(prisma_debug_wave_times_lite)
