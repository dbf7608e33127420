// prisma_engine_fused.hip -- the register-resident engine's table-policy step kernels for fused
// runs only (step_kernel.h prisma_step_kernel_fused_t): no external-policy path and the table read
// from LDS, without the --train echo and notify_dest code paths.  prisma_run with a table launches
// them on identity-overlay envs without the ctrl paths whose table sits in LDS (the headline among
// them); prisma_step and every other env launch the general instances.
#include "step_kernel.h"

PRISMA_TU_STEP_SET(kSetFused)

PRISMA_TU_TIMING(prisma_debug_timing_fused)
PRISMA_TU_WAVE_TIMES(prisma_debug_wave_times_fused)
