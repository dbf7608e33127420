// prisma_engine_smart.hip -- the register-resident engine's table-policy step kernels with
// history-weighted exploration (engine_core.h smart_explore_action) and without the --train echo
// and notify_dest code paths (step_kernel.h): prisma_run_explore_smart with PRISMA_POLICY_TABLE.
#include "step_kernel.h"

const void* prisma_pick_step_smart(int fs, int ls, bool tun) { return pick_step_smart<false>(fs, ls, tun); }

PRISMA_TU_TIMING(prisma_debug_timing_smart)
