// step_kernel.h -- the register-resident engine's step kernel template and its instance table,
// included by prisma_engine.hip (instances with the --train echo / notify_dest code, CTRL) and
// prisma_engine_lite.hip (instances without it: the compiler allocates registers for every
// path a kernel contains, and these rarely-taken ones cost the common case ~2 %), and by
// prisma_engine_fused.hip (table instances for fused runs only, without the external-policy path).
#pragma once
#include "engine_core.h"

// waves per SIMD the register allocator must leave room for: 4 (<= 128
// VGPRs) for small replicas so 4096 of them are resident on 256 CUs at
// once, 2 (<= 256) up to 512 flows x 128 links
template <int FS, int LS> struct StepOcc {
    static constexpr int waves = (FS <= 2 && LS == 1) ? 4 : (LS <= 2 ? 2 : 1);
    // DQN-buffer weight loads in flight per lane: 4 where the kernel must fit 128 VGPRs
    // (4 waves per SIMD), 8 where it has 256
    static constexpr int mlp_batch = waves >= 4 ? 4 : 8;
};

// MLP: the in-kernel DQN-buffer policy is compiled in (mode 4 only); the table /
// external instances carry none of its code or registers.  CTRL: the --train echo and
// notify_dest paths are compiled in (used when either is set).  EXPL: epsilon-greedy exploration
// of the fused policy (engine_core.h explore_action) -- instances of their own, so the greedy
// ones keep their code and registers.  (The parameter sits in the kernel itself: with the body in
// a shared inlined function taking the arguments by reference the headline instance came out
// with 7 more SGPR spill slots and the DQN-buffer one with 16 B more scratch.)  LQ: the MLP is the
// reduced DQN-buffer models' decision (engine_core.h lightq_action_reg; widths in KParams::lq_dims)
// -- instance sets of their own again, greedy and exploring, without the ctrl paths.  FUSED: the
// table instances that only fused runs (prisma_run with a table) launch, for identity-overlay envs
// without the ctrl paths whose table sits in LDS: event_loop's table_mode and the table's place are compile-time
// constants there, so the external-policy exit of an arrival (the Decision stored to the header,
// the pending observation, the PENDING record), the P.actions branch and the HBM table pointer are
// not in the kernel.  The MLP / LQ instances fold table_mode already (MLP is a template argument);
// the general table instances keep the run-time value and serve prisma_step, the ctrl envs, envs
// whose table stays in HBM and the tunnelled overlays (A/B, profiles/fused_inst/: headline +3.2 %,
// SP at its shape +2.6 %, but config 3's SP line on the tunnelled (2, 1) instance -0.35 % at a
// 0.25 % spread, so those are not instantiated).
#if PRISMA_WAVE_TIMES
// diagnostic build only (scripts/wave_times.py): each replica's wave start / end (s_memrealtime,
// 100 MHz) and hardware ids of its last launch
__device__ unsigned long long g_wave_times[4 * 65536];
#define WT_START() const uint64_t wt0_ = __builtin_amdgcn_s_memrealtime()
#define WT_END()                                                                                       \
    do {                                                                                               \
        const uint64_t wt1_ = __builtin_amdgcn_s_memrealtime();                                        \
        if (lane == 0 && r < 65536) {                                                                  \
            g_wave_times[4 * r] = wt0_; g_wave_times[4 * r + 1] = wt1_;                                \
            g_wave_times[4 * r + 2] = (unsigned)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)); \
            g_wave_times[4 * r + 3] = (unsigned)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (15 << 11)); \
        }                                                                                              \
    } while (0)
#else
#define WT_START() do { } while (0)
#define WT_END() do { } while (0)
#endif

// The kernel body, shared by the kernel templates below (EXPL_: 0 greedy, 1 uniform
// exploration, 2 history-weighted exploration, 3 stochastic multipath routing; FUSED_: the fused-only
// table instances).  A macro
// rather than an inlined function, for the reason given above, and rather than one more template
// parameter, so the existing instances keep their symbol names.
//
// S.prio_total and S.prio_shift (the ladder): 4-wave instances only (at 2 waves per SIMD, config 4's, thresholds lost
// 2 %).
//
// An episode that ends with hop budget left (fused run with auto_reset) continues into the next
// episode from its prebuilt image, in a second inlined copy of the event loop.  A restart inside
// the first loop would give its clock and sequence numbers a second incoming value each iteration
// and cost the hot loop ~20 VGPRs (scripts/asm_headline.sh); this copy runs at most once per
// launch, after which a second episode end stops the replica as before.  The kernel arguments are
// read again there rather than kept in SGPRs across the first loop, and the stage-out uses the
// reloaded arguments too: with P's pointers kept live across the second loop the headline instance
// spilled 7 VGPRs and reloaded them inside it (round 6: 128 VGPRs + 32 B scratch -> 123 VGPRs, no
// scratch).  The reloaded arguments sit in VGPRs; the smart instances move the history pointer
// to SGPRs there (two more VGPRs held across the second loop made the headline shape's instance
// spill 4 VGPRs in that loop's prologue: 20 B scratch, none with the pointer in SGPRs).
#define PRISMA_STEP_KERNEL_BODY(EXPL_, FUSED_)                                                          \
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];                                 \
    const int r = blockIdx.x, lane = threadIdx.x;                                                       \
    WT_START();                                                                                         \
    CLayout& LC = *(CLayout*)P.lay;                                                                     \
    LV lv;                                                                                              \
    lv.load(P.lay, lane);                                                                               \
    Regs<FS, LS> R;                                                                                     \
    stage_in(lds, P, r, lane, R);                                                                       \
    __syncthreads();                                                                                    \
    Sim S;                                                                                              \
    sim_bind(S, lv, lds, P.topo, P.log + (size_t)r * LC.log_cap * LC.rec_bytes, LC.replica_base + (uint32_t)r, lane); \
    S.tun = TUN;                                                                                        \
    S.ctrl = CTRL;                                                                                      \
    S.lanel = PRISMA_LANE_LINKS != 0 && (FUSED_) && (EXPL_) == 0 && LS == 1 && FS <= 4 && !TUN && !CTRL; \
    if (S.lanel) lane_links_bind(S);                                                                    \
    if (TUN) S.ring = (uint32_t*)(P.state + (size_t)r * LC.state_bytes + LC.s_ring);   /* HBM FIFOs */  \
    uint32_t budget = (uint32_t)P.max_hops;                                                             \
    S.prio_total = StepOcc<FS, LS>::waves >= 4 ? budget : 0u;                                           \
    S.prio_shift = StepOcc<FS, LS>::waves >= 4 ? prio_ladder_shift(budget) : 31u;                       \
    const uint32_t done = event_loop<MLP, StepOcc<FS, LS>::mlp_batch, EXPL_, LQ, FUSED_>(P, S, R, r, budget); \
    if (P.spare && done < budget) {                                                                     \
        const KParams* kp = (const KParams*)__builtin_amdgcn_kernarg_segment_ptr();                     \
        asm volatile("" : "+s"(kp));                                                                    \
        KParams P2 = *kp;                                                                               \
        if (EXPL_ == 2) P2.action_hist = rfl_ptr(P2.action_hist);                                       \
        if (EXPL_ == 3) P2.stoch_tab = rfl_ptr(P2.stoch_tab);                                           \
        if (spare_restart(P2, S, R, r, done, budget)) {                                                 \
            S.prio_base = done;                                                                         \
            event_loop<MLP, StepOcc<FS, LS>::mlp_batch, EXPL_, LQ, FUSED_>(P2, S, R, r, budget);        \
            stage_out(lds, P2, r, lane, R);                                                             \
            WT_END();                                                                                   \
            return;                                                                                     \
        }                                                                                               \
    }                                                                                                   \
    stage_out(lds, P, r, lane, R);                                                                      \
    WT_END();

template <int FS, int LS, bool MLP, bool TUN, bool CTRL, bool EXPL = false, bool LQ = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(StepOcc<FS, LS>::waves)))
prisma_step_kernel_t(KParams P) {
    PRISMA_STEP_KERNEL_BODY(EXPL ? 1 : 0, false)
}

// SMART: the instances with history-weighted exploration (engine_core.h smart_explore_action;
// prisma_run_explore_smart), without the ctrl paths -- sets of their own once more, beside the
// exploring ones
template <int FS, int LS, bool MLP, bool TUN, bool LQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(StepOcc<FS, LS>::waves)))
prisma_step_kernel_smart_t(KParams P) {
    constexpr bool CTRL = false;
    PRISMA_STEP_KERNEL_BODY(2, false)
}

// FUSED: the table instances of fused runs (above).  The parameters end in TUN, CTRL as the
// general template's label does; only TUN = false, CTRL = false is instantiated.
template <int FS, int LS, bool TUN, bool CTRL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(StepOcc<FS, LS>::waves)))
prisma_step_kernel_fused_t(KParams P) {
    static_assert(!CTRL, "the fused-only instances carry no ctrl paths");
    constexpr bool MLP = false, LQ = false;
    PRISMA_STEP_KERNEL_BODY(0, true)
}

// STOCH: the instances of prisma_run_stochastic (engine_core.h stoch_action), without the ctrl
// paths and fused-only: no table is read and no external action taken, so event_loop's FUSED
// folding applies to the tunnelled ones as well.  The parameters end in TUN, CTRL as the fused
// template's do; only CTRL = false is instantiated.
template <int FS, int LS, bool TUN, bool CTRL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(StepOcc<FS, LS>::waves)))
prisma_step_kernel_stoch_t(KParams P) {
    static_assert(!CTRL, "the stoch instances carry no ctrl paths");
    constexpr bool MLP = false, LQ = false;
    PRISMA_STEP_KERNEL_BODY(3, true)
}

// instantiations: flow slots FS in {1,2,4,8} (F <= 512), link slots LS in {1,2,4} (L <= 256)
template <int FS, int LS, bool CTRL, bool MLP, bool EXPL = false, bool LQ = false> const void* step_kernel(bool tun) {
    static_assert(!(EXPL && CTRL), "the exploring instances carry no ctrl paths");
    static_assert(!LQ || (MLP && !CTRL), "the reduced-model instances are MLP instances without the ctrl paths");
    return tun ? (const void*)prisma_step_kernel_t<FS, LS, MLP, true, CTRL, EXPL, LQ>
               : (const void*)prisma_step_kernel_t<FS, LS, MLP, false, CTRL, EXPL, LQ>;
}

// tun: tunnelled-overlay instance (identity overlays run code without the tunnel paths).
// One translation unit per (CTRL, MLP) instance set, so the sets compile in parallel:
// prisma_engine.hip (CTRL, tables), prisma_engine_mlp.hip (CTRL, MLP), prisma_engine_lite.hip
// and prisma_engine_lite_mlp.hip (without the ctrl paths), prisma_engine_explore.hip and
// prisma_engine_explore_mlp.hip (EXPL, without the ctrl paths), prisma_engine_lightq.hip and
// prisma_engine_explore_lightq.hip (LQ, without the ctrl paths), prisma_engine_smart.hip,
// prisma_engine_smart_mlp.hip and prisma_engine_smart_lightq.hip (SMART, without the ctrl paths),
// prisma_engine_fused.hip (FUSED tables, without the ctrl paths), prisma_engine_stoch.hip (STOCH)
template <bool CTRL, bool MLP, bool EXPL = false, bool LQ = false>
static const void* pick_step(int fs, int ls, bool tun) {
#ifdef PRISMA_DEV_HEADLINE
    // register-allocation experiments only: compile the headline instance alone -- the fused
    // one (pick_step_fused), or with -DPRISMA_DEV_GENERAL the general one prisma_step launches
#ifdef PRISMA_DEV_GENERAL
    return (!CTRL && !MLP && !EXPL && !LQ && fs == 2 && ls == 1 && !tun) ? (const void*)prisma_step_kernel_t<2, 1, false, false, false>
                                                         : nullptr;
#else
    return nullptr;
#endif
#else
#define PK(F_, L_) if (fs == F_ && ls == L_) return step_kernel<F_, L_, CTRL, MLP, EXPL, LQ>(tun);
    PK(1, 1) PK(1, 2) PK(1, 4) PK(2, 1) PK(2, 2) PK(2, 4) PK(4, 1) PK(4, 2) PK(4, 4) PK(8, 1) PK(8, 2) PK(8, 4)
#undef PK
    return nullptr;
#endif
}

// (a template as pick_step is, so only the translation unit that calls it instantiates the kernels)
template <bool CTRL>
static const void* pick_step_fused(int fs, int ls, bool tun) {
    static_assert(!CTRL, "the fused-only instances carry no ctrl paths");
#ifdef PRISMA_DEV_HEADLINE
#ifdef PRISMA_DEV_GENERAL
    return nullptr;
#else
    return (fs == 2 && ls == 1 && !tun) ? (const void*)prisma_step_kernel_fused_t<2, 1, false, CTRL> : nullptr;
#endif
#else
    if (tun) return nullptr;
#define PK(F_, L_) if (fs == F_ && ls == L_) return (const void*)prisma_step_kernel_fused_t<F_, L_, false, CTRL>;
    PK(1, 1) PK(1, 2) PK(1, 4) PK(2, 1) PK(2, 2) PK(2, 4) PK(4, 1) PK(4, 2) PK(4, 4) PK(8, 1) PK(8, 2) PK(8, 4)
#undef PK
    return nullptr;
#endif
}

template <bool MLP, bool LQ = false>
static const void* pick_step_smart(int fs, int ls, bool tun) {
#ifdef PRISMA_DEV_HEADLINE
    return nullptr;
#else
#define PK(F_, L_)                                                                                      \
    if (fs == F_ && ls == L_)                                                                           \
        return tun ? (const void*)prisma_step_kernel_smart_t<F_, L_, MLP, true, LQ>                     \
                   : (const void*)prisma_step_kernel_smart_t<F_, L_, MLP, false, LQ>;
    PK(1, 1) PK(1, 2) PK(1, 4) PK(2, 1) PK(2, 2) PK(2, 4) PK(4, 1) PK(4, 2) PK(4, 4) PK(8, 1) PK(8, 2) PK(8, 4)
#undef PK
    return nullptr;
#endif
}

template <bool CTRL>
static const void* pick_step_stoch(int fs, int ls, bool tun) {
#ifdef PRISMA_DEV_HEADLINE
    return nullptr;
#else
#define PK(F_, L_)                                                                                      \
    if (fs == F_ && ls == L_)                                                                           \
        return tun ? (const void*)prisma_step_kernel_stoch_t<F_, L_, true, CTRL>                        \
                   : (const void*)prisma_step_kernel_stoch_t<F_, L_, false, CTRL>;
    PK(1, 1) PK(1, 2) PK(1, 4) PK(2, 1) PK(2, 2) PK(2, 4) PK(4, 1) PK(4, 2) PK(4, 4) PK(8, 1) PK(8, 2) PK(8, 4)
#undef PK
    return nullptr;
#endif
}

#if PRISMA_WAVE_TIMES
#define PRISMA_TU_WAVE_TIMES(NAME)                                                                      \
    extern "C" int NAME(unsigned long long* out, int n) {                                               \
        return (hipDeviceSynchronize() == hipSuccess &&                                                 \
                hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), 4 * sizeof(unsigned long long) * n) == hipSuccess) ? 0 : -1; \
    }
#else
#define PRISMA_TU_WAVE_TIMES(NAME)
#endif

#if PRISMA_TIMING
// diagnostic build only: read and clear this translation unit's per-phase cycle totals
// (g_prisma_timing is one copy per translation unit; scripts/timing.py)
#define PRISMA_TU_TIMING(NAME)                                                                          \
    extern "C" int NAME(unsigned long long* out32) {                                                    \
        if (hipDeviceSynchronize() != hipSuccess ||                                                     \
            hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_prisma_timing), kTimingWords * sizeof(unsigned long long)) != \
                hipSuccess) return -1;                                                                  \
        unsigned long long z[kTimingWords] = {0};                                                                 \
        return hipMemcpyToSymbol(HIP_SYMBOL(g_prisma_timing), z, sizeof(z)) == hipSuccess ? 0 : -1;     \
    }
#else
#define PRISMA_TU_TIMING(NAME)
#endif
