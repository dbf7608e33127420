// step_kernel.h -- the register-resident engine's step kernel templates and the table of their
// instance sets (StepSet, kStepSets), included by every translation unit that compiles one set.
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

// The instance sets: one translation unit each (prisma_engine_<name>.hip; ctrl in prisma_engine.hip,
// ctrl_mlp in prisma_engine_mlp.hip), so the sets compile in parallel.  This table is the list of
// sets: a row gives the template arguments of the set's kernels (step_kernel below), and prisma_create
// fills one launch slot per row from it (which also says what adding a set touches).
//   mlp:   the in-kernel model is compiled in (mode 4 only) and its LDS is part of the launch
//          (Layout::lds_mlp_bytes, else lds_bytes); the table / external instances carry none of
//          its code or registers.
//   ctrl:  the --train echo and notify_dest paths are compiled in; these sets serve the envs that
//          need them (ns-3 streams and tunnelled overlays with a log of 2^18 records too), the
//          others every other env.
//   expl:  event_loop's EXPL -- 0 greedy, 1 epsilon-greedy exploration of the fused policy
//          (engine_core.h explore_action), 2 history-weighted exploration (smart_explore_action),
//          3 stochastic multipath routing (stoch_action).  Sets of their own, so the greedy ones keep
//          their code and registers.  (The parameter sits in the kernel itself: with the body in a
//          shared inlined function taking the arguments by reference the headline instance came out
//          with 7 more SGPR spill slots and the DQN-buffer one with 16 B more scratch.)
//   lq:    the model is one of the reduced DQN-buffer models (lightq_action_reg; widths in
//          KParams::lq_dims).
//   fused: the table instances that only fused runs (prisma_run with a table) launch, on
//          identity-overlay envs whose table sits in LDS: event_loop's table_mode and the table's
//          place are compile-time constants there, so the external-policy exit of an arrival (the
//          Decision stored to the header, the pending observation, the PENDING record), the
//          P.actions branch and the HBM table pointer are not in the kernel.  The mlp / lq sets
//          fold table_mode already; the general table sets keep the run-time value and serve
//          prisma_step, the ctrl envs, envs whose table stays in HBM and the tunnelled overlays
//          (A/B, profiles/fused_inst/: headline +3.2 %, SP at its shape +2.6 %, but config 3's SP
//          line on the tunnelled (2, 1) instance -0.35 % at a 0.25 % spread, so those are not
//          instantiated).  (stoch: event_loop's folding only -- no table is read and no external
//          action taken, so it holds for the tunnelled ones as well.)
#define PRISMA_STEP_SETS(X)                                                                             \
    /* id            name              mlp    ctrl   expl lq     fused */                               \
    X(Ctrl,          "ctrl",           false, true,  0,   false, false) /* prisma_step, table runs: ctrl envs */ \
    X(CtrlMlp,       "ctrl_mlp",       true,  true,  0,   false, false) /* PRISMA_POLICY_DQN_BUFFER: ctrl envs */ \
    X(Lite,          "lite",           false, false, 0,   false, false) /* prisma_step, table runs: other envs */ \
    X(LiteMlp,       "lite_mlp",       true,  false, 0,   false, false) /* PRISMA_POLICY_DQN_BUFFER (configs 3, 4) */ \
    X(Fused,         "fused",          false, false, 0,   false, true)  /* prisma_run with a table (the headline) */ \
    X(Explore,       "explore",        false, false, 1,   false, false) /* prisma_run_explore */        \
    X(ExploreMlp,    "explore_mlp",    true,  false, 1,   false, false)                                 \
    X(Lightq,        "lightq",         true,  false, 0,   true,  false) /* PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3 */ \
    X(ExploreLightq, "explore_lightq", true,  false, 1,   true,  false)                                 \
    X(Smart,         "smart",          false, false, 2,   false, false) /* prisma_run_explore_smart */  \
    X(SmartMlp,      "smart_mlp",      true,  false, 2,   false, false)                                 \
    X(SmartLightq,   "smart_lightq",   true,  false, 2,   true,  false)                                 \
    X(Stoch,         "stoch",          false, false, 3,   false, true)  /* prisma_run_stochastic */
#define PRISMA_SET_ID_(ID_, ...) kSet##ID_,
enum StepSet { PRISMA_STEP_SETS(PRISMA_SET_ID_) kNumStepSets };
struct StepSetInfo { const char* name; bool mlp, ctrl; int expl; bool lq, fused; };
#define PRISMA_SET_ROW_(ID_, ...) { __VA_ARGS__ },
constexpr StepSetInfo kStepSets[kNumStepSets] = { PRISMA_STEP_SETS(PRISMA_SET_ROW_) };
// The set's kernel for an env's slot counts and overlay kind, or null (fused: tunnelled overlays;
// every set: a shape outside PRISMA_STEP_SHAPES).  It dispatches to the set's translation unit,
// which defines its specialisation of prisma_pick_step_set with PRISMA_TU_STEP_SET.
const void* prisma_pick_step(StepSet set, int fs, int ls, bool tun);
template <StepSet S> const void* prisma_pick_step_set(int fs, int ls, bool tun);
#define PRISMA_SET_DECL_(ID_, ...) template <> const void* prisma_pick_step_set<kSet##ID_>(int fs, int ls, bool tun);
PRISMA_STEP_SETS(PRISMA_SET_DECL_)

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
    sim_bind(S, lv, lds, replica_topo(P, r), P.log + (size_t)r * LC.log_cap * LC.rec_bytes, LC.replica_base + (uint32_t)r, lane); \
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
#define PRISMA_STEP_SHAPES(X) X(1, 1) X(1, 2) X(1, 4) X(2, 1) X(2, 2) X(2, 4) X(4, 1) X(4, 2) X(4, 4) X(8, 1) X(8, 2) X(8, 4)

// the kernel of set S for <FS, LS, TUN> (tun: tunnelled-overlay instance; identity overlays run
// code without the tunnel paths), by its row of kStepSets
template <StepSet S, int FS, int LS, bool TUN> const void* step_kernel() {
    constexpr StepSetInfo I = kStepSets[S];
    static_assert(!(I.expl && I.ctrl), "the exploring instances carry no ctrl paths");
    static_assert(!I.lq || (I.mlp && !I.ctrl), "the reduced-model instances are MLP instances without the ctrl paths");
    if constexpr (I.expl == 3) return (const void*)prisma_step_kernel_stoch_t<FS, LS, TUN, I.ctrl>;
    else if constexpr (I.expl == 2) return (const void*)prisma_step_kernel_smart_t<FS, LS, I.mlp, TUN, I.lq>;
    else if constexpr (I.fused) return TUN ? nullptr : (const void*)prisma_step_kernel_fused_t<FS, LS, false, I.ctrl>;
    else return (const void*)prisma_step_kernel_t<FS, LS, I.mlp, TUN, I.ctrl, I.expl == 1, I.lq>;
}

// (a template, so only the translation unit that names a set instantiates its kernels)
template <StepSet S> static const void* pick_step(int fs, int ls, bool tun) {
#ifdef PRISMA_DEV_HEADLINE
    // register-allocation experiments only (scripts/asm_headline.sh): compile the headline instance
    // alone -- the fused one, or with -DPRISMA_DEV_GENERAL the general one prisma_step launches
#ifdef PRISMA_DEV_GENERAL
    constexpr StepSet kDev = kSetLite;
#else
    constexpr StepSet kDev = kSetFused;
#endif
    if constexpr (S == kDev) return (fs == 2 && ls == 1 && !tun) ? step_kernel<S, 2, 1, false>() : nullptr;
    else return nullptr;
#else
#define PK(F_, L_) if (fs == F_ && ls == L_) return tun ? step_kernel<S, F_, L_, true>() : step_kernel<S, F_, L_, false>();
    PRISMA_STEP_SHAPES(PK)
#undef PK
    return nullptr;
#endif
}
#define PRISMA_TU_STEP_SET(S)                                                                           \
    template <> const void* prisma_pick_step_set<S>(int fs, int ls, bool tun) { return pick_step<S>(fs, ls, tun); }

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
