// engine_core.h — device code shared by the two gfx950 engines:
//   * the register-resident engine (prisma_engine.hip): link / flow / ping state
//     lane-distributed in VGPRs (Regs<FS, LS>), FIFOs and wires in LDS -- topologies
//     up to 255 nodes, 256 links and 512 flows;
//   * the memory-resident engine (prisma_engine_mem.hip): the same state as
//     128-byte link records and a 64-ary tournament tree of event keys in HBM
//     (MemSt), for large irregular topologies (ER-256: 2 304 links, 65 280 flows).
// The event handlers below are written once, templated on the store (RS), and
// compiled into both; only the store primitives (link_get / link_put, flow keys,
// ping state, the observation, event selection, init and staging) differ.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/prisma.h"
#include "engine_layout.h"
#include "numerics.h"
#include "mrg32k3a.h"
#include "prio_ladder.h"

using namespace prisma;

#define HIP_OK(x) ((x) == hipSuccess)

// Diagnostic timing build (-DPRISMA_TIMING=1, scripts/timing.py): s_memtime
// cycle totals per loop phase, summed over waves into g_prisma_timing.
#ifndef PRISMA_TIMING
#define PRISMA_TIMING 0
#endif
// Diagnostic event-trace build (-DPRISMA_TRACE=1, scripts/diag_trace.py): lane 0 of
// replicas 0-7 appends (time, kind, id) of every executed event to a device buffer.
#ifndef PRISMA_TRACE
#define PRISMA_TRACE 0
#endif
#if PRISMA_TRACE
static __device__ long long* g_prisma_trace;      // [8][cap][3]
static __device__ unsigned int g_prisma_trace_cap;
static __device__ unsigned int g_prisma_trace_n[8];
#endif
#if PRISMA_TIMING
// one copy per engine (translation unit): 0-7 loop phases, 8-15 their counts, 16-19 mlp_action
// phases, 20-23 memory-resident on_flow phases, 24-39 fine probes TP(i), 40-55 their counts
constexpr int kTimingWords = 64;
static __device__ unsigned long long g_prisma_timing[kTimingWords];
#define TM_NOW() ((uint64_t)__builtin_amdgcn_s_memtime())
#define TM_FLOW(i) do { const uint64_t t_ = TM_NOW(); S.tflow[i] += t_ - S.tfl; S.tfl = t_; } while (0)
// fine probes: cycles since the previous probe (or TP_START) into slot i, scheduling fenced
#define TP_START() do { __builtin_amdgcn_sched_barrier(0); S.tpl = TM_NOW(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define TP(i) do { __builtin_amdgcn_sched_barrier(0); const uint64_t t_ = TM_NOW(); S.tp[i] += t_ - S.tpl; S.tpn[i]++; \
                   S.tpl = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TM_FLOW(i) do { } while (0)
#define TP_START() do { } while (0)
#define TP(i) do { } while (0)
#endif
// probe sets (timing build, -DPRISMA_TP_SET): 0 the decision (mlp_action, apply_decision), 1 the
// memory-resident arrival / completion / flow handlers, 2 the register-resident ones
#ifndef PRISMA_TP_SET
#define PRISMA_TP_SET 0
#endif
#if PRISMA_TP_SET == 0
#define TP0(i) TP(i)
#else
#define TP0(i) do { } while (0)
#endif
#if PRISMA_TP_SET == 1
#define TP1(i) TP(i)
#define TP1_START() TP_START()
#else
#define TP1(i) do { } while (0)
#define TP1_START() do { } while (0)
#endif
#if PRISMA_TP_SET == 2
#define TP2(i) do { if (!S.mem) TP(i); } while (0)
#define TP2_START() do { if (!S.mem) TP_START(); } while (0)
#else
#define TP2(i) do { } while (0)
#define TP2_START() do { } while (0)
#endif

// ---------------------------------------------------------------------------
// kernel parameters
// ---------------------------------------------------------------------------
struct KParams {
    const Layout* __restrict__ lay;  // device copy (read through the scalar cache)
    unsigned char* state;        // [R][state_bytes]
    const unsigned char* topo;   // [topo_bytes]
    unsigned char* log;          // [R][log_cap][rec_bytes]
    prisma_counters_t* cnt_out;  // [R]
    const int32_t* actions;      // [R] or null
    int32_t* obs_out;            // [R][W] or null
    uint8_t* mask_out;           // [R] or null
    int32_t* node_out;           // [R] or null
    const uint8_t* table;        // [N][N] or null
    const float* mlp;            // packed DQN-buffer weights or null (mode 4)
    const float* mlp_rp;         // layers 2-4 of `mlp` interleaved by 4 inputs (mlp_repack), mode 4
    int32_t R;
    int32_t max_hops;
    uint32_t episode;            // reset kernel only
    int32_t mode;                // 0 reset, 1 external step, 2 table run, 3 auto-reset, 4 MLP run
    unsigned char* spare;        // [R][state_bytes] next-episode images (register engine with
                                 // auto_reset), or null
    const uint32_t* rng;         // ns-3 stream mode: the rng table (engine_layout.h kMrgPowers), or null
    const uint32_t* explore_thr; // [N] epsilon-greedy thresholds (prisma_run_explore, EXPL instances), or
                                 // null; last, so the other instances' kernarg offsets stay put
    uint32_t lq_dims;            // reduced DQN-buffer models (the LQ instances): lq_pack_dims(B, H, NH) of the
                                 // weights in `mlp` / `mlp_rp`, else 0; after explore_thr for the same reason
    uint32_t* action_hist;       // [R][T] per-action counts (prisma_run_explore_smart, the smart instances), or
                                 // null; T = ovrow[N].  Last again: no other instance's kernarg offset moves
    const uint32_t* stoch_tab;   // [NO][NO][T] class << 24 | weight (prisma_run_stochastic, the stoch instances), or
                                 // null; last once more
    const uint32_t* topo_off;    // [R] byte offset of replica r's topology image in `topo` (an env with a scenario
                                 // set: one whole image per scenario, prisma_create_scenarios), or null: every
                                 // replica reads the image at `topo`.  Last, as the others
};

// The topology image replica r binds: one scalar load at the start of a launch, and with a single
// scenario (null) the pointer every kernel took before.  The event loop sees one base pointer
// either way (Sim::T, the memory-resident engine's m_* arrays).
__device__ __forceinline__ const unsigned char* replica_topo(const KParams& P, int r) {
    // (the offset selected as a 32-bit value and added once: selecting between the two 64-bit pointers
    // instead cost the headline 0.7 % in alternating A/B, with the same register counts)
    const uint32_t off = P.topo_off ? P.topo_off[r] : 0u;
    return P.topo + off;
}

// ---------------------------------------------------------------------------
// cross-lane helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
// write one lane of a VGPR (v_cmp + v_cndmask; there is no writelane builtin)
__device__ __forceinline__ uint32_t wrl(uint32_t old, uint32_t v, uint32_t lane) {
    return threadIdx.x == lane ? v : old;
}
// lane `src` of v (a wave-wide ds_bpermute; src < 64, no lane-id arithmetic as in __shfl)
__device__ __forceinline__ uint32_t bperm(uint32_t v, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}
__device__ __forceinline__ int64_t mk64(uint32_t lo, uint32_t hi) { return (int64_t)(((uint64_t)hi << 32) | lo); }
__device__ __forceinline__ uint32_t lo32(int64_t v) { return (uint32_t)(uint64_t)v; }
__device__ __forceinline__ uint32_t hi32(int64_t v) { return (uint32_t)((uint64_t)v >> 32); }

// A lane-distributed u32 array of 64*S elements: element i lives in lane
// i % 64, register slot i / 64.  get/set take a wave-uniform index.
template <int S>
struct LA {
    uint32_t v[S];
    // Every slot is read / compared unconditionally so the slot index never
    // becomes a dynamic array index (which would demote v[] to scratch).
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        const uint32_t slot = i >> 6, owner = i & 63u;
        uint32_t r = rdl(v[0], owner);
#pragma unroll
        for (int j = 1; j < S; ++j) {
            const uint32_t t = rdl(v[j], owner);
            r = (slot == (uint32_t)j) ? t : r;
        }
        return r;
    }
    __device__ __forceinline__ void set(uint32_t i, uint32_t x) {
#pragma unroll
        for (int j = 0; j < S; ++j)
            v[j] = (threadIdx.x + 64u * (uint32_t)j == i) ? x : v[j];
    }
    __device__ __forceinline__ void load(const uint32_t* img, int lane) {
#pragma unroll
        for (int j = 0; j < S; ++j) v[j] = img[lane + 64 * j];
    }
    __device__ __forceinline__ void store(uint32_t* img, int lane) const {
#pragma unroll
        for (int j = 0; j < S; ++j) img[lane + 64 * j] = v[j];
    }
};

// Per-episode counters live in the LDS image and are bumped by lane 0 with
// no-return LDS atomics (ds_add_u32/u64/f32/f64): fire-and-forget, in order
// per wave, and bit-identical to sequential IEEE adds on gfx950 (checked by
// scripts/ubench/lds_fadd.hip) -- no read-modify-write to wait on, no VGPRs.
template <class T>
__device__ __forceinline__ void lds_add(T* p, T v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#define CNT_ADD(S_, field_, v_) \
    do { if ((S_).lane == 0) lds_add(&(S_).c->field_, (decltype((S_).c->field_))(v_)); } while (0)

// register-resident replica state (image order: the fields below, each a
// [64*S] u32 array)
template <int FS, int LS>
struct Regs {
    LA<FS> fk_lo, fk_hi, fk_seq, f_draw;         // flow next event (time, seq) + draw index
    // link times are kept as their low 32 bits: every pending link event is
    // less than 2^31 ns ahead of the clock (checked on the host), so
    // t = now + (uint32)(t_lo - lo32(now)); select_event derives each link's candidate event
    LA<LS> cp_t, cp_seq;                         // tx completion event (valid while busy)
    LA<LS> wh_t, wh_seq;                         // arrival event of the wire head (valid while n_wire > 0)
    LA<LS> p0, p1, p2, qb;                       // head|txp<<16, tail|n_wire<<16, n_queue|busy<<16, queued bytes
    // per TUNNEL t (lane t % 64, slot t / 64; tunnel == link on identity overlays):
    LA<LS> pm_lo, pm_mlo, pm_mhi;                // ping: oldest unacked round, acked bits of rounds lo+1..lo+64
    LA<LS> pm_win;                               // win_n | win_head << 16 | saturated << 31
    LA<LS> pav_lo, pav_hi;                       // ping window mean (double), refreshed per ping-back
    LA<LS> od_lo, od_hi;                         // send time (s) of round lo
    static constexpr int NF = 4, NL = 16;
    static constexpr bool kLazy = true;          // empty-queue transmit completions elided (lazy_resolve)
    static constexpr bool kMem = false;
    // the draw cache's code (flow_next) in the instances of up to 128 flows: larger scenarios
    // have no LDS room for it (GEANT's 506 flows: 4 KB at 8 replicas per CU), and its code cost
    // their register allocation 1.3 % (config 4)
    static constexpr bool kDcache = FS <= 2;
    // not staged: each lane's earliest flow (time, seq, code), refreshed when one of its flows
    // changes (flow_set, ~0.3 per hop) instead of on every event selection (~2.6 per hop)
    int64_t fm_t;
    uint32_t fm_s, fm_c;
};

template <int FS, int LS>
__device__ __forceinline__ void regs_io(Regs<FS, LS>& R, uint32_t* img, int lane, bool store) {
    uint32_t* fb = img;
    uint32_t* lb = img + 4 * 64 * FS;
#define RIO_F(fld, a) if (store) R.fld.store(fb + (a) * 64 * FS, lane); else R.fld.load(fb + (a) * 64 * FS, lane);
#define RIO_L(fld, a) if (store) R.fld.store(lb + (a) * 64 * LS, lane); else R.fld.load(lb + (a) * 64 * LS, lane);
    RIO_F(fk_lo, 0) RIO_F(fk_hi, 1) RIO_F(fk_seq, 2) RIO_F(f_draw, 3)
    RIO_L(wh_t, 0) RIO_L(cp_t, 1) RIO_L(wh_seq, 2)
    RIO_L(cp_seq, 3) RIO_L(p0, 4) RIO_L(p1, 5) RIO_L(p2, 6) RIO_L(qb, 7) RIO_L(pm_lo, 8)
    RIO_L(pm_mlo, 9) RIO_L(pm_mhi, 10) RIO_L(pm_win, 11) RIO_L(pav_lo, 12) RIO_L(pav_hi, 13)
    RIO_L(od_lo, 14) RIO_L(od_hi, 15)
#undef RIO_F
#undef RIO_L
}

// wave-uniform scalar state ("SGPR state"): clock, counters, event sources
struct Hot {
    int64_t  now, ping_t;
    uint32_t ping_seq, seq, uid, dec, ping_rounds, episode;
    uint32_t pend, over, error, stop, hops_launch;
    uint32_t ev_launch;          // events executed in this launch (the running
                                 // totals stay in the LDS header until exit)
    uint32_t cur_seq;            // seq of the event being executed (0 at launch start)
};


// Read-only topology in HBM through the constant address space: every index
// is wave-uniform, so these become s_load through the scalar cache.
#define CAS __attribute__((address_space(4)))
typedef const CAS int32_t c_i32;
typedef const CAS uint32_t c_u32;
typedef const CAS int64_t c_i64;
typedef const CAS double c_f64;
typedef const CAS Layout CLayout;        // scenario constants: s_load, never clobbered

// Scenario constants in one VGPR: lane i holds dword i of the Layout, read
// with v_readlane (25-cycle dependent latency on gfx950, measured by
// scripts/ubench/latency.hip) instead of s_load through the scalar cache
// (60 cycles) -- the compiler re-issued those loads inside the event loop
// because the constants do not fit in SGPRs next to the replica state.
static_assert(offsetof(Layout, mem) == 4 * kLVWords && kLVWords == kWave, "LV covers the first 64 dwords");
struct LV {
    uint32_t w;
    __device__ __forceinline__ void load(const Layout* lay, int lane) {
        w = ((const uint32_t*)lay)[lane];
    }
    __device__ __forceinline__ uint32_t u(int i) const { return (uint32_t)__builtin_amdgcn_readlane((int)w, i); }
    __device__ __forceinline__ int32_t N() const { return (int32_t)u(offsetof(Layout, N) / 4); }
    __device__ __forceinline__ int32_t E() const { return (int32_t)u(offsetof(Layout, E) / 4); }
    __device__ __forceinline__ int32_t L() const { return (int32_t)u(offsetof(Layout, L) / 4); }
    __device__ __forceinline__ int32_t F() const { return (int32_t)u(offsetof(Layout, F) / 4); }
    __device__ __forceinline__ int32_t W() const { return (int32_t)u(offsetof(Layout, W) / 4); }
    __device__ __forceinline__ int32_t max_deg() const { return (int32_t)u(offsetof(Layout, max_deg) / 4); }
    __device__ __forceinline__ int32_t WCAP() const { return (int32_t)u(offsetof(Layout, WCAP) / 4); }
    __device__ __forceinline__ int32_t MA() const { return (int32_t)u(offsetof(Layout, MA) / 4); }
    __device__ __forceinline__ uint32_t topo_bytes() const { return (uint32_t)u(offsetof(Layout, topo_bytes) / 4); }
    __device__ __forceinline__ uint32_t state_bytes() const { return (uint32_t)u(offsetof(Layout, state_bytes) / 4); }
    __device__ __forceinline__ uint32_t lds_bytes() const { return (uint32_t)u(offsetof(Layout, lds_bytes) / 4); }
    __device__ __forceinline__ uint32_t s_dcache() const { return (uint32_t)u(offsetof(Layout, s_dcache) / 4); }
    __device__ __forceinline__ uint32_t s_hdr() const { return (uint32_t)u(offsetof(Layout, s_hdr) / 4); }
    __device__ __forceinline__ uint32_t s_cnt() const { return (uint32_t)u(offsetof(Layout, s_cnt) / 4); }
    __device__ __forceinline__ uint32_t s_obs() const { return (uint32_t)u(offsetof(Layout, s_obs) / 4); }
    __device__ __forceinline__ uint32_t s_wt() const { return (uint32_t)u(offsetof(Layout, s_wt) / 4); }
    __device__ __forceinline__ uint32_t s_wseq() const { return (uint32_t)u(offsetof(Layout, s_wseq) / 4); }
    __device__ __forceinline__ uint32_t s_ring() const { return (uint32_t)u(offsetof(Layout, s_ring) / 4); }
    __device__ __forceinline__ uint32_t s_win() const { return (uint32_t)u(offsetof(Layout, s_win) / 4); }
    __device__ __forceinline__ uint32_t s_pbd() const { return (uint32_t)u(offsetof(Layout, s_pbd) / 4); }
    __device__ __forceinline__ uint32_t s_mlp() const { return (uint32_t)u(offsetof(Layout, s_mlp) / 4); }
    __device__ __forceinline__ int32_t T() const { return (int32_t)u(offsetof(Layout, T) / 4); }
    __device__ __forceinline__ int32_t NO() const { return (int32_t)u(offsetof(Layout, NO) / 4); }
    __device__ __forceinline__ uint32_t tunnels() const { return (uint32_t)u(offsetof(Layout, tunnels) / 4); }
    __device__ __forceinline__ uint32_t PLEN() const { return (uint32_t)u(offsetof(Layout, PLEN) / 4); }
    __device__ __forceinline__ uint32_t ring_total() const { return (uint32_t)u(offsetof(Layout, ring_total) / 4); }
    __device__ __forceinline__ uint32_t lds_state_bytes() const { return (uint32_t)u(offsetof(Layout, lds_state_bytes) / 4); }
    __device__ __forceinline__ uint32_t s_regs() const { return (uint32_t)u(offsetof(Layout, s_regs) / 4); }
    __device__ __forceinline__ uint32_t PBK() const { return (uint32_t)u(offsetof(Layout, PBK) / 4); }
    __device__ __forceinline__ int32_t FS() const { return (int32_t)u(offsetof(Layout, FS) / 4); }
    __device__ __forceinline__ int32_t LS() const { return (int32_t)u(offsetof(Layout, LS) / 4); }
    __device__ __forceinline__ int64_t sw_txd() const { return mk64(u(offsetof(Layout, sw_txd) / 4), u(offsetof(Layout, sw_txd) / 4 + 1)); }
    __device__ __forceinline__ int64_t sw_txp() const { return mk64(u(offsetof(Layout, sw_txp) / 4), u(offsetof(Layout, sw_txp) / 4 + 1)); }
    __device__ __forceinline__ int64_t sw_txe() const { return mk64(u(offsetof(Layout, sw_txe) / 4), u(offsetof(Layout, sw_txe) / 4 + 1)); }
    __device__ __forceinline__ int64_t sw_prop() const { return mk64(u(offsetof(Layout, sw_prop) / 4), u(offsetof(Layout, sw_prop) / 4 + 1)); }
    __device__ __forceinline__ uint32_t qcap_s() const { return (uint32_t)u(offsetof(Layout, qcap_s) / 4); }
    __device__ __forceinline__ uint32_t qcap_a() const { return (uint32_t)u(offsetof(Layout, qcap_a) / 4); }
    __device__ __forceinline__ uint32_t qmax_bytes() const { return (uint32_t)u(offsetof(Layout, qmax_bytes) / 4); }
    __device__ __forceinline__ uint32_t acc_qmax_pkts() const { return (uint32_t)u(offsetof(Layout, acc_qmax_pkts) / 4); }
    __device__ __forceinline__ int64_t t_end() const { return mk64(u(offsetof(Layout, t_end) / 4), u(offsetof(Layout, t_end) / 4 + 1)); }
    __device__ __forceinline__ int64_t ping_period() const { return mk64(u(offsetof(Layout, ping_period) / 4), u(offsetof(Layout, ping_period) / 4 + 1)); }
    __device__ __forceinline__ uint32_t data_size() const { return (uint32_t)u(offsetof(Layout, data_size) / 4); }
    __device__ __forceinline__ uint32_t ping_size() const { return (uint32_t)u(offsetof(Layout, ping_size) / 4); }
    __device__ __forceinline__ uint32_t echo_size() const { return (uint32_t)u(offsetof(Layout, echo_size) / 4); }
    __device__ __forceinline__ uint32_t ma() const { return (uint32_t)u(offsetof(Layout, ma) / 4); }
    __device__ __forceinline__ uint32_t ping_as_obs() const { return (uint32_t)u(offsetof(Layout, ping_as_obs) / 4); }
    __device__ __forceinline__ uint32_t auto_reset() const { return (uint32_t)u(offsetof(Layout, auto_reset) / 4); }
    __device__ __forceinline__ uint32_t notify_dest() const { return (uint32_t)u(offsetof(Layout, notify_dest) / 4); }
    __device__ __forceinline__ uint32_t train() const { return (uint32_t)u(offsetof(Layout, train) / 4); }
    __device__ __forceinline__ uint32_t seed_lo() const { return (uint32_t)u(offsetof(Layout, seed_lo) / 4); }
    __device__ __forceinline__ uint32_t replica_base() const { return (uint32_t)u(offsetof(Layout, replica_base) / 4); }
    __device__ __forceinline__ uint32_t log_cap() const { return (uint32_t)u(offsetof(Layout, log_cap) / 4); }
    __device__ __forceinline__ uint32_t rec_bytes() const { return (uint32_t)u(offsetof(Layout, rec_bytes) / 4); }
    __device__ __forceinline__ double loss_penalty() const { return __longlong_as_double(mk64(u(offsetof(Layout, loss_penalty) / 4), u(offsetof(Layout, loss_penalty) / 4 + 1))); }
    __device__ __forceinline__ float loss_penalty_f() const { return __uint_as_float(u(offsetof(Layout, loss_penalty_f) / 4)); }
    __device__ __forceinline__ uint32_t rng_mode() const { return (uint32_t)u(offsetof(Layout, rng_mode) / 4); }
};


// LDS views of one replica + its topology
struct Sim {
    LV lv;                                  // scenario constants (one VGPR)
    unsigned char* base;
    Hdr* h;
    prisma_counters_t* c;
    uint32_t* obs;
    uint32_t* wt; uint32_t* wseq;           // wire: arrival time (low 32 bits) and seq
    uint32_t* went;                         // tunnelled overlays: wire packet entries (LDS)
    uint32_t* qwin;                         // ... and the FIFO windows of relay_ip kernels (LDS, q_put)
    uint32_t* ring;                         // link FIFOs: LDS, or HBM (tunnelled / memory-resident)
    float* win;
    float* pbd;                             // ping-back delays [responder slot][PBK]
    const CAS TopoImage* T;                 // topology (scalar loads at fixed offsets)
    const uint8_t* table;                   // action table in LDS (register engine, table_in_lds)
    const uint8_t* table_g;                 // ... or in HBM (memory-resident engine, or not in LDS)
    bool tab_lds;
    const float* mlp;                       // DQN-buffer weights (HBM) or null
    const float* mlp_rp;                    // layers 2-4 interleaved by 4 inputs (mlp_repack)
    float* hbuf;                            // 64 floats of LDS: a layer's activations
    unsigned char* logrep;
    uint32_t gid;
    int lane;
    uint32_t m1, m2, m4, m8;                // per-lane word masks -(lane & 1), -(lane>>1 & 1), -(lane>>2 & 1), -(lane < 8)
    bool tun;                               // tunnelled overlay: a compile-time constant in the
                                            // step kernels (template TUN), folded after inlining
    bool mem;                               // memory-resident engine (compile-time constant, folded)
    bool ctrl;                              // --train echo / notify_dest paths compiled in (constant)
    bool mlp_inst;                          // an in-kernel MLP instance (event_loop's MLP, constant)
    bool lanel;                             // lane-resident link handlers (lane_links_bind; constant)
    // ... and their per-lane constants of link `lane`: ring offset | capacity << 16, tx time of a
    // data / ping entry and the propagation delay (low 32 bits), the admission limit (bytes on a
    // switch link, packets on an access link) and the topology word (access flag on top, the far
    // end, its row pointer and degree below: lane_links_bind)
    uint32_t lk_rinfo, lk_txd, lk_txp, lk_prop, lk_lim, lk_acc;
    // memory-resident engine: variable-size topology arrays (scalar loads)
    const CAS int32_t* m_rowptr;
    const CAS int32_t* m_ldst;
    const CAS int32_t* m_lrev;
    const CAS int64_t* m_acctx;
    const CAS int32_t* m_fsrc;
    const CAS int32_t* m_fdst;
    const CAS double* m_fmean;
    const CAS uint32_t* m_esz;              // ... and the signalling arrays of the --train instances
    const CAS uint32_t* m_etx;
    const CAS uint32_t* m_abtx;
    const CAS uint32_t* m_bpair;
    const CAS uint32_t* m_fseq;
    const CAS BigSig* m_bs;
    uint32_t* lrec;                         // link records [L][kLRec] (HBM)
    // issue priority by launch progress (prio_update): hops of the whole launch (0: off), hops done
    // before this event loop, the loop's hop count at which the priority next changes, and the
    // launch's chunk shift (prio_ladder_shift(prio_total), set with prio_total)
    uint32_t prio_total, prio_base, prio_next, prio_shift;
#if PRISMA_TIMING
    mutable uint64_t tsub[2], tlast;             // sub-phase cycles inside apply_decision
    mutable uint64_t tmlp[4];                    // mlp_action phases (timing build)
    mutable uint64_t tflow[4], tfl;              // memory-resident on_flow phases (timing build)
    mutable uint64_t tp[16], tpl;                // fine probes TP(i) (timing build)
    mutable uint32_t tpn[16];
#endif
};

__device__ inline void sim_bind(Sim& S, const LV& L, unsigned char* lds, const unsigned char* topo,
                                unsigned char* logrep, uint32_t gid, int lane) {
    S.lv = L;
    S.base = lds;
    S.h = (Hdr*)(lds + kOffHdr);                // fixed offsets (asserted in build_layout)
    S.c = (prisma_counters_t*)(lds + kOffCnt);
    S.obs = (uint32_t*)(lds + kOffObs);
    S.wt = (uint32_t*)(lds + L.s_wt());
    S.wseq = (uint32_t*)(lds + L.s_wseq());
    S.went = S.wseq + (uint32_t)L.L() * (uint32_t)L.WCAP();
    S.qwin = S.went + (uint32_t)L.L() * (uint32_t)L.WCAP();
    S.ring = (uint32_t*)(lds + L.s_ring());
    S.win = (float*)(lds + L.s_win());
    S.pbd = (float*)(lds + L.s_pbd());
    S.T = (const CAS TopoImage*)topo;
    S.table = (const uint8_t*)(lds + L.lds_state_bytes());
    S.table_g = nullptr;
    S.tab_lds = true;
    S.hbuf = (float*)(lds + L.s_mlp());
    S.mlp = nullptr;
    S.mlp_rp = nullptr;
    S.logrep = logrep;
    S.gid = gid;
    S.lane = lane;
    // opaque to the optimiser, so write_record's selects stay bitfield inserts on VGPR masks
    // instead of loop-invariant lane-compare SGPR pairs (which the headline kernel spilled)
    S.m1 = 0u - ((uint32_t)lane & 1u);
    S.m2 = 0u - (((uint32_t)lane >> 1) & 1u);
    S.m4 = 0u - (((uint32_t)lane >> 2) & 1u);
    S.m8 = lane < 8 ? ~0u : 0u;
    asm volatile("" : "+v"(S.m1), "+v"(S.m2), "+v"(S.m4), "+v"(S.m8));
    S.tun = L.tunnels() != 0u;
    S.mem = false;
    S.ctrl = true;
    S.mlp_inst = false;
    S.lanel = false;
    S.lk_rinfo = 0; S.lk_txd = 0; S.lk_txp = 0; S.lk_prop = 0; S.lk_lim = 0; S.lk_acc = 0;
    S.lrec = nullptr;
    S.prio_total = 0; S.prio_base = 0; S.prio_next = kPrioNever; S.prio_shift = 31u;
}

// Issue priority by launch progress.  A SIMD arbitrates its waves' issue by priority, then age
// (MI355X_MICROARCH.md, two waves per SIMD), so at equal priority the oldest of a SIMD's 4
// replicas runs ahead and the youngest finishes alone: measured on the headline
// (scripts/wave_times.py), the 4 waves of a SIMD ended at about 89, 113, 124 and 146 ms of a
// 146-ms launch, the last ~22 ms with one wave left to hide its own latency.  Here a wave's priority
// follows the share of the launch's hops it has done, so a wave that is ahead yields issue to the
// ones behind it and the SIMD keeps all four to the end.  The level and the next boundary come
// from prio_ladder.h (plain C++, tested on the CPU): the fixed thresholds 5/8, 13/16, 15/16
// (3, 2, 1, then 0) and / or chunks of T / PRISMA_PRIO_CHUNKS hops whose level steps down and wraps,
// which keep correcting to the launch's end.  Build switches, for A/B variants
// (scripts/build_variant.sh <name> -DPRISMA_PRIO_CHUNKS=128 -DPRISMA_PRIO_HYBRID_FROM=0):
//   PRISMA_PRIO_HYBRID_FROM  how many of the fixed thresholds hold before the chunks take over
//                            (0: chunks from the first hop, the cyclic ladder; 4: thresholds only)
//   PRISMA_PRIO_CHUNKS       chunk count of the launch (power of two)
// The shipped defaults are the winners of profiles/prio_ladder/ab_sweep.txt.
// (round-6 A/B on one box, profiles/r06_ab/ab_prio.txt: thresholds 5/8, 13/16, 15/16 +13.4 % at
// the headline and +8.9 % at config 3; 1/2, 3/4, 7/8 +13.2 %; 1/4, 1/2, 3/4 +10 %;
// 7/8, 15/16, 31/32 +4.5 %; a least-progress-first rank over the SIMD's four waves, exchanged
// through global memory every 64 or 256 hops, -2 %)
// hops_loop: the hops of this event loop; S.prio_base those of the launch before it (the second
// loop after spare_restart), so the level is that of the launch's progress wherever the loop
// stands -- also when finish_pending stepped over a boundary -- and S.prio_next is loop-local.
__device__ __forceinline__ void prio_update(Sim& S, uint32_t hops_loop) {
    // the instances without the ladder (prio_total a constant 0): nothing, so the event loop's test
    // folds away with it -- the opaque T below would otherwise keep the ladder's code in them
    if (__builtin_constant_p(S.prio_total) && S.prio_total == 0u) return;
    // (the launch's progress is the same in every lane, but prio_base -- the restart loop's hops
    // done -- lives in a VGPR: the whole sum goes through readfirstlane, so in both event-loop
    // copies the ladder is scalar arithmetic and scalar branches.  As lane values the switch became
    // exec-masked regions, and s_setprio, which ignores exec, ran in every one of them.)
    // T opaque here: the thresholds are then derived in this rarely-run block instead of being
    // hoisted out of the event loop, where each would hold (and spill) an SGPR for the whole launch
    uint32_t T = S.prio_total;
    asm volatile("" : "+s"(T));
    const PrioStep st = prio_ladder(T, S.prio_shift, rfl(S.prio_base + hops_loop));
    switch (st.level) {                              // (s_setprio takes an immediate)
    case 3u: __builtin_amdgcn_s_setprio(3); break;
    case 2u: __builtin_amdgcn_s_setprio(2); break;
    case 1u: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(0); break;
    }
    S.prio_next = prio_ladder_local(st.next, S.prio_base);
}

// Topology reads.  The register-resident engine reads the fixed-offset TopoImage,
// the memory-resident one its variable-size arrays; S.mem is a compile-time
// constant in every kernel, so each accessor folds to one scalar load.
__device__ __forceinline__ int32_t t_ovrow(const Sim& S, uint32_t u) { return S.mem ? S.m_rowptr[u] : S.T->ovrow[u]; }
__device__ __forceinline__ int32_t t_ldst(const Sim& S, uint32_t l) { return S.mem ? S.m_ldst[l] : S.T->ldst[l]; }
__device__ __forceinline__ int32_t t_lrev(const Sim& S, uint32_t l) { return S.mem ? S.m_lrev[l] : S.T->lrev[l]; }
__device__ __forceinline__ int64_t t_acctx(const Sim& S, uint32_t u) { return S.mem ? S.m_acctx[u] : S.T->acctx[u]; }
__device__ __forceinline__ int32_t t_fsrc(const Sim& S, uint32_t f) { return S.mem ? S.m_fsrc[f] : S.T->fsrc[f]; }
__device__ __forceinline__ int32_t t_fdst(const Sim& S, uint32_t f) { return S.mem ? S.m_fdst[f] : S.T->fdst[f]; }
__device__ __forceinline__ double t_fmean(const Sim& S, uint32_t f) { return S.mem ? S.m_fmean[f] : S.T->fmean[f]; }
__device__ __forceinline__ uint32_t t_esz(const Sim& S, uint32_t l) { return S.mem ? S.m_esz[l] : S.T->esz[l]; }
__device__ __forceinline__ uint32_t t_etx(const Sim& S, uint32_t l) { return S.mem ? S.m_etx[l] : S.T->etx[l]; }
__device__ __forceinline__ uint32_t t_abtx(const Sim& S, uint32_t u) { return S.mem ? S.m_abtx[u] : S.T->abtx[u]; }
__device__ __forceinline__ uint32_t t_bpair(const Sim& S, uint32_t g) { return S.mem ? S.m_bpair[g] : S.T->bpair[g]; }
__device__ __forceinline__ uint32_t t_fseq(const Sim& S, uint32_t f) { return S.mem ? S.m_fseq[f] : S.T->fseq[f]; }
__device__ __forceinline__ uint32_t t_ngen(const Sim& S) { return S.mem ? S.m_bs->n_gen : S.T->n_bsig; }
__device__ __forceinline__ uint32_t t_bs_nseg(const Sim& S) { return S.mem ? S.m_bs->nseg : S.T->bs_nseg; }
__device__ __forceinline__ uint32_t t_bs_size(const Sim& S) { return S.mem ? S.m_bs->size : S.T->bs_size; }
__device__ __forceinline__ int64_t t_bs_period(const Sim& S) { return S.mem ? S.m_bs->period : S.T->bs_period; }

// A store to replica state that every lane may read back, by every lane (same address, same
// value): no exec-mask juggling in LDS, and in HBM each lane's later read of the address is
// ordered after its own store.
template <class T>
__device__ __forceinline__ void st_rep(const Sim& S, T* p, T v) {
    *p = v;
}

// A FIFO entry, written by every lane (same address, same value).  Identity overlays of the
// register-resident engine keep the rings in LDS, where an all-lane store needs no exec-mask
// juggling (A/B +1 % against lane 0 only); tunnelled overlays and the memory-resident engine
// keep them in the HBM state image (their arrivals read the packet from the wire slot, so only
// a dequeue behind a busy transmitter reads the ring back).
__device__ __forceinline__ void ring_put(const Sim& S, uint32_t i, uint32_t e) {
    S.ring[i] = e;
}

// Relay entries carry (decision, live TTL, tunnel target) -- rip_make, engine_layout.h -- in the
// register-resident engine's tunnelled-overlay kernels without the --train / notify_dest paths
// (a compile-time constant): a switch inside a tunnel forwards a data packet on its entry alone,
// as IpForward does on the IP header (ipv4-l3-protocol.cc IpForward), instead of reading the
// deciding node, action and TTL back from the decision record in HBM.
__device__ __forceinline__ bool relay_ip(const Sim& S) { return S.tun && !S.mem && !S.ctrl; }

// The same kernels keep the first kQWin packets queued behind each link's busy transmitter -- the
// ones its next completions dequeue -- in an LDS window, slot = ring index mod kQWin, stored
// complemented (0 = empty; none of these kernels' entries is all ones); a packet with kQWin or
// more queued ahead of it goes to the HBM ring.  A dequeue finds the queue head in its window slot
// iff it was stored there: any later packet for that slot would have had kQWin packets ahead of it
// (ring capacities are multiples of kQWin, so indices stay consecutive across the wrap).  Their
// FIFOs had read every dequeued packet back from HBM, most of the time after the line had left L2.
__device__ __forceinline__ void q_put(const Sim& S, uint32_t l, uint32_t off, uint32_t idx, uint32_t ahead,
                                      uint32_t e) {
    if (relay_ip(S) && ahead < kQWin) S.qwin[l * kQWin + (idx & (kQWin - 1u))] = ~e;
    else ring_put(S, off + idx, e);
}
__device__ __forceinline__ uint32_t q_take(const Sim& S, uint32_t l, uint32_t off, uint32_t idx) {
    if (relay_ip(S)) {
        uint32_t* w = &S.qwin[l * kQWin + (idx & (kQWin - 1u))];
        const uint32_t v = rfl(*w);
        if (v != 0u) { *w = 0u; return ~v; }
    }
    return rfl(S.ring[off + idx]);
}

// uniform LDS reads (every lane reads the same address: broadcast, no conflict)
__device__ __forceinline__ uint32_t u_ld32(const uint32_t* p) { return rfl(*p); }
__device__ __forceinline__ int32_t u_ldi(const int32_t* p) { return (int32_t)rfl((uint32_t)*p); }
__device__ __forceinline__ int64_t u_ld64(const int64_t* p) {
    int64_t v = *p;
    return mk64(rfl(lo32(v)), rfl(hi32(v)));
}
__device__ __forceinline__ double u_ldd(const double* p) {
    double v = *p;
    uint64_t b = __double_as_longlong(v);
    return __longlong_as_double((long long)(((uint64_t)rfl((uint32_t)(b >> 32)) << 32) | rfl((uint32_t)b)));
}

__device__ inline void hot_load(const Sim& S, Hot& H) {
    const Hdr& h = *S.h;
    H.now = u_ld64(&h.now); H.ping_t = u_ld64(&h.ping_t);
    H.ping_seq = u_ld32(&h.ping_seq); H.seq = u_ld32(&h.seq); H.uid = u_ld32(&h.uid);
    H.dec = u_ld32(&h.dec_count); H.ping_rounds = u_ld32(&h.ping_rounds); H.episode = u_ld32(&h.episode);
    H.pend = u_ld32(&h.pend); H.over = u_ld32(&h.over); H.error = u_ld32(&h.error);
    H.stop = u_ld32(&h.stop); H.hops_launch = u_ld32(&h.hops_launch);
    H.ev_launch = 0;
    H.cur_seq = 0;
}

template <class RS>
__device__ inline void hot_store(Sim& S, const RS& R, const Hot& H) {
    if (S.lane == 0) {
        Hdr& h = *S.h;
        h.now = H.now; h.ping_t = H.ping_t; h.ping_seq = H.ping_seq; h.seq = H.seq; h.uid = H.uid;
        h.dec_count = H.dec; h.ping_rounds = H.ping_rounds; h.episode = H.episode; h.pend = H.pend;
        h.over = H.over; h.error = H.error; h.stop = H.stop; h.hops_launch = H.hops_launch;
        h.hops_total += H.hops_launch; h.events_total += H.ev_launch;
        prisma_counters_t& c = *S.c;
        c.now_ns = H.now; c.episode = H.episode; c.ping_rounds = H.ping_rounds; c.seq = H.seq; c.uid = H.uid;
        c.dec_count = H.dec; c.error = H.error; c.episode_over = H.over;
        c.hops_total = h.hops_total; c.events_total = h.events_total;
        c.events += H.ev_launch;
    }
}

__device__ __forceinline__ void fail(Hot& H, uint32_t bit) {
    H.error |= bit;
    H.over = 1;
    H.stop = 1;
}

__device__ __forceinline__ bool key_less(int64_t t, uint32_t s, int64_t bt, uint32_t bs) {
    return t < bt || (t == bt && s < bs);
}

// size on the wire of entry x on link l.  The --train instances read an echo's size per
// link (its sender's payload with signalling type "NN" or "target", sim.cc:373-392) and
// know the big-signalling segment; the other instances never see either.
__device__ __forceinline__ uint32_t ent_size(const Sim& S, uint32_t x, uint32_t l) {
    const LV& L = S.lv;
    if (S.ctrl) {
        if (ent_is_echo(x)) return t_esz(S, l);
        if (ent_is_big(x)) return t_bs_size(S);
    }
    return ent_is_data(x) ? L.data_size() : (ent_is_echo(x) ? L.echo_size() : L.ping_size());
}
// whole seconds of a (non-negative) time, on the vector unit (numerics.h div_1e9)
#define TSEC(t) div_1e9((uint64_t)(t))
// class of entry x (type | echo bit << 2): index of TopoImage::ctx
__device__ __forceinline__ uint32_t ent_cls(uint32_t x) { return (x & 3u) | ((x >> 29) & 4u); }
// FIFO ring of link l: uniform capacities on identity overlays, per-link (sized by the
// control traffic crossing each link) on tunnelled ones.  The register-resident engine
// reads (offset | capacity << 16) from the topology image: one scalar load instead of the
// scalar arithmetic on scenario constants (A/B: +3.7 % at the headline)
__device__ __forceinline__ uint32_t ring_off(const Sim& S, uint32_t l) {
    const LV& L = S.lv;
    if (!S.mem) return S.T->rinfo[l] & 0xffffu;
    return l < (uint32_t)L.E() ? l * L.qcap_s() : (uint32_t)L.E() * L.qcap_s() + (l - (uint32_t)L.E()) * L.qcap_a();
}
__device__ __forceinline__ uint32_t ring_cap(const Sim& S, uint32_t l) {
    const LV& L = S.lv;
    if (!S.mem) return S.T->rinfo[l] >> 16;
    return l < (uint32_t)L.E() ? L.qcap_s() : L.qcap_a();
}

// one link's fields as uniform scalars
struct LinkV {
    uint32_t head, txp, tail, n_wire, n_queue, busy, qb;
    uint32_t cp_t, cp_seq;       // completion time (low 32 bits), seq
    uint32_t wh_t, wh_seq;       // wire-head arrival time (low 32 bits), seq
    uint32_t rec;                // memory-resident engine: the link's record, lane j = word j
};

template <int FS, int LS>
__device__ __forceinline__ LinkV link_get(const Regs<FS, LS>& R, uint32_t l) {
    LinkV k;
    uint32_t a = R.p0.get(l), b = R.p1.get(l), c = R.p2.get(l);
    k.head = a & 0xffffu; k.txp = a >> 16;
    k.tail = b & 0xffffu; k.n_wire = b >> 16;
    k.n_queue = c & 0xffffu; k.busy = c >> 16;
    k.qb = R.qb.get(l);
    k.cp_t = R.cp_t.get(l);
    k.cp_seq = R.cp_seq.get(l);
    k.wh_t = R.wh_t.get(l);
    k.wh_seq = R.wh_seq.get(l);
    return k;
}

// write back a link's fields and recompute its candidate key (registers only:
// the wire head's key is cached in wh_t / wh_seq)
// fields a link write-back stores: all, or (wire_pop) only the head, wire count and head key --
// the readlanes of the fields it leaves alone are then dead code
constexpr unsigned LP_ALL = 0u, LP_WIRE = 1u;
template <unsigned MASK = LP_ALL, int FS, int LS>
__device__ __forceinline__ void link_put(const Sim& S, Regs<FS, LS>& R, const Hot& H, uint32_t l, const LinkV& k) {
    R.p0.set(l, k.head | (k.txp << 16));
    R.p1.set(l, k.tail | (k.n_wire << 16));
    if (MASK == LP_ALL) {
        R.p2.set(l, k.n_queue | (k.busy << 16));
        R.qb.set(l, k.qb);
        R.cp_t.set(l, k.cp_t);
        R.cp_seq.set(l, k.cp_seq);
    }
    R.wh_t.set(l, k.wh_t);
    R.wh_seq.set(l, k.wh_seq);
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t v);
__device__ __forceinline__ uint32_t wave_umin_fast(uint32_t v);
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v);

// Elided completions.  A transmit completion that finds its queue empty only clears
// `busy` (point-to-point-net-device.cc:305-336: TransmitComplete with no packet left
// schedules nothing and consumes no event uid), so the register-resident engine keeps it
// out of the event set (link_put) and settles it lazily: in link_send when the link is used
// again, and for every link at once when a launch stops (lazy_resolve).  Settling counts the
// event the reference executed (events / events_total), so every counter equals the eager
// schedule's.  Whether an elided completion precedes the event being executed (now,
// cur_seq): if the wire is empty, the transmitted packet's arrival -- scheduled after its
// completion -- has run, so the completion has too; otherwise that arrival is still ahead,
// so the completion lies within one propagation delay before the clock or one transmission
// after it (< 2^31 ns, checked on the host) and its 32-bit time offset is exact.
__device__ __forceinline__ bool lazy_due(uint32_t n_wire, uint32_t cp_t, uint32_t cp_seq, const Hot& H) {
    // (dt, cp_seq) < (0, cur_seq) with dt = cp_t - lo32(now) as a signed 32-bit offset: the sign
    // of dt * 2^32 + cp_seq - cur_seq, one 64-bit subtraction (|dt| < 2^31 whenever the wire holds
    // a packet, so the difference does not wrap; with an empty wire it is not consulted)
    const uint64_t d = ((uint64_t)(cp_t - lo32(H.now)) << 32) + (uint64_t)cp_seq - (uint64_t)H.cur_seq;
    return n_wire == 0u || (int64_t)d < 0;
}

// Settle every elided completion that precedes the current event, or -- at the end of an
// episode -- every one before simTime, moving the clock to the latest of them
// (Simulator::Stop runs every event < simTime).
template <int FS, int LS>
__device__ __forceinline__ void lazy_resolve(const Sim& S, Regs<FS, LS>& R, Hot& H, bool episode_end) {
    const LV& L = S.lv;
    const uint32_t n0 = lo32(H.now);
    const int64_t t_end = L.t_end();
    uint32_t n = 0;
    int64_t tmax = H.now;
#pragma unroll
    for (int j = 0; j < LS; ++j) {
        const uint32_t p1 = R.p1.v[j], p2 = R.p2.v[j];
        const int32_t dt = (int32_t)(R.cp_t.v[j] - n0);
        const int64_t t = H.now + (int64_t)dt;
        const bool lazy = (p2 >> 16) != 0u && (p2 & 0xffffu) == 0u;
        const bool due = lazy && (episode_end ? ((p1 >> 16) == 0u || t < t_end)
                                              : lazy_due(p1 >> 16, R.cp_t.v[j], R.cp_seq.v[j], H));
        R.p2.v[j] = due ? (p2 & 0xffffu) : p2;
        if (due && (p1 >> 16) != 0u && t > tmax) tmax = t;
        n += (uint32_t)__builtin_popcountll(__ballot(due));
    }
    H.ev_launch += n;
    if (episode_end && n) {
        const int64_t m = -wave_min_i64(-tmax);          // times are >= 0
        if (m > H.now) H.now = m;
    }
}

// flow f's next send: time, seq, draw index of that send
template <int FS, int LS>
__device__ __forceinline__ uint32_t flow_draw(const Sim& S, const Regs<FS, LS>& R, uint32_t f) {
    return R.f_draw.get(f);
}
template <int FS, int LS>
__device__ __forceinline__ void flow_min_refresh(const Sim& S, Regs<FS, LS>& R, const Hot& H) {
    int64_t ft = INT64_MAX;
    uint32_t s = 0xffffffffu, c = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < FS; ++j) {
        const int64_t tj = mk64(R.fk_lo.v[j], R.fk_hi.v[j]);
        const uint32_t sj = R.fk_seq.v[j];
        if (key_less(tj, sj, ft, s)) { ft = tj; s = sj; c = (K_FLOW << 28) | (uint32_t)(S.lane + 64 * j); }
    }
    // the ping timer competes in lane 0 (refreshed when a round re-arms it)
    if (S.lane == 0 && key_less(H.ping_t, H.ping_seq, ft, s)) { ft = H.ping_t; s = H.ping_seq; c = K_PING << 28; }
    R.fm_t = ft; R.fm_s = s; R.fm_c = c;
}
template <int FS, int LS>
__device__ __forceinline__ void flow_set(const Sim& S, Regs<FS, LS>& R, const Hot& H, uint32_t f, int64_t t,
                                         uint32_t seq, uint32_t draw) {
    R.fk_lo.set(f, lo32(t));
    R.fk_hi.set(f, hi32(t));
    R.fk_seq.set(f, seq);
    R.f_draw.set(f, draw);
    flow_min_refresh(S, R, H);
}

// ping state of tunnel t (ping_ack): oldest unacked round, acked mask, window
// state; the window mean and round lo's send time are written back only
struct PingV { uint32_t lo, mlo, mhi, win; };
template <int FS, int LS>
__device__ __forceinline__ PingV ping_get(const Sim& S, const Regs<FS, LS>& R, uint32_t t) {
    PingV p;
    p.lo = R.pm_lo.get(t); p.mlo = R.pm_mlo.get(t); p.mhi = R.pm_mhi.get(t); p.win = R.pm_win.get(t);
    return p;
}
template <int FS, int LS>
__device__ __forceinline__ void ping_set_lo(const Sim& S, Regs<FS, LS>& R, uint32_t t, uint32_t lo, uint64_t od) {
    R.pm_lo.set(t, lo);
    R.od_lo.set(t, (uint32_t)od);
    R.od_hi.set(t, (uint32_t)(od >> 32));
}
template <int FS, int LS>
__device__ __forceinline__ void ping_set_mask(const Sim& S, Regs<FS, LS>& R, uint32_t t, uint64_t mask) {
    R.pm_mlo.set(t, (uint32_t)mask);
    R.pm_mhi.set(t, (uint32_t)(mask >> 32));
}
template <int FS, int LS>
__device__ __forceinline__ void ping_set_win(const Sim& S, Regs<FS, LS>& R, uint32_t t, uint32_t win, uint64_t avg) {
    R.pm_win.set(t, win);
    R.pav_lo.set(t, (uint32_t)avg);
    R.pav_hi.set(t, (uint32_t)(avg >> 32));
}

// Wire slot i of link l: arrival time (low 32 bits), seq and -- memory-resident
// engine -- the packet entry.  Register-resident: LDS arrays; memory-resident: words
// LR_WT + {i, WCAP + i, 2 WCAP + i} of the link record held in k.rec (written back by
// link_put), so an arrival reads its packet without a ring access.
__device__ __forceinline__ void wire_set(const Sim& S, LinkV& k, uint32_t l, uint32_t i, uint32_t t, uint32_t s,
                                         uint32_t x) {
    const uint32_t W = (uint32_t)S.lv.WCAP();
    if (S.mem) {
        const uint32_t j = (uint32_t)S.lane;
        k.rec = j == LR_WT + i ? t : (j == LR_WT + W + i ? s : (j == LR_WT + 2u * W + i ? x : k.rec));
    } else {                                  // every lane stores the same value to the same address:
        S.wt[l * W + i] = t;                  // no exec-mask juggling (A/B +1 % against lane 0 only)
        S.wseq[l * W + i] = s;
        if (S.tun) S.went[l * W + i] = x;
    }
}
__device__ __forceinline__ void wire_get(const Sim& S, const LinkV& k, uint32_t l, uint32_t i, uint32_t& t,
                                         uint32_t& s) {
    const uint32_t W = (uint32_t)S.lv.WCAP();
    if (S.mem) {
        t = rdl(k.rec, LR_WT + i);
        s = rdl(k.rec, LR_WT + W + i);
    } else {
        t = u_ld32(S.wt + l * W + i);
        s = u_ld32(S.wseq + l * W + i);
    }
}
__device__ __forceinline__ uint32_t wire_ent(const Sim& S, const LinkV& k, uint32_t i) {
    return rdl(k.rec, LR_WT + 2u * (uint32_t)S.lv.WCAP() + i);
}

// ---- link FIFO / transmitter (point-to-point-net-device.cc:273-336, 595-666)
__device__ __forceinline__ void transmit_start(const Sim& S, Hot& H, uint32_t l, LinkV& k, uint32_t ring_idx,
                                               uint32_t x) {
    const LV& L = S.lv;
    const bool sw = l < (uint32_t)L.E();
    x = rfl(x);                  // uniform entry: its class indexes the topology image with a scalar load
    // register-resident engine: a switch link's tx time by entry class from the topology image
    // (--train instances: an echo's by link, sized by its sender)
    // (memory-resident: by entry type from the scenario constants; --train instances: echoes by
    // link, big-signalling segments from the BigSig header)
    uint32_t at;
    k.busy = 1;
    if (S.mem) {
        int64_t tx = sw ? ((S.ctrl && ent_is_echo(x)) ? (int64_t)t_etx(S, l)
                           : ((S.ctrl && ent_is_big(x)) ? (int64_t)S.m_bs->tx_sw
                              : (ent_is_data(x) ? L.sw_txd() : (ent_is_echo(x) ? L.sw_txe() : L.sw_txp()))))
                        : ((S.ctrl && ent_is_big(x)) ? (int64_t)t_abtx(S, l - (uint32_t)L.E())
                                                     : t_acctx(S, l - (uint32_t)L.E()));
        int64_t prop = sw ? L.sw_prop() : 0;
        k.cp_t = lo32(H.now + tx);
        at = lo32(H.now + tx + prop);
    } else {
        // register-resident engine: (tx, tx + propagation) of link l for the entry's class, low 32
        // bits, one scalar load from the topology image (TopoImage::ltx) -- the switch/access
        // selects, the 64-bit adds and the second load are the host's
        const uint32_t i = 2u * (l * 8u + ent_cls(x));
        k.cp_t = lo32(H.now) + S.T->ltx[i];
        at = lo32(H.now) + S.T->ltx[i + 1u];
    }
    k.cp_seq = H.seq++;                                        // TransmitComplete
    const uint32_t w = ring_idx & (uint32_t)(L.WCAP() - 1);
    const uint32_t as = H.seq++;                               // channel Receive
    wire_set(S, k, l, w, at, as, x);
    if (k.n_wire == 1) { k.wh_t = at; k.wh_seq = as; }        // the wire was empty: new head
    if (k.n_wire > (uint32_t)L.WCAP()) fail(H, PRISMA_EBIT_WIRE);
}

// Whether a send must store its packet in the link's FIFO ring.  Tunnelled overlays and the
// memory-resident engine keep the packets on a wire in wire slots (LDS / the link record), so a
// packet that finds the transmitter idle and nothing queued goes straight onto the wire and its
// ring slot is never read: the store -- an HBM write there -- is skipped.  The
// register-resident identity overlays read arrivals from the ring and always store.
__device__ __forceinline__ bool ring_store_needed(const Sim& S, const LinkV& k) {
    if (S.tun || S.mem) return k.busy || k.n_queue != 0u;
    return true;
}

// ---- lane-resident link handlers (register-resident engine, LS = 1: link l lives in lane l)
// The handlers below pull one link's fields out of their lane with ~8 v_readlane, run the FIFO
// and transmitter arithmetic on the scalar unit -- with two dependent scalar loads (rinfo, ltx)
// -- and write the fields back through 8 compare/selects.  At 4 waves per SIMD the headline is
// bound by instruction issue with the scalar unit the busy side (one per CU against four SIMDs;
// DESIGN.md §9), so the instances with S.lanel run the same arithmetic in the fields' own lane
// instead: every lane computes the update of ITS link as if the packet were sent on it, and
// only the owner lane (lane == l) commits.  The per-link constants sit in VGPRs, loaded once
// before the event loop (lane_links_bind) and opaque to the optimiser, so no handler loads a
// constant.  What stays scalar: the sequence numbers (H.seq), the event count and the error
// flags, which link_send_lane takes from one status word read back with a single v_readlane.
// PRISMA_LANE_LINKS (build switch for the A/B variants of profiles/lane_links/): bit 0 the
// completion handler, bit 1 link_send, bit 2 the arrival's wire_pop; 0 compiles the gate out.
#ifndef PRISMA_LANE_LINKS
#define PRISMA_LANE_LINKS 7
#endif
// PRISMA_FLAT_SEND (build switch for the A/B variants of profiles/flat_sends/): link_send_lane
// commits with per-lane predicates and no uniform branch on the status word -- 1 fully flat, 2 flat
// behind the uniform early exit of a dropped send (the default: the headline's random-initialised
// table drops often, and the fully flat form lost 1.5 % there), 0 the branching form.
// PRISMA_TOPO_WORD: lk_acc carries the link's far end and that node's row (lane_links_bind), which
// a data arrival takes from one v_readlane instead of three dependent scalar loads.
#ifndef PRISMA_FLAT_SEND
#define PRISMA_FLAT_SEND 2
#endif
#ifndef PRISMA_TOPO_WORD
#define PRISMA_TOPO_WORD 1
#endif
// the access mask (all ones / 0) of lane_links_bind's lk_acc
__device__ __forceinline__ uint32_t lk_acc_mask(uint32_t acc) {
    return PRISMA_TOPO_WORD ? (uint32_t)((int32_t)acc >> 31) : acc;
}
__device__ __forceinline__ void lane_links_bind(Sim& S) {
    const LV& L = S.lv;
    const uint32_t l = (uint32_t)S.lane;         // (the image's arrays hold 256 links, zero past L)
    const bool acc = l >= (uint32_t)L.E();
    S.lk_rinfo = S.T->rinfo[l];
    S.lk_txd = S.T->ltx[2u * (l * 8u + T_RELAY)];
    S.lk_txp = S.T->ltx[2u * (l * 8u + T_PFWD)];
    S.lk_prop = S.T->ltx[2u * (l * 8u + T_RELAY) + 1u] - S.lk_txd;
    S.lk_lim = acc ? L.acc_qmax_pkts() : L.qmax_bytes();
    if (PRISMA_TOPO_WORD) {
        // the link's topology word: far end v (bits 0-7), v's row pointer (8-15) and degree
        // (16-23), the access flag on top.  8 bits hold whatever the image can: its arrays end at
        // 256 links, nodes and tunnels (an LS = 1 instance meets at most 64 links, so 33 nodes,
        // row pointers up to 63 and degrees up to 21)
        static_assert(sizeof(TopoImage::ldst) / sizeof(int32_t) <= 256 && sizeof(TopoImage::ovrow) / sizeof(int32_t) <= 256 &&
                      sizeof(TopoImage::tinfo) / sizeof(uint32_t) <= 256, "topology word: 8-bit fields");
        const uint32_t v = (uint32_t)S.T->ldst[l];
        const uint32_t r0 = (uint32_t)S.T->ovrow[v], deg = (uint32_t)S.T->ovrow[v + 1u] - r0;
        S.lk_acc = (acc ? 1u << 31 : 0u) | (deg & 255u) << 16 | (r0 & 255u) << 8 | (v & 255u);
    } else {
        S.lk_acc = acc ? ~0u : 0u;
    }
    asm volatile("" : "+v"(S.lk_rinfo), "+v"(S.lk_txd), "+v"(S.lk_txp), "+v"(S.lk_prop), "+v"(S.lk_lim),
                 "+v"(S.lk_acc));
}

// status word of link_send_lane (owner lane's, read back by the caller)
constexpr uint32_t LST_DROP = 1u, LST_DUE = 2u, LST_RING = 4u, LST_START = 8u, LST_WIRE = 16u, LST_OLDER = 32u;

// link_send in the link's lane.  The instances that run it see data and ping entries only (no
// ctrl paths), identity overlays (rings in LDS, always stored) and the lazy completions.
template <int FS, int LS>
__device__ __forceinline__ int link_send_lane(const Sim& S, Regs<FS, LS>& R, Hot& H, uint32_t l, uint32_t e) {
    const LV& L = S.lv;
    const uint32_t dsz = L.data_size(), psz = L.ping_size();       // both readlanes first, then selects
    const uint32_t WC = (uint32_t)L.WCAP();
    const uint32_t size = (e & 2u) ? psz : dsz;
    const bool me = (uint32_t)S.lane == l;
    const uint32_t p0 = R.p0.v[0], p1 = R.p1.v[0], p2 = R.p2.v[0], qb = R.qb.v[0];
    const uint32_t nq = p2 & 0xffffu, nw = p1 >> 16, tail = p1 & 0xffffu;
    const uint32_t off = S.lk_rinfo & 0xffffu, cap = S.lk_rinfo >> 16;
    // admission: queued bytes on a switch link, queued packets on an access link
    const uint32_t am = lk_acc_mask(S.lk_acc);
    const uint32_t have = (am & (nq + 1u)) | (~am & (qb + size));
    const bool drop = have > S.lk_lim;
    // an elided completion that precedes the event being executed has happened (lazy_due)
    const uint64_t dd = ((uint64_t)(R.cp_t.v[0] - lo32(H.now)) << 32) + (uint64_t)R.cp_seq.v[0] - (uint64_t)H.cur_seq;
    const bool due = !drop && p2 == 0x10000u && (nw == 0u || (int64_t)dd < 0);
    const bool rfail = !drop && nw + nq + 1u > cap;
    const bool start = !drop && !rfail && (due || (p2 >> 16) == 0u);   // :643-650
    uint32_t st = drop ? LST_DROP : 0u;
    st |= due ? LST_DUE : 0u;
    st |= rfail ? LST_RING : 0u;
    st |= start ? LST_START : 0u;
    st |= (start && nw + 1u > WC) ? LST_WIRE : 0u;
    st |= (start && nq != 0u) ? LST_OLDER : 0u;
    const uint32_t s = rdl(st, l);
    if constexpr (PRISMA_FLAT_SEND != 0) {
        // One straight-line body: the owner lane commits under its own predicates and the scalar
        // side takes the sequence numbers, the event count and the flags from the status word.
        // (With uniform branches on the word the START and the queue path wrote different subsets
        // of the lane fields, which the compiler copied out and back around every inlined site.)
        // A dropped send changes nothing (no other bit stands beside LST_DROP); a ring failure
        // changes nothing but ev_launch (if due) and the flags; a wire failure sets its flag after
        // the state update.
        if (PRISMA_FLAT_SEND == 2 && (s & LST_DROP)) return 0;
        const bool ok = me && !drop && !rfail;
        const bool go = ok && start;
        const uint32_t xi = p0 >> 16;
        uint32_t hx = e;
        if (go && nq != 0u) hx = S.ring[off + xi];                     // (a queue behind an idle transmitter)
        const uint32_t nt = (tail + 1u == cap) ? 0u : tail + 1u;
        const uint32_t nx = (xi + 1u == cap) ? 0u : xi + 1u;
        const bool ping = (hx & 2u) != 0u;
        const uint32_t cpt = lo32(H.now) + (ping ? S.lk_txp : S.lk_txd);
        const uint32_t at = cpt + S.lk_prop;
        const uint32_t cps = H.seq, as = H.seq + 1u;                   // TransmitComplete, channel Receive
        H.seq += (s / LST_START) * 2u & 2u;
        H.ev_launch += (s / LST_DUE) & 1u;
        if (ok) S.ring[off + tail] = e;
        if (go) {
            S.wt[l * WC + (xi & (WC - 1u))] = at;
            S.wseq[l * WC + (xi & (WC - 1u))] = as;
        }
        R.p0.v[0] = go ? ((p0 & 0xffffu) | (nx << 16)) : p0;
        R.p1.v[0] = ok ? (nt | ((nw + (start ? 1u : 0u)) << 16)) : p1;
        R.p2.v[0] = ok ? (start ? (nq | 0x10000u) : p2 + 1u) : p2;
        R.qb.v[0] = ok ? qb + size - (start ? (ping ? psz : dsz) : 0u) : qb;
        R.cp_t.v[0] = go ? cpt : R.cp_t.v[0];
        R.cp_seq.v[0] = go ? cps : R.cp_seq.v[0];
        const bool head = go && nw == 0u;                              // the wire was empty: new head
        R.wh_t.v[0] = head ? at : R.wh_t.v[0];
        R.wh_seq.v[0] = head ? as : R.wh_seq.v[0];
        if (__builtin_expect((s & (LST_RING | LST_WIRE)) != 0u, 0))
            fail(H, (s & LST_RING) ? PRISMA_EBIT_RING : PRISMA_EBIT_WIRE);
        return (s & (LST_DROP | LST_RING)) == 0u;
    }
    if (s & LST_DROP) return 0;
    H.ev_launch += (s / LST_DUE) & 1u;
    if (s & LST_RING) { fail(H, PRISMA_EBIT_RING); return 0; }
    const uint32_t nt = (tail + 1u == cap) ? 0u : tail + 1u;
    if (s & LST_START) {
        const uint32_t xi = p0 >> 16;
        uint32_t hx = e;
        if (s & LST_OLDER) hx = S.ring[off + xi];                  // (a queue behind an idle transmitter)
        const uint32_t nx = (xi + 1u == cap) ? 0u : xi + 1u;
        const bool ping = (hx & 2u) != 0u;
        const uint32_t cpt = lo32(H.now) + (ping ? S.lk_txp : S.lk_txd);
        const uint32_t at = cpt + S.lk_prop;
        const uint32_t cps = H.seq, as = H.seq + 1u;               // TransmitComplete, channel Receive
        H.seq += 2u;
        if (me) {
            S.ring[off + tail] = e;
            S.wt[l * WC + (xi & (WC - 1u))] = at;
            S.wseq[l * WC + (xi & (WC - 1u))] = as;
        }
        R.p0.v[0] = me ? ((p0 & 0xffffu) | (nx << 16)) : p0;
        R.p1.v[0] = me ? (nt | ((nw + 1u) << 16)) : p1;
        R.p2.v[0] = me ? (nq | 0x10000u) : p2;
        R.qb.v[0] = me ? qb + size - (ping ? psz : dsz) : qb;
        R.cp_t.v[0] = me ? cpt : R.cp_t.v[0];
        R.cp_seq.v[0] = me ? cps : R.cp_seq.v[0];
        const bool head = me && nw == 0u;                          // the wire was empty: new head
        R.wh_t.v[0] = head ? at : R.wh_t.v[0];
        R.wh_seq.v[0] = head ? as : R.wh_seq.v[0];
        if (s & LST_WIRE) fail(H, PRISMA_EBIT_WIRE);
    } else {
        if (me) S.ring[off + tail] = e;
        R.p1.v[0] = me ? (nt | (nw << 16)) : p1;
        R.p2.v[0] = me ? p2 + 1u : p2;
        R.qb.v[0] = me ? qb + size : qb;
    }
    return 1;
}

// on_complete in the link's lane.  A completion is only selected while packets wait behind the
// transmitter (select_event's cpv: busy = 1, n_queue > 0), so the dequeue and the next
// transmission are unconditional and no field has to become uniform.
template <int FS, int LS>
__device__ __forceinline__ void on_complete_lane(const Sim& S, Regs<FS, LS>& R, Hot& H, uint32_t l) {
    const LV& L = S.lv;
    const uint32_t dsz = L.data_size(), psz = L.ping_size();
    const uint32_t WC = (uint32_t)L.WCAP();
    const bool me = (uint32_t)S.lane == l;
    const uint32_t p0 = R.p0.v[0], p1 = R.p1.v[0], p2 = R.p2.v[0], qb = R.qb.v[0];
    const uint32_t off = S.lk_rinfo & 0xffffu, cap = S.lk_rinfo >> 16;
    const uint32_t xi = p0 >> 16, nw = p1 >> 16;
    const uint32_t hx = S.ring[off + xi];                          // each lane its own ring's head
    const uint32_t nx = (xi + 1u == cap) ? 0u : xi + 1u;
    const bool ping = (hx & 2u) != 0u;
    const uint32_t cpt = lo32(H.now) + (ping ? S.lk_txp : S.lk_txd);
    const uint32_t at = cpt + S.lk_prop;
    const uint32_t cps = H.seq, as = H.seq + 1u;                   // TransmitComplete, channel Receive
    H.seq += 2u;
    if (me) {
        S.wt[l * WC + (xi & (WC - 1u))] = at;
        S.wseq[l * WC + (xi & (WC - 1u))] = as;
    }
    R.p0.v[0] = me ? ((p0 & 0xffffu) | (nx << 16)) : p0;
    R.p1.v[0] = me ? p1 + 0x10000u : p1;
    R.p2.v[0] = me ? p2 - 1u : p2;                                 // busy stays 1
    R.qb.v[0] = me ? qb - (ping ? psz : dsz) : qb;
    R.cp_t.v[0] = me ? cpt : R.cp_t.v[0];
    R.cp_seq.v[0] = me ? cps : R.cp_seq.v[0];
    const bool head = me && nw == 0u;                              // the wire was empty: new head
    R.wh_t.v[0] = head ? at : R.wh_t.v[0];
    R.wh_seq.v[0] = head ? as : R.wh_seq.v[0];
    if (__ballot(me && nw + 1u > WC) != 0ull) fail(H, PRISMA_EBIT_WIRE);
}

// returns 1 if enqueued, 0 if dropped (a ring overflow fails the replica)
// link_send with the link's state already fetched (the memory-resident engine's flow event
// issues the record load early); the register-resident engine keeps the plain form below,
// whose register allocation the by-value LinkV disturbs
template <class RS>
__device__ __forceinline__ int link_send_k(const Sim& S, RS& R, Hot& H, uint32_t l, uint32_t e, LinkV k) {
    const LV& L = S.lv;
    TP1_START();
    uint32_t size = ent_size(S, e, l);
    bool ok = l < (uint32_t)L.E() ? (k.qb + size <= L.qmax_bytes()) : (k.n_queue + 1u <= L.acc_qmax_pkts());
    TP1(11);
    if (!ok) return 0;
    if (RS::kLazy) {
        // the transmitter's completion was elided (nothing queued behind it): if it precedes
        // the event being executed it has happened -- count it now (lazy_due)
        const bool due = k.busy && k.n_queue == 0u && lazy_due(k.n_wire, k.cp_t, k.cp_seq, H);
        k.busy = due ? 0u : k.busy;
        H.ev_launch += due ? 1u : 0u;
    }
    uint32_t cap = ring_cap(S, l), off = ring_off(S, l);
    if (k.n_wire + k.n_queue + 1u > cap) { fail(H, PRISMA_EBIT_RING); return 0; }
    if (ring_store_needed(S, k)) q_put(S, l, off, k.tail, k.n_queue, e);
    k.tail = (k.tail + 1 == cap) ? 0 : k.tail + 1;
    k.n_queue++;
    k.qb += size;
    TP1(12);
    if (!k.busy) {                                              // :643-650
        uint32_t xi = k.txp;
        uint32_t hx = (k.n_queue == 1) ? e : q_take(S, l, off, xi);
        k.txp = (xi + 1 == cap) ? 0 : xi + 1;
        k.n_queue--;
        k.n_wire++;
        k.qb -= ent_size(S, hx, l);
        transmit_start(S, H, l, k, xi, hx);
    }
    TP1(13);
    link_put(S, R, H, l, k);
    TP1(15);
    return 1;
}
template <class RS>
__device__ __forceinline__ int link_send(const Sim& S, RS& R, Hot& H, uint32_t l, uint32_t e) {
    const LV& L = S.lv;
    if constexpr (!RS::kMem && (PRISMA_LANE_LINKS & 2) != 0) {
        if (S.lanel) return link_send_lane(S, R, H, l, e);
    }
    LinkV k = link_get(R, l);
    uint32_t size = ent_size(S, e, l);
    // admission (switch links by queued bytes, access links by queued packets) as one compare
    // of selected operands: the compiler had branched on the link kind
    const bool sw = l < (uint32_t)L.E();
    const uint32_t have = sw ? k.qb + size : k.n_queue + 1u;
    const uint32_t lim = sw ? L.qmax_bytes() : L.acc_qmax_pkts();
    if (have > lim) return 0;
    if (RS::kLazy) {
        // the transmitter's completion was elided (nothing queued behind it): if it precedes
        // the event being executed it has happened -- count it now (lazy_due).  A uniform branch
        // on the elided state: the combined condition had become ~15 scalar mask operations
        // (busy is 0 or 1: one compare of the packed transmitter word instead of two conditions
        // the compiler combined as 64-bit lane masks)
        if (((k.busy << 16) | k.n_queue) == 0x10000u) {
            if (lazy_due(k.n_wire, k.cp_t, k.cp_seq, H)) { k.busy = 0u; H.ev_launch++; }
        }
    }
    uint32_t cap = ring_cap(S, l), off = ring_off(S, l);
    if (k.n_wire + k.n_queue + 1u > cap) { fail(H, PRISMA_EBIT_RING); return 0; }
    if (ring_store_needed(S, k)) q_put(S, l, off, k.tail, k.n_queue, e);
    k.tail = (k.tail + 1 == cap) ? 0 : k.tail + 1;
    k.n_queue++;
    k.qb += size;
    if (!k.busy) {                                              // :643-650
        uint32_t xi = k.txp;
        uint32_t hx = (k.n_queue == 1) ? e : q_take(S, l, off, xi);
        k.txp = (xi + 1 == cap) ? 0 : xi + 1;
        k.n_queue--;
        k.n_wire++;
        k.qb -= ent_size(S, hx, l);
        transmit_start(S, H, l, k, xi, hx);
    }
    link_put(S, R, H, l, k);
    return 1;
}


template <class RS>
__device__ __forceinline__ void on_complete(const Sim& S, RS& R, Hot& H, uint32_t l) {   // :305-336
    const LV& L = S.lv;
    if constexpr (!RS::kMem && (PRISMA_LANE_LINKS & 1) != 0) {
        if (S.lanel) { on_complete_lane(S, R, H, l); return; }
    }
    if (S.mem) TP1_START();
    TP2_START();
    LinkV k = link_get(R, l);
    k.busy = 0;
    if (S.mem) TP1(7);
    TP2(11);
    if (k.n_queue) {
        uint32_t cap = ring_cap(S, l);
        uint32_t xi = k.txp;
        uint32_t hx = q_take(S, l, ring_off(S, l), xi);
        if (S.mem) TP1(8);
        k.txp = (xi + 1 == cap) ? 0 : xi + 1;
        k.n_queue--;
        k.n_wire++;
        k.qb -= ent_size(S, hx, l);
        transmit_start(S, H, l, k, xi, hx);
    }
    if (S.mem) TP1(9);
    TP2(12);
    link_put(S, R, H, l, k);
    if (S.mem) TP1(10);
    TP2(13);
}

// ---- observation (data-packet-manager.cc:171-206)
// send time in seconds of ping round k as the ping-back manager stores it:
// (double)GetMilliSeconds() * 0.001 (ping-back-packet-manager.cc:98-116)
// floor((k + 1) period / 10^6) on the vector unit: the product is exact (< 2^42 ns), and the
// reciprocal of 10^6 rounded up keeps a multiple of 10^6 on its quotient (numerics.h div_1e3)
__device__ __forceinline__ double ping_send_s(const LV& L, int64_t k) {
    const double ms = __builtin_floor((double)(k + 1) * (double)L.ping_period() * 0x1.0c6f7a0b5ed8ep-20);
    return ms * 0.001;
}

__device__ __forceinline__ double ld_d(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// 1000 * max(mean(window), min(now - oldest unacknowledged send, 2.6)) of a
// tunnel (data-packet-manager.cc:171-206).  The unacknowledged list is kept
// as its oldest round lo (pending iff lo < rounds sent) plus the acked bits
// of the 64 rounds after it; the window mean and lo's send time are cached
// per tunnel and refreshed on every ping-back.  Evaluated per lane for the
// tunnels the lane owns.
__device__ __forceinline__ uint32_t ping_value_lane(double avg, uint32_t lo, double od, uint32_t rounds, double now_s) {
    const bool pend = lo < rounds;
    const double a = now_s - od;
    const double b = 2.60;
    const float mt = pend ? (float)((b < a) ? b : a) : 0.0f;
    const double mx = (avg < (double)mt) ? (double)mt : avg;
    return (uint32_t)(1000 * mx);
}

// Observation of node v as a per-lane register (lane i holds obs[i], lane 0
// left 0 for the destination): every lane evaluates the tunnels (ping
// statistic) or links (queued bytes) it owns in parallel, then lane i pulls
// the value of action i-1 with one permute per register slot.  Action a of v
// is tunnel ovrow[v] + a; its queue is that of the tunnel's first link
// (the device RouteOutput picks, data-packet-manager.cc:180-195), which is
// the tunnel itself on identity overlays.
// (r0, deg: node v's row pointer and degree, read by the caller, which hands them on to the
// decision's send)
template <int FS, int LS>
__device__ __forceinline__ uint32_t observe_links(const Sim& S, const Regs<FS, LS>& R, const Hot& H, uint32_t v,
                                                  double now_s, int r0 = -1, int deg = 0) {
    if (r0 < 0) { r0 = t_ovrow(S, v); deg = t_ovrow(S, v + 1) - r0; }
    const int lane = S.lane;
    uint32_t src = (uint32_t)(r0 + lane - 1);
    const bool pobs = S.lv.ping_as_obs() != 0u;
    if (!pobs && S.tun) {
        const bool act = lane >= 1 && lane <= deg;
        src = act ? ti_link(S.T->tinfo[act ? src : 0u]) : 0u;
    }
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < LS; ++j) {
        uint32_t val;
        if (pobs)
            val = ping_value_lane(ld_d(R.pav_lo.v[j], R.pav_hi.v[j]), R.pm_lo.v[j], ld_d(R.od_lo.v[j], R.od_hi.v[j]),
                                  H.ping_rounds, now_s);
        else
            val = R.qb.v[j];
        const uint32_t g = bperm(val, src & 63u);
        if ((src >> 6) == (uint32_t)j) o = g;
    }
    return (lane >= 1 && lane <= deg) ? o : 0u;
}

// one coalesced wave store of a decision record (lane i writes word i)
__device__ __forceinline__ void write_record(const Sim& S, const Hot& H, uint32_t d, double reward, uint32_t uid,
                                             int32_t prev, uint32_t node, uint32_t dst, uint32_t start, int action,
                                             uint32_t status, uint32_t obs_reg, uint32_t ttl) {
    const int lane = S.lane;
    uint64_t rb = __double_as_longlong(reward);
    uint32_t w7 = (uint32_t)(uint8_t)(int8_t)action | (status << 8) | (ttl << 16) | ((H.episode & 0xffu) << 24);
    // lane l < 8 picks header word l with three lane-bit selects, no per-lane compares
    // (A/B +3.5 % at the headline against a switch on the lane id)
    // (bitfield inserts on the per-lane masks, v_bfi_b32: A/B +1.4 % at the headline against
    // lane-bit selects, whose loop-invariant SGPR-pair conditions were spilled and reloaded)
    auto bfi = [](uint32_t m, uint32_t a, uint32_t b) { return (m & a) | (~m & b); };
    const uint32_t a01 = bfi(S.m1, hi32(H.now), lo32(H.now));
    const uint32_t a23 = bfi(S.m1, (uint32_t)prev, uid);
    const uint32_t a45 = bfi(S.m1, (uint32_t)(rb >> 32), (uint32_t)rb);
    const uint32_t a67 = bfi(S.m1, w7, node | (dst << 8) | (start << 16));
    const uint32_t a03 = bfi(S.m2, a23, a01);
    const uint32_t a47 = bfi(S.m2, a67, a45);
    const uint32_t hw = bfi(S.m4, a47, a03);
    uint32_t ob = bperm(obs_reg, (uint32_t)(lane - 8) & 63u);
    uint32_t word = bfi(S.m8, hw, ob);
    uint32_t* p = (uint32_t*)(S.logrep + (size_t)(d & (S.lv.log_cap() - 1)) * S.lv.rec_bytes());
    if (lane < 8 + S.lv.W()) p[lane] = word;
}

// action + status of a record written earlier (TTL and episode bytes kept)
__device__ __forceinline__ void patch_record(const Sim& S, const Hot& H, uint32_t d, int action, uint32_t status) {
    if (S.lane == 0) {
        unsigned char* p = S.logrep + (size_t)(d & (S.lv.log_cap() - 1)) * S.lv.rec_bytes();
        *(uint16_t*)(p + 28) = (uint16_t)((uint32_t)(uint8_t)(int8_t)action | (status << 8));
    }
}
__device__ __forceinline__ void patch_status(const Sim& S, uint32_t d, uint32_t status) {
    if (S.lane == 0) S.logrep[(size_t)(d & (S.lv.log_cap() - 1)) * S.lv.rec_bytes() + 29] = (unsigned char)status;
}

// Receive tail after the MacRx trace (point-to-point-net-device.cc:430-463).
// arrived: a data packet at its destination (start = its start second).
// l: the arrival link (the size of an echo)
template <class RS>
__device__ __forceinline__ void receive_counters(const Sim& S, RS& R, const Hot& H, uint32_t x, bool arrived,
                                                 uint32_t start, uint32_t l) {
    const LV& L = S.lv;
    if (arrived) {
        // valable, nextHop == finalDest on identity overlays
        CNT_ADD(S, ov_arrived, 1u);
        const float cost = (float)(ns_to_sec(H.now) - (double)start);
        CNT_ADD(S, cost_sum, cost);
        CNT_ADD(S, cost_n, 1u);
        CNT_ADD(S, e2e_sum, cost);
        CNT_ADD(S, e2e_n, 1u);
    }
    // pings are always addressed to the node that receives them
    if (!ent_is_data(x)) CNT_ADD(S, bytes_signaling, ent_size(S, x, l) - 2u);
    if (ent_type(x) == T_FRESH) {
        CNT_ADD(S, ov_injected, 1u);
        CNT_ADD(S, bytes_data, L.data_size() - 2u);
    }
}

constexpr uint32_t kNoLink = 0xffffffffu;

// source node of a data entry (MyTag source) that arrived at node v: a fresh
// packet arrives at its own source switch
__device__ __forceinline__ uint32_t ent_src(uint32_t x, uint32_t v) {
    return ent_type(x) == T_FRESH ? v : r_src(x);
}

// DataPacketManager::sendSmallSignalingPacket (data-packet-manager.cc:301-347): a 0-B
// payload (30 B on the wire, signalling type "ideal") back on the arrival device,
// addressed to the data packet's last hop `to`
template <class RS>
__device__ __forceinline__ void send_echo(const Sim& S, RS& R, Hot& H, uint32_t link, uint32_t uid,
                                          uint32_t to) {
    if (!link_send(S, R, H, link, e_make(uid, to))) CNT_ADD(S, ctrl_dropped, 1u);
}

// routing table of a tunnelled overlay: next link x -> y | hops(x, y) << 8
__device__ __forceinline__ uint32_t route(const Sim& S, uint32_t x, uint32_t y) {
    const c_u32* rt = (const c_u32*)((const CAS unsigned char*)S.T + sizeof(TopoImage));
    return rt[x * (uint32_t)S.lv.N() + y];
}
// first link of tunnel t
__device__ __forceinline__ uint32_t tunnel_link(const Sim& S, uint32_t t) {
    return S.tun ? ti_link(S.T->tinfo[t]) : t;
}

// (relay_ip: ring_put)
__device__ __forceinline__ uint32_t relay_dist(const Sim& S, uint32_t d, uint32_t x) {
    return relay_ip(S) ? (d - rip_dec(x)) & kRipMask : (d - r_dec(x)) & kRelayMask;
}
// byte offsets of record words 6 (node | dst << 8 | start << 16) and 7 (action | status << 8 |
// TTL << 16 | episode << 24): write_record
__device__ __forceinline__ uint32_t record_word(const Sim& S, uint32_t d, uint32_t off) {
    return rfl(*(const uint32_t*)(S.logrep + (size_t)(d & (S.lv.log_cap() - 1)) * S.lv.rec_bytes() + off));
}
// a relayed data packet dropped on an intermediate FIFO: point-to-point-net-device.cc:655-664 at
// switch v, MacTxDrop -> the sender's loss (data-packet-manager.cc:88-98, forwarder.py:214-244)
__device__ __forceinline__ void relay_dropped(const Sim& S, uint32_t dd, uint32_t dst, uint32_t v) {
    const LV& L = S.lv;
    if (dst != v) {
        CNT_ADD(S, ov_lost, 1u);
        CNT_ADD(S, cost_sum, L.loss_penalty_f());
        CNT_ADD(S, cost_n, 1u);
    } else {
        CNT_ADD(S, un_lost, 1u);
        CNT_ADD(S, un_cost_sum, L.loss_penalty_f());
        CNT_ADD(S, un_cost_n, 1u);
    }
    patch_status(S, dd, PRISMA_ST_DROPPED);
    CNT_ADD(S, reward_sum, L.loss_penalty());
}

// DataPacketManager::sendPacket (data-packet-manager.cc:251-299) for decision
// d at node v, then the Receive tail.  x is the arriving entry (for the
// counters); fused: the record is written here once, with the final status
// (table policy).
// ROW: r0_in / deg_in hold node v's row pointer and degree (read on the arrival)
template <bool ROW = false, class RS>
__device__ __forceinline__ void apply_decision(const Sim& S, RS& R, Hot& H, uint32_t x, uint32_t dst,
                                               uint32_t start, uint32_t uid, uint32_t v, uint32_t d, int action,
                                               bool fused, double reward, int32_t prev, uint32_t obs_reg,
                                               uint32_t echo_link, uint32_t last, uint32_t ttl,
                                               int r0_in = -1, int deg_in = 0) {
    const LV& L = S.lv;
#if PRISMA_TIMING
    S.tlast = TM_NOW();
#endif
    // ExecuteActions (packet-routing-gym.cc:203-208): the --train echo goes first
    if (echo_link != kNoLink) send_echo(S, R, H, echo_link, uid, last);
    TP2_START();
    v = rfl(v);                                     // (scalar loads of the row pointers)
    int r0 = r0_in, deg = deg_in;
    if (!ROW) { r0 = t_ovrow(S, v); deg = t_ovrow(S, v + 1) - r0; }
    uint32_t status;
    if ((uint32_t)action < (uint32_t)deg) {                      // 0 <= action < deg
        const uint32_t tiw = S.tun ? (uint32_t)S.T->tinfo[(uint32_t)(r0 + action)] : 0u;
        const uint32_t l = S.tun ? ti_link(tiw) : (uint32_t)(r0 + action);   // RouteOutput (:281-287)
        if (RS::kMem || S.mlp_inst) {
            CNT_ADD(S, hops, 1u);
            CNT_ADD(S, hop_deg_sum, (uint64_t)deg);
        }
        // (memory-resident engine without the ctrl paths: the destination instead of the
        // source, engine_layout.h)
        const uint32_t src = (RS::kMem && !S.ctrl) ? dst : ent_src(x, v);
        const uint32_t fwd = relay_ip(S) ? rip_make(d, ttl, ti_tgt(tiw)) : r_make(d, src);
        TP2(7);
        if (link_send(S, R, H, l, fwd)) {                         // lastHop = v, previous decision = d
            status = PRISMA_ST_ENQUEUED;
        } else {
            status = PRISMA_ST_DROPPED;              // :655-664 + forwarder.py:214-244
            CNT_ADD(S, ov_lost, 1u);
            CNT_ADD(S, cost_sum, L.loss_penalty_f());
            CNT_ADD(S, cost_n, 1u);
            CNT_ADD(S, reward_sum, L.loss_penalty());
        }
    } else {
        status = PRISMA_ST_DISCARDED;
    }
#if PRISMA_TIMING
    { const uint64_t t = TM_NOW(); S.tsub[0] += t - S.tlast; S.tlast = t; }
#endif
    TP0(12);
    TP2(8);
    if (fused) write_record(S, H, d, reward, uid, prev, v, dst, start, action, status, obs_reg, ttl);
    else patch_record(S, H, d, action, status);
    TP2(9);
    if (RS::kMem || S.mlp_inst) {
        receive_counters(S, R, H, x, false, 0u, 0u);
    } else if (S.lane == 0) {
        // table instances: the hop's integer counters and the Receive tail's (a data packet:
        // receive_counters) in one lane-0 region -- integer adds, so their order is free (A/B:
        // headline +0.7 %)
        if ((uint32_t)action < (uint32_t)deg) {
            lds_add(&S.c->hops, (decltype(S.c->hops))1u);
            lds_add(&S.c->hop_deg_sum, (decltype(S.c->hop_deg_sum))deg);
        }
        if (ent_type(x) == T_FRESH) {
            lds_add(&S.c->ov_injected, (decltype(S.c->ov_injected))1u);
            lds_add(&S.c->bytes_data, (decltype(S.c->bytes_data))(L.data_size() - 2u));
        }
    }
    TP2(10);
#if PRISMA_TIMING
    { const uint64_t t = TM_NOW(); S.tsub[1] += t - S.tlast; S.tlast = t; }
#endif
    TP0(13);
}

// Answer to the pending notification.  Returns 1 if a hop was executed (0 for a
// destination or control notification, whose action is ignored: sendPacket at
// the destination does nothing (:256-260), ExecuteActions sends nothing for a
// small-signalling packet).
template <class RS>
__device__ __forceinline__ int finish_pending(const Sim& S, RS& R, Hot& H, int action) {
    const Hdr& h = *S.h;
    H.pend = 0;
    const uint32_t x = u_ld32(&h.pend_ent[0]), flags = u_ld32(&h.pend_ent[3]);
    if (S.ctrl && (flags & PEND_CTRL)) {
        receive_counters(S, R, H, x, false, 0u, u_ld32(&h.pend_link));
        return 0;
    }
    const uint32_t echo_link = (S.ctrl && (flags & PEND_ECHO)) ? (uint32_t)t_lrev(S, u_ld32(&h.pend_link)) : kNoLink;
    const uint32_t last = u_ld32(&h.pend_last);
    if (S.ctrl && (flags & PEND_DEST)) {
        if (echo_link != kNoLink) send_echo(S, R, H, echo_link, u_ld32(&h.pend_uid), last);
        receive_counters(S, R, H, x, true, u_ld32(&h.pend_ent[2]), 0u);
        return 0;
    }
    // (relay entries with the TTL: the pending decision's, from its record)
    const uint32_t pdec = u_ld32(&h.pend_dec);
    const uint32_t ttl = relay_ip(S) ? (record_word(S, pdec, 28) >> 16) & 255u : 0u;
    apply_decision(S, R, H, x, 0u, 0u, u_ld32(&h.pend_uid), u_ld32(&h.pend_node), pdec, action,
                   false, 0.0, 0, 0u, echo_link, last, ttl);
    return 1;
}

// ---- handlers (uniform) ------------------------------------------------------
template <class RS>
__device__ __forceinline__ void on_ping_round(const Sim& S, RS& R, Hot& H) {   // data-packet-manager.cc:350-413
    const LV& L = S.lv;
    uint32_t k = H.ping_rounds;
    uint32_t first_rearm = 0;
    for (int i = 0; i < L.NO(); ++i) {                            // timers in overlay order (sim.cc:528-546)
        const int u = S.tun ? S.T->ovnode[i] : i;
        const int r0 = t_ovrow(S, u), r1 = t_ovrow(S, u + 1);
        for (int t = r0; t < r1; ++t) {
            if (!link_send(S, R, H, tunnel_link(S, (uint32_t)t), p_make(T_PFWD, (uint32_t)t, 0u, k)))
                CNT_ADD(S, ctrl_dropped, 1u);
        }
        uint32_t s = H.seq++;                                    // re-arm of node u
        if (i == 0) first_rearm = s;
    }
    H.ping_rounds = k + 1;
    // one ns-3 event per overlay node timer (the round is NO consecutive events)
    H.ev_launch += (uint32_t)(L.NO() - 1);
    H.ping_t = H.now + L.ping_period();
    H.ping_seq = first_rearm;
    flow_min_refresh(S, R, H);
}

// ns-3 stream mode (PRISMA_RNG_NS3): the uniform of the ExponentialRandomVariable that
// ScheduleNextTx creates for every packet (poisson-application.cc:281-284) -- the first value
// of a new stream.  A packet's SendPacket creates a UniformRandomVariable first (:311-314; its
// value only sets the tag's overlay flag, 1 for every flow here), so draws after the first skip
// one stream.  State: the next stream's initial state and the jump J, in LDS (kRngBytes).
__device__ __forceinline__ double ns3_exp_u01(const Sim& S, uint32_t draw) {
    uint32_t* g = (uint32_t*)(S.base + S.lv.lds_state_bytes() - kRngBytes);
    uint32_t st[6], J[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = u_ld32(g + i);
#pragma unroll
    for (int i = 0; i < 18; ++i) J[i] = u_ld32(g + 8 + i);
    if (draw != 0) mrg_apply(J, st);                              // SendPacket's uniform stream
    uint32_t e[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] = st[i];
    const double U = mrg_u01(e);
    mrg_apply(J, st);
#pragma unroll
    for (int i = 0; i < 6; ++i) st_rep(S, g + i, st[i]);
    return U;
}

// ns-3 stream mode at an episode start: flow f's start offset comes from the
// UniformRandomVariable the flow loop creates for it (sim.cc:610-620), the f-th stream from
// rng_stream_offset on -- state J^f T, from the table's powers of J -- and the LDS image gets
// the run's first stream (the one after the flows') and J.  rep: the replica's table entry.
__device__ __forceinline__ double ns3_start_u01(const uint32_t* rng, const uint32_t* rep, uint32_t f) {
    uint32_t st[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) st[i] = rep[i];
    for (uint32_t b = 0; b < kMrgPowers; ++b)
        if ((f >> b) & 1u) mrg_apply(rng + 18u * b, st);
    return mrg_u01(st);
}
__device__ __forceinline__ void ns3_init_lds(const Sim& S, const uint32_t* rng, const uint32_t* rep) {
    uint32_t* g = (uint32_t*)(S.base + S.lv.lds_state_bytes() - kRngBytes);
    if (S.lane < 6) g[S.lane] = rep[6 + S.lane];
    else if (S.lane >= 8 && S.lane < 26) g[S.lane] = rng[S.lane - 8];
}

template <class RS>
__device__ __forceinline__ void flow_next(const Sim& S, RS& R, Hot& H, uint32_t f, uint32_t draw) {
    // (only the CTRL instances carry the ns-3 streams: the host picks them for rng_mode, so the
    // Philox instances' event loop keeps its registers)
    if (S.ctrl && S.lv.rng_mode()) {
        const double delay = -t_fmean(S, f) * det_log(ns3_exp_u01(S, draw));
        flow_set(S, R, H, f, H.now + sec_to_ns(delay), H.seq++, draw + 1);
        return;
    }
    // The draw cache (register-resident engine, where LDS has room: Layout::s_dcache = LDS offset
    // | K): a flow's draws come in groups of K (2 or 3). The first draw of a group is computed in
    // lane 0 and the next K - 1 in lanes 1 .. K-1 by the same vector instructions -- Philox, the
    // logarithm and the conversion cost one draw -- and their send delays wait in the flow's LDS
    // slots for its next sends. Every draw keeps its own Philox counter (flow, draw, episode), so
    // the values are the uncached ones; an episode starts each flow at draw 0, which refills the
    // slots before the first read.
    constexpr bool kDc = !RS::kMem && RS::kDcache;
    const uint32_t dcw = kDc ? S.lv.s_dcache() : 0u;
    if (kDc && dcw != 0u) {
        const uint32_t K = dcw & 15u;
        int64_t* slot = (int64_t*)(S.base + (dcw & ~15u)) + f * (K - 1u);
        const uint32_t g = (K == 2u) ? (draw & 1u) : draw - 3u * (uint32_t)(((uint64_t)draw * 0xAAAAAAABull) >> 33);
        int64_t dns;
        if (g != 0u) {
            dns = u_ld64(slot + (g - 1u));
        } else {
            const uint32_t j = (uint32_t)S.lane < K ? (uint32_t)S.lane : 0u;
            uint32_t c[4] = { f, draw + j, H.episode, 1u };
            philox4x32_10(c, S.lv.seed_lo(), S.gid);
            const uint64_t u53 = ((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6);
            const double U = ((double)u53 + 1.0) * (1.0 / 9007199254740992.0);
            const int64_t dn = sec_to_ns(-t_fmean(S, f) * det_log(U));
            if (j != 0u) slot[j - 1u] = dn;
            dns = mk64(rfl(lo32(dn)), rfl(hi32(dn)));
        }
        flow_set(S, R, H, f, H.now + dns, H.seq++, draw + 1);
        return;
    }
    uint32_t c[4] = { f, draw, H.episode, 1u };                   // poisson-application.cc:265-295
    // The table-policy instances run the rounds on the vector unit (the values pass through
    // VGPRs, so the compiler cannot keep them scalar) and take back the two words they use:
    // ~80 scalar instructions per flow event moved off the headline's busiest unit.  The MLP
    // instances keep the scalar rounds with their keys hoisted out of the event loop.
    uint32_t k0 = S.lv.seed_lo(), k1 = S.gid;
    if (!S.mlp_inst) asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(k0), "+v"(k1));
    philox4x32_10(c, k0, k1);
    if (!S.mlp_inst) { c[0] = __builtin_amdgcn_readfirstlane(c[0]); c[1] = __builtin_amdgcn_readfirstlane(c[1]); }
    uint64_t u53 = ((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6);
    double U = ((double)u53 + 1.0) * (1.0 / 9007199254740992.0);
    double delay = -t_fmean(S, f) * det_log(U);
    int64_t t = H.now + sec_to_ns(delay);
    if constexpr (RS::kMem) TM_FLOW(2);
    flow_set(S, R, H, f, t, H.seq++, draw + 1);
    if constexpr (RS::kMem) TM_FLOW(3);
}

// The BigSignalingGeneratorApplications (big-signaling-application.cc:224-309), all in flow
// slot F.  Every generator starts at AppStartTime and sends one 512-B segment per period, so
// all of them fire at the same instants, in install order (their seqs were taken in that order
// one period earlier, and every seq taken in between belongs to an access-link event of the
// group, at most one transmission later): like a ping round, one slot executes the G
// consecutive ns-3 events -- the first of them starts the sends (StartSending), the others
// hand segment k to the traffic node's access link (SendPacket :261-309) -- and re-arms with
// the seq of the first reschedule (ScheduleNextTx :235-259).
template <class RS>
__device__ __forceinline__ void on_bsig(const Sim& S, RS& R, Hot& H, uint32_t f) {
    const uint32_t k = flow_draw(S, R, f);
    const uint32_t G = t_ngen(S), E = (uint32_t)S.lv.E();
    if (k > kGenSendMask) fail(H, PRISMA_EBIT_TIME);                // 17-bit send index (host-checked)
    uint32_t first = 0;
    for (uint32_t g = 0; g < G; ++g) {
        if (k != 0 && !link_send(S, R, H, E + bp_src(t_bpair(S, g)), g_make(g, k))) CNT_ADD(S, ctrl_dropped, 1u);
        const uint32_t sq = H.seq++;
        if (g == 0) first = sq;
    }
    H.ev_launch += G - 1u;
    flow_set(S, R, H, f, H.now + t_bs_period(S), first, k + 1u);
}

template <class RS>
__device__ __forceinline__ void on_flow(const Sim& S, RS& R, Hot& H, uint32_t f) {
    // memory-resident engine: the access link's record is fetched first, so its load and the
    // flow block's are in flight together (one HBM round trip)
    uint32_t draw;
#if PRISMA_TIMING
    S.tfl = TM_NOW();
#endif
    if constexpr (RS::kMem) {
        if (S.ctrl && f >= (uint32_t)S.lv.F()) { on_bsig(S, R, H, f); return; }
        const uint32_t acc = (uint32_t)S.lv.E() + (uint32_t)t_fsrc(S, f);
        const LinkV k = link_get(R, acc);
        draw = flow_draw(S, R, f);
        TM_FLOW(0);
        if (draw != 0) {                                            // SendPacket :297-358
            const uint32_t par = (uint32_t)(TSEC(H.now)) & 1u;          // start second (its parity)
            link_send_k(S, R, H, acc, f_make((uint32_t)t_fdst(S, f), par, H.uid & kUidMask), k);
            H.uid++;
        }
        TM_FLOW(1);
    } else {
        if (S.ctrl && f >= (uint32_t)S.lv.F()) { on_bsig(S, R, H, f); return; }
        TP2_START();
        draw = flow_draw(S, R, f);
        if (draw != 0) {
            const uint32_t src = (uint32_t)t_fsrc(S, f);
            const uint32_t par = (uint32_t)(TSEC(H.now)) & 1u;
            TP2(14);
            link_send(S, R, H, (uint32_t)S.lv.E() + src, f_make((uint32_t)t_fdst(S, f), par, H.uid & kUidMask));
            H.uid++;
        }
        TP2(15);
    }
    flow_next(S, R, H, f, draw);                                    // StartSending / ScheduleNextTx
}

// ---- in-kernel DQN_buffer_model (models.py:258-306; fixed fp32 operation order,
// DESIGN.md §2, restated by the oracle's mlp_action): lane j computes unit j of
// each layer, activations are broadcast through 64 floats of LDS, weights are
// read per lane from HBM (L2-resident, shared by every replica).
// The layers read their weights from an interleaved per-node copy (prisma_mlp_repack_kernel,
// filled by prisma_run from the caller's row-major weights). Node block = [L1][L2][L3][L4]:
// * L1: the buffers branch, chunk c holding Wb[4c..4c+3][j] as one float4 per unit j < 32
//   (rows k >= D zero), then bb[32] and b1[32] (the one-hot rows of W1 stay in the caller's
//   buffer: one row per decision);
// * L2, L3, L4: chunk c holding W[4c..4c+3][j] as one float4 per output unit j, then the
//   bias row.
// Lane j loads one coalesced 16-B value per 4 inputs instead of 4 dependent 4-B ones, and
// the accumulation order (input 0, 1, 2, ..., one fmaf each) is unchanged.
__host__ __device__ constexpr int mlp_rp_l1_floats(int D) { return 128 * ((D + 3) / 4) + 64; }
__host__ __device__ constexpr int mlp_rp_layer_floats(int units) { return 64 * units + units; }
__host__ __device__ constexpr int mlp_rp_node_floats(int D) {   // rounded to whole float4s
    return (mlp_rp_l1_floats(D) + 2 * mlp_rp_layer_floats(64) + mlp_rp_layer_floats(D) + 3) & ~3;
}

// memory-resident engine (one wave per SIMD and VGPRs to spare): every weight of layers 2-4
// is loaded when the decision starts, one round trip in all
struct MlpPre {
    float4 w2[16], w3[16], w4[16];
    float b2, b3, b4;
};
// what the memory-resident engine's arrival handler fetches for the decision that follows
// (layer 1's buffer-branch chunks and bias): it rides along the arrival's second
// round trip; layer 2 is issued when the decision starts and layers 3-4 load while layers
// 1-2 compute
struct MlpPre1 {
    // (w2, b2: layer 2's weights, which rode along too until round 5, never written or read now.
    // They stay: the compiler scalarises this struct by its layout, and without them the
    // memory-resident MLP kernels come out with another register allocation -- 143 SGPR spills
    // for 116 in the ctrl instance)
    float4 w2[16];
    float b2;
    float4 wb[4];
    float b1v;
    float w1v;                   // the one-hot row element, when the destination was known (has_w1)
    bool has_w1;
};

// (l2: every caller loads layer 2.  The parameter and the pointer test stay: written without
// them the memory-resident MLP kernels come out with another register allocation)
__device__ __forceinline__ void mlp_preload(MlpPre& M, const float* __restrict__ RP, int lane, int D, int deg,
                                            bool l2 = true) {
    const float4* __restrict__ W2 = l2 ? (const float4*)RP : nullptr;
    const float4* __restrict__ W3 = (const float4*)(RP + mlp_rp_layer_floats(64));
    const float4* __restrict__ W4 = (const float4*)(RP + 2 * mlp_rp_layer_floats(64));
    if (W2) {
#pragma unroll
        for (int c = 0; c < 16; ++c) M.w2[c] = W2[c * 64 + lane];
        M.b2 = RP[64 * 64 + lane];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) M.w3[c] = W3[c * 64 + lane];
    // layer 4: lanes past deg read lane 0's weights (their outputs are discarded), so every
    // load of the stream is unconditional and the in-order load counter can be waited on
    // exactly (exec-masked loads made the compiler wait for layer 3's weights in layer 1)
    const int l4 = lane < deg ? lane : 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) M.w4[c] = W4[c * D + l4];
    M.b3 = RP[mlp_rp_layer_floats(64) + 64 * 64 + lane];
    M.b4 = RP[2 * mlp_rp_layer_floats(64) + 64 * D + l4];
}

// mlp_preload's layer-3 and layer-4 halves (the memory-resident engine issues them apart)
__device__ __forceinline__ void mlp_preload_w3(MlpPre& M, const float* __restrict__ RP, int lane) {
    const float4* __restrict__ W3 = (const float4*)(RP + mlp_rp_layer_floats(64));
#pragma unroll
    for (int c = 0; c < 16; ++c) M.w3[c] = W3[c * 64 + lane];
    M.b3 = RP[mlp_rp_layer_floats(64) + 64 * 64 + lane];
}
__device__ __forceinline__ void mlp_preload_w4(MlpPre& M, const float* __restrict__ RP, int lane, int D, int deg) {
    const float4* __restrict__ W4 = (const float4*)(RP + 2 * mlp_rp_layer_floats(64));
    const int l4 = lane < deg ? lane : 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) M.w4[c] = W4[c * D + l4];
    M.b4 = RP[2 * mlp_rp_layer_floats(64) + 64 * D + l4];
}

// layer 1 of a decision at node v (the one-hot row too when the destination dst is
// known, has_w1): issued by the memory-resident engine's arrival handler together with
// its second round trip (previous decision record, observation), so the decision finds
// it in registers
// Layer 2's weights once rode along the arrival's second round trip too; they are issued when
// the decision starts instead (round 5: +4.8 % at config 5 -- the arrival's gather no longer waits
// behind 17 weight loads, and their 64 VGPRs are not held across the arrival's tree repair)
__device__ __forceinline__ void mlp_preload_node(MlpPre1& M, const Sim& S, uint32_t v, uint32_t dst, bool has_w1) {
    const int lane = S.lane;
    v = rfl(v);                  // uniform: the row pointers come from scalar loads
    const int D = S.lv.max_deg();
    const float* __restrict__ RP1 = S.mlp_rp + (size_t)v * mlp_rp_node_floats(D);
    const int deg = t_ovrow(S, v + 1) - t_ovrow(S, v);
    M.has_w1 = has_w1;
    M.w1v = 0.0f;
    if (has_w1 && lane < 32) M.w1v = S.mlp[((int)v * S.lv.N() + (int)dst) * 32 + (lane & 31)];
    const int j32 = lane & 31, nck = (deg + 3) >> 2;
    const float4* __restrict__ Wb4 = (const float4*)RP1;
#pragma unroll
    for (int c = 0; c < 4; ++c) M.wb[c] = (c < nck) ? Wb4[c * 32 + j32] : make_float4(0.f, 0.f, 0.f, 0.f);
    M.b1v = (lane < 32) ? RP1[128 * ((D + 3) / 4) + 32 + j32] : RP1[128 * ((D + 3) / 4) + j32];
}

__device__ __forceinline__ float mlp_dense64_pre(const Sim& S, const float4 (&w)[16], float b) {
    const float4* __restrict__ hb = (const float4*)S.hbuf;
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float4 h = hb[c];
        acc = __builtin_fmaf(h.x, w[c].x, acc);
        acc = __builtin_fmaf(h.y, w[c].y, acc);
        acc = __builtin_fmaf(h.z, w[c].z, acc);
        acc = __builtin_fmaf(h.w, w[c].w, acc);
    }
    return __fadd_rn(acc, b);
}

// Layers 2-4 of the register-resident instances with the weight loads one batch ahead: batch
// t+1's loads (across layer boundaries too) are issued before batch t's FMAs, so each L2 round
// trip overlaps a batch of FMAs instead of standing alone.  Per lane the same operations in
// the same order as mlp_dense64_pre for each layer (bit-identical); layer 4's lanes past deg read
// lane 0's weights and their outputs are discarded by the caller.
// B: float4 weight loads in flight per lane and buffer (one L2 round trip per B chunks)
template <int B>
__device__ __forceinline__ void mlp_l2_first(float4 (&w0)[B], const float* __restrict__ RP, int lane) {
    const float4* __restrict__ W4 = (const float4*)RP;
#pragma unroll
    for (int c = 0; c < B; ++c) w0[c] = W4[c * 64 + lane];
}
// w0: layer 2's first batch, issued by the caller before layer 1 (mlp_l2_first) when EARLY
// (the 256-VGPR instances: config 4 +1.2 % over issuing it here; the 128-VGPR ones lose 0.5 %)
template <int B, bool EARLY>
__device__ __forceinline__ float mlp_l234_pipe(const Sim& S, const float* __restrict__ RP, int lane, int D, int deg,
                                               const float4 (&w0)[B]) {
    constexpr int NB = 16 / B, T = 3 * NB;
    // B must divide the 16 chunks of a layer, and EARLY (issue(0) skipped: the caller issued
    // batch 0) needs a later batch of layer 2 to load its bias
    static_assert(16 % B == 0 && (!EARLY || NB >= 2), "mlp_l234_pipe: B must divide 16; EARLY needs 16 / B >= 2");
    const float4* __restrict__ hb = (const float4*)S.hbuf;
    const int l4 = lane < deg ? lane : 0;
    float4 w[2][B];
    float bias[3];
    if constexpr (EARLY) {
#pragma unroll
        for (int c = 0; c < B; ++c) w[0][c] = w0[c];
    }
    auto issue = [&](int t) {
        const int Lk = t / NB, c0 = (t % NB) * B;
        const int units = Lk < 2 ? 64 : D, ln = Lk < 2 ? lane : l4;
        const float* __restrict__ Wl = RP + Lk * mlp_rp_layer_floats(64);
        const float4* __restrict__ W4 = (const float4*)Wl;
#pragma unroll
        for (int c = 0; c < B; ++c) w[t & 1][c] = W4[(c0 + c) * units + ln];
        if (t % NB == NB - 1) bias[Lk] = Wl[64 * units + ln];
    };
    float acc = 0.0f, q = 0.0f;
    if constexpr (!EARLY) issue(0);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t + 1 < T) issue(t + 1);
        __builtin_amdgcn_sched_barrier(0);
        const int c0 = (t % NB) * B;
#pragma unroll
        for (int c = 0; c < B; ++c) {
            const float4 h = hb[c0 + c];
            acc = __builtin_fmaf(h.x, w[t & 1][c].x, acc);
            acc = __builtin_fmaf(h.y, w[t & 1][c].y, acc);
            acc = __builtin_fmaf(h.z, w[t & 1][c].z, acc);
            acc = __builtin_fmaf(h.w, w[t & 1][c].w, acc);
        }
        if (t % NB == NB - 1) {
            const int Lk = t / NB;
            const float o = det_elu(__fadd_rn(acc, bias[Lk]));
            acc = 0.0f;
            if (Lk < 2) {
                __builtin_amdgcn_wave_barrier();
                S.hbuf[lane] = o;
                __builtin_amdgcn_wave_barrier();
            } else {
                q = o;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return q;
}

// one-hot input: obs[0] (the destination's overlay index, lane 0 of obs_reg)
__device__ __forceinline__ float rdlf(float x, uint32_t k) { return __uint_as_float(rdl(__float_as_uint(x), k)); }

// tf.argmin over q of lanes 0..n-1 as the reference's scan: the first minimum (learner.py:145)
// (the register-resident instances: their degrees are small)
__device__ __forceinline__ int lane_argmin_first_seq(float q, int n) {
    int best = 0;
    float bq = rdlf(q, 0);
    for (int a = 1; a < n; ++a) {
        const float qa = rdlf(q, (uint32_t)a);
        if (qa < bq) { bq = qa; best = a; }
    }
    return best;
}

// tf.argmin over q of lanes 0..n-1, the first minimum (learner.py:145): the result of
// `best = 0; for a in 1..n-1: if q[a] < q[best]: best = a`, as one DPP reduction of an
// order-preserving key (+0 and -0 equal; a NaN past lane 0 never wins; a NaN in lane 0 wins,
// since nothing compares below it) and a ballot for the lowest lane among equal keys
__device__ __forceinline__ int lane_argmin_first(float q, int n) {
    const int lane = (int)threadIdx.x;
    uint32_t u = __float_as_uint(q);
    u = (u << 1) == 0u ? 0u : u;                                    // -0 -> +0
    uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    key = (lane >= n || (q != q)) ? 0xffffffffu : key;
    const uint32_t kmin = wave_umin_fast(key);
    const float q0 = rdlf(q, 0);
    if (q0 != q0) return 0;
    return (int)__builtin_ctzll(__ballot(key == kmin));
}

// LayerNorm and layer 1 from LDS (the memory-resident engine): the deg buffer
// values (and later their squared deviations and normalised values) sit at hbuf[0..deg-1], +0
// past the degree, and every lane reads them back as 16-B broadcasts -- the sums and the layer-1
// FMA chain run in the oracle's order on VGPR operands instead of a v_readlane per term.  A +0 term
// is an exact identity here: the sums start at +0 and add non-negative values (never -0), and
// fma(+0, w, acc) = acc for finite w and acc != -0 (acc starts at +0 and an exact cancellation
// rounds to +0).
__device__ __forceinline__ float lds_sum_ordered(const float4* hb4, int nck) {
    float4 h[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = hb4[c];                      // 32 slots, all written
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c >= nck) break;                                        // uniform
        s = __fadd_rn(s, h[c].x); s = __fadd_rn(s, h[c].y); s = __fadd_rn(s, h[c].z); s = __fadd_rn(s, h[c].w);
    }
    for (int c = 8; c < nck; ++c) {                                 // degrees beyond 32
        const float4 g = hb4[c];
        s = __fadd_rn(s, g.x); s = __fadd_rn(s, g.y); s = __fadd_rn(s, g.z); s = __fadd_rn(s, g.w);
    }
    return s;
}
// a / d for an integer d (the node's degree) with rd = RN(1/d): q = a rd and one FMA correction
// (Markstein), the correctly rounded quotient for 2^-120 <= a (and a = 0) and 1 <= d <= 64 --
// checked exhaustively over every float a in that range (scripts/checks/div_deg_exhaustive.c; a
// sample in tests/test_numerics_division.py)
__device__ __forceinline__ float div_deg(float a, float d, float rd) {
    const float q = __fmul_rn(a, rd);
    const float e = __builtin_fmaf(-q, d, a);
    return __builtin_fmaf(e, rd, q);
}

// mlp_action phase totals (timing build, scripts/timing.py)
#if PRISMA_TIMING
#define TM_MLP_START() uint64_t tq = TM_NOW(), tq1
#define TM_MLP(i) do { tq1 = TM_NOW(); S.tmlp[i] += tq1 - tq; tq = tq1; } while (0)
#else
#define TM_MLP_START() do { } while (0)
#define TM_MLP(i) do { } while (0)
#endif

// The DQN-buffer decision at node v, register-resident engine.
// B: float4 weight loads in flight per lane (StepOcc::mlp_batch), as two half batches
// (P1 is not used: this engine prefetches nothing on arrival.  The parameter stays, with the
// object the pending-decision site constructs for it: without it the 24 register-resident MLP
// kernels come out with another register allocation, as they do with `chunk` written out
// in the layer-1 loop instead of as a closure)
template <int B>
__device__ __forceinline__ int mlp_action_reg(const Sim& S, uint32_t v, uint32_t obs_reg, const MlpPre1& P1) {
    const LV& L = S.lv;
    const int lane = S.lane;
    const int N = L.N(), D = L.max_deg();
    // v (and with it deg) uniform: the row pointers then come from scalar loads.  Passed through
    // the decision record the compiler had lost that, loaded deg with vector loads and waited
    // for them behind the layer 3-4 weight stream (s_waitcnt vmcnt), and ran the LayerNorm
    // sums as exec-mask loops
    v = rfl(v);
    const float* __restrict__ W1 = S.mlp;
    const float* __restrict__ RP1 = S.mlp_rp + (size_t)v * mlp_rp_node_floats(D);
    const float* __restrict__ RP = RP1 + mlp_rp_l1_floats(D);
    TM_MLP_START();
    if (PRISMA_TP_SET == 0) TP_START();
    TP0(0);
    const int deg = t_ovrow(S, v + 1) - t_ovrow(S, v);
    const uint32_t dst = rdl(obs_reg, 0);
    // layer-1 weights first (independent of the normalisation): one W1 row element and
    // b1 for the one-hot branch (lanes 0-31), the Wb chunks and bb for the buffers branch
    // (lanes 32-63; deg <= D, so at most ceil(D/4) chunks)
    const int j32 = lane & 31;
    const int nck = (deg + 3) >> 2;
    const float4* __restrict__ Wb4 = (const float4*)RP1;
    const float w1v = (lane < 32) ? W1[((int)v * N + (int)dst) * 32 + j32] : 0.0f;
    const float b1v = (lane < 32) ? RP1[128 * ((D + 3) / 4) + 32 + j32] : RP1[128 * ((D + 3) / 4) + j32];
    float4 wb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wb[c] = (c < nck) ? Wb4[c * 32 + j32] : make_float4(0.f, 0.f, 0.f, 0.f);
    // layer 2's first weights go out now and load during the LayerNorm and layer 1
    constexpr int kPipeB = B >= 2 ? B / 2 : 1;
    constexpr bool kPipeEarly = B >= 8;
    float4 w20[kPipeB];
    if constexpr (kPipeEarly) mlp_l2_first<kPipeB>(w20, RP, lane);
    // LayerNormalization of the deg buffer values (population variance, epsilon 1e-3):
    // lane k+1 holds buffer value k; sums run in k order through readlanes
    // (the memory-resident engine's LDS form lost 0.5-1.2 % here at 4 waves per SIMD, round-5 A/B,
    // its 4-wide sums and DPP argmin 1 %, A/B on GEANT)
    const float xf = (float)obs_reg;
    float sum = 0.0f;
    for (int k = 0; k < deg; ++k) sum = __fadd_rn(sum, rdlf(xf, (uint32_t)(k + 1)));
    TP0(1);
    TP0(2);
    const float mean = __fdiv_rn(sum, (float)deg);
    const float dv = __fsub_rn(xf, mean);
    const float sq = __fmul_rn(dv, dv);
    float var = 0.0f;
    for (int k = 0; k < deg; ++k) var = __fadd_rn(var, rdlf(sq, (uint32_t)(k + 1)));
    TP0(3);
    TP0(4);
    var = __fdiv_rn(var, (float)deg);
    const float den = __fsqrt_rn(__fadd_rn(var, 1e-3f));
    const float xn = __fdiv_rn(dv, den);                          // lane k+1: normalised value k
    TP0(5);
    // layer 1: one-hot(dst) branch in lanes 0-31, buffers branch in lanes 32-63. The
    // buffers dot product runs with every lane active (lanes 0-31 discard it): its
    // readlanes read xn from lanes 1..deg, which must not sit in an inactive branch.
    float acc = 0.0f;
    auto chunk = [&](int c, const float4& w) {
        const int k = 4 * c;
        acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 1)), w.x, acc);
        if (k + 1 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 2)), w.y, acc);
        if (k + 2 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 3)), w.z, acc);
        if (k + 3 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 4)), w.w, acc);
    };
    for (int c = 0; c < nck; ++c) {
        float4 w;
        if (c < 4) {
            w = (c == 0) ? wb[0] : (c == 1) ? wb[1] : (c == 2) ? wb[2] : wb[3];
        } else {
            w = Wb4[c * 32 + j32];
        }
        chunk(c, w);
    }
    TP0(6);
    S.hbuf[lane] = det_elu(__fadd_rn(lane < 32 ? w1v : acc, b1v));
    __builtin_amdgcn_wave_barrier();
    TP0(7);
    TM_MLP(0);
    // (half batches double-buffered: the same weight registers as B loads in flight)
    const float q4 = mlp_l234_pipe<kPipeB, kPipeEarly>(S, RP, lane, D, deg, w20);
    __builtin_amdgcn_wave_barrier();
    // tf.argmin: first minimum (learner.py:145)
    return lane_argmin_first_seq(q4, deg);
}

// ---- the reduced DQN-buffer models (models.py:39-227: DQN_buffer_lite / lighter / lighter_2 /
// lighter_3; include/prisma.h PRISMA_POLICY_DQN_LITE ... _DQN_LIGHTER_3): DQN_buffer_model's
// structure with both first-layer branches B wide, NH hidden layers H wide and the deg outputs,
// B in {4, 8, 16}, H in {8, 16, 32}, NH in {1, 2}.  One instance set serves all of them: B, H and
// NH are wave-uniform run-time values (KParams::lq_dims), so every pointer and loop bound below is
// scalar.  The operation order is mlp_action_reg's with 32 -> B and 64 -> H: at
// (32, 64, 2) it would be the oracle's.
// The interleaved per-node copy (prisma_lightq_repack_kernel) is [L1][L2]([L3])[Lo]:
// * L1: the buffers branch, chunk c holding Wb[4c..4c+3][j] as one float4 per unit j < B (rows
//   k >= D zero), ceil(D / 4) chunks, then bb[B] and b1[B] (the one-hot rows of W1 stay in the
//   caller's buffer: one row per decision);
// * L2 (2B inputs, H units), L3 (H inputs, H units; NH = 2 only), Lo (H inputs, D units): chunk c
//   holding W[4c..4c+3][j] as one float4 per unit j, then the bias row.
// B and H are multiples of 4, so every section starts on a float4.
__host__ __device__ constexpr uint32_t lq_pack_dims(int B, int H, int NH) {
    return (uint32_t)B | ((uint32_t)H << 8) | ((uint32_t)NH << 16);
}
__host__ __device__ constexpr int lq_rp_l1_floats(int D, int B) { return 4 * B * ((D + 3) / 4) + 2 * B; }
__host__ __device__ constexpr int lq_rp_layer_floats(int in, int units) { return in * units + units; }
__host__ __device__ constexpr int lq_rp_node_floats(int D, int B, int H, int NH) {   // whole float4s
    return (lq_rp_l1_floats(D, B) + lq_rp_layer_floats(2 * B, H) + (NH - 1) * lq_rp_layer_floats(H, H) +
            lq_rp_layer_floats(H, D) + 3) & ~3;
}

// Layers 2.. of a reduced model as straight-line code, mlp_l234_pipe's shape: NH + 1 layers of NC
// chunks each (the three widths have B / 2 = H / 4 = NC: 8, 4, 2, so the concat and the hidden
// layers are equally deep and H = 4 NC), in batches of min(PB, NC) chunks through a ring of DEPTH
// weight buffers: batch t + DEPTH - 1's loads (across layer boundaries too) are issued before
// batch t's FMAs.  The 256-VGPR instances run 2 chunks x 3 buffers (four chunks ahead of the
// chain in 24 weight registers; 4 x 2, mlp_l234_pipe's, left the (8, 2) instance 3 VGPR spills),
// the 128-VGPR ones 1 chunk x 2 (8 registers; with 2 x 2 the (2, 1) instances spilled 9 and 12
// VGPRs, with 1 x 3 one to four, with 1 x 2 none).  NC and NH are
// template arguments so that every load, wait and FMA sits at a fixed place with no branch
// between them; lightq_action_reg picks the copy by the wave-uniform widths.  Per lane the same
// operations in the same order for each unit; the output layer's lanes past deg read lane 0's
// weights, the hidden layers' lanes past H likewise, and their results are never read.
// w0: layer 2's first half batch, issued by the caller before layer 1 when EARLY.
template <int PB, int DEPTH, int NC, int NH, bool EARLY>
__device__ __forceinline__ float lq_stream(const Sim& S, const float* __restrict__ RP, int lane, int D, int deg,
                                           const float4 (&w0)[PB]) {
    constexpr int H = 4 * NC, PBE = PB < NC ? PB : NC, NB = NC / PBE, T = (NH + 1) * NB;
    constexpr int kLayer = lq_rp_layer_floats(H, H);    // = lq_rp_layer_floats(2 B, H): 2 B = H
    static_assert(NC % PBE == 0 && DEPTH >= 2 && DEPTH - 1 <= T, "lq_stream: the batch must divide a layer's chunks");
    const float4* __restrict__ hb = (const float4*)S.hbuf;
    const int lH = lane < H ? lane : 0, lo = lane < deg ? lane : 0;
    float4 w[DEPTH][PBE];
    float bias[NH + 1];
    if constexpr (EARLY) {
#pragma unroll
        for (int c = 0; c < PBE; ++c) w[0][c] = w0[c];
        if constexpr (NB == 1) bias[0] = RP[H * H + lH];
    }
    auto issue = [&](int t) {
        const int Lk = t / NB, c0 = (t % NB) * PBE;
        const bool out = Lk == NH;
        const int U = out ? D : H, ln = out ? lo : lH;
        const float* __restrict__ Wl = RP + Lk * kLayer;
        const float4* __restrict__ W4 = (const float4*)Wl;
#pragma unroll
        for (int c = 0; c < PBE; ++c) w[t % DEPTH][c] = W4[(c0 + c) * U + ln];
        if (t % NB == NB - 1) bias[Lk] = Wl[H * U + ln];
    };
    float acc = 0.0f, q = 0.0f;
    if constexpr (!EARLY) issue(0);
#pragma unroll
    for (int t = 1; t < DEPTH - 1; ++t) issue(t);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t + DEPTH - 1 < T) issue(t + DEPTH - 1);
        __builtin_amdgcn_sched_barrier(0);
        const int c0 = (t % NB) * PBE;
#pragma unroll
        for (int c = 0; c < PBE; ++c) {
            const float4 h = hb[c0 + c];
            acc = __builtin_fmaf(h.x, w[t % DEPTH][c].x, acc);
            acc = __builtin_fmaf(h.y, w[t % DEPTH][c].y, acc);
            acc = __builtin_fmaf(h.z, w[t % DEPTH][c].z, acc);
            acc = __builtin_fmaf(h.w, w[t % DEPTH][c].w, acc);
        }
        if (t % NB == NB - 1) {
            const int Lk = t / NB;
            const float o = det_elu(__fadd_rn(acc, bias[Lk]));
            acc = 0.0f;
            if (Lk < NH) {
                __builtin_amdgcn_wave_barrier();
                S.hbuf[lane] = o;
                __builtin_amdgcn_wave_barrier();
            } else {
                q = o;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return q;
}

// The reduced models' decision at node v, register-resident engine.
// MB: float4 weight loads in flight per lane (StepOcc::mlp_batch), as in mlp_action_reg: layer 1
// holds 4 Wb chunks; the layers after it stream as half batches of MB / 2 chunks (lq_stream).
// Every weight load is unconditional: a lane past a layer's width reads lane 0's column and its
// result is never read (hbuf slots past the width; outputs past deg), and a Wb chunk past the
// node's degree reads chunk 0, so no load sits under an exec mask and the in-order load counter
// can be waited on exactly.  Activations go through the 64 floats of S.hbuf (the 256 B every MLP
// launch reserves): a layer is at most 32 wide here.
template <int MB>
__device__ __forceinline__ int lightq_action_reg(const Sim& S, uint32_t v, uint32_t obs_reg, uint32_t dims) {
    const LV& L = S.lv;
    // the lane id opaque here: every copy of the layer stream derives its own per-lane offsets
    // from it (lane < H ? lane : 0, ...), which are invariants of the event loop -- hoisted out of
    // it they sat in VGPRs across the whole loop (61 VGPR spills on the 4-wave instances)
    int lane = S.lane;
    asm volatile("" : "+v"(lane));
    const int N = L.N(), D = L.max_deg();
    // v, deg and the widths uniform: the row pointers come from scalar loads (see mlp_action_reg)
    v = rfl(v);
    dims = rfl(dims);
    const int B = (int)(dims & 0xffu), H = (int)((dims >> 8) & 0xffu), NH = (int)(dims >> 16);
    const float* __restrict__ W1 = S.mlp;
    const float* __restrict__ RP1 = S.mlp_rp + (size_t)v * lq_rp_node_floats(D, B, H, NH);
    const float* __restrict__ RP = RP1 + lq_rp_l1_floats(D, B);
    const int deg = t_ovrow(S, v + 1) - t_ovrow(S, v);
    const uint32_t dst = rdl(obs_reg, 0);
    // layer 1: one-hot branch in lanes 0..B-1, buffers branch in lanes B..2B-1 (unit lane & (B-1));
    // the lanes past 2B repeat them and write hbuf slots no layer reads
    const int jb = lane & (B - 1);
    const int nck = (deg + 3) >> 2;
    const int kc = (D + 3) >> 2;
    const float4* __restrict__ Wb4 = (const float4*)RP1;
    const float w1v = W1[((int)v * N + (int)dst) * B + jb];
    const float b1v = RP1[4 * B * kc + (lane < B ? B + jb : jb)];
    float4 wb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wb[c] = Wb4[(c < nck ? c : 0) * B + jb];
    // layer 2's first weights go out now and load during the LayerNorm and layer 1 (as
    // mlp_action_reg: the 256-VGPR instances only); a chunk past the layer's reads chunk 0, unused
    // chunks per batch x ring of buffers: 2 x 3 with 256 VGPRs, 1 x 2 with 128 (register figures of
    // the alternatives: lq_stream)
    constexpr int PB = MB >= 8 ? 2 : 1, kDepth = MB >= 8 ? 3 : 2;
    constexpr bool kEarly = MB >= 8;
    float4 w20[PB];
    if constexpr (kEarly) {
        const float4* __restrict__ W24 = (const float4*)RP;
        const int lH = lane < H ? lane : 0, nc = H >> 2;
#pragma unroll
        for (int c = 0; c < PB; ++c) w20[c] = W24[(c < nc ? c : 0) * H + lH];
    }

    // LayerNormalization of the deg buffer values, mlp_action_reg's order
    const float xf = (float)obs_reg;
    float sum = 0.0f;
    for (int k = 0; k < deg; ++k) sum = __fadd_rn(sum, rdlf(xf, (uint32_t)(k + 1)));
    const float mean = __fdiv_rn(sum, (float)deg);
    const float dv = __fsub_rn(xf, mean);
    const float sq = __fmul_rn(dv, dv);
    float var = 0.0f;
    for (int k = 0; k < deg; ++k) var = __fadd_rn(var, rdlf(sq, (uint32_t)(k + 1)));
    var = __fdiv_rn(var, (float)deg);
    const float den = __fsqrt_rn(__fadd_rn(var, 1e-3f));
    const float xn = __fdiv_rn(dv, den);                          // lane k+1: normalised value k
    // the buffers dot product with every lane active (its readlanes read lanes 1..deg)
    float acc = 0.0f;
    auto chunk = [&](int c, const float4& w) {
        const int k = 4 * c;
        acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 1)), w.x, acc);
        if (k + 1 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 2)), w.y, acc);
        if (k + 2 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 3)), w.z, acc);
        if (k + 3 < deg) acc = __builtin_fmaf(rdlf(xn, (uint32_t)(k + 4)), w.w, acc);
    };
    for (int c = 0; c < nck; ++c) {
        float4 w;
        if (c < 4) {
            w = (c == 0) ? wb[0] : (c == 1) ? wb[1] : (c == 2) ? wb[2] : wb[3];
        } else {
            w = Wb4[c * B + jb];
        }
        chunk(c, w);
    }
    S.hbuf[lane] = det_elu(__fadd_rn(lane < B ? w1v : acc, b1v));
    __builtin_amdgcn_wave_barrier();

    // layers 2..: one straight-line copy per model, picked by scalar branches on the widths (a
    // schedule with run-time chunk counts needed a scalar branch per chunk, which kept every
    // 16-B activation read in front of its four FMAs: `buffer_lite` 5 % behind `buffer` at
    // config 4; a run-time loop over the half batches waited the load counter to zero: 17 %)
    // (the markers keep the copies apart: with the common start of the `buffer_lite` and
    // `buffer_lighter` copies hoisted in front of the branch the 4-wave instances spilled 44 VGPRs)
    float q;
    if (H == 32) {
        if (NH == 2) {
            asm volatile("; buffer_lite");
            q = lq_stream<PB, kDepth, 8, 2, kEarly>(S, RP, lane, D, deg, w20);
            asm volatile("; buffer_lite end" : "+v"(q));
        } else {
            asm volatile("; buffer_lighter");
            q = lq_stream<PB, kDepth, 8, 1, kEarly>(S, RP, lane, D, deg, w20);
            asm volatile("; buffer_lighter end" : "+v"(q));
        }
    } else if (H == 16) {
        asm volatile("; buffer_lighter_2");
        q = lq_stream<PB, kDepth, 4, 1, kEarly>(S, RP, lane, D, deg, w20);
        asm volatile("; buffer_lighter_2 end" : "+v"(q));
    } else {
        asm volatile("; buffer_lighter_3");
        q = lq_stream<PB, kDepth, 2, 1, kEarly>(S, RP, lane, D, deg, w20);
        asm volatile("; buffer_lighter_3 end" : "+v"(q));
    }
    __builtin_amdgcn_wave_barrier();
    // tf.argmin: first minimum (learner.py:145)
    return lane_argmin_first_seq(q, deg);
}

// The DQN-buffer decision at node v, memory-resident engine (one wave per SIMD and VGPRs to
// spare): every weight of layers 2-4 is loaded as the decision starts (MlpPre), one round trip
// in all.  PRE: the decision follows an arrival that fetched P1 (mlp_preload_node); the pending
// decision at launch start has none and loads everything here (P1 unused).
template <bool PRE>
__device__ __forceinline__ int mlp_action_mem(const Sim& S, uint32_t v, uint32_t obs_reg, const MlpPre1& P1) {
    const LV& L = S.lv;
    const int lane = S.lane;
    const int N = L.N(), D = L.max_deg();
    // v (and with it deg) uniform: see mlp_action_reg
    v = rfl(v);
    const float* __restrict__ W1 = S.mlp;
    const float* __restrict__ RP1 = S.mlp_rp + (size_t)v * mlp_rp_node_floats(D);
    const float* __restrict__ RP = RP1 + mlp_rp_l1_floats(D);
    TM_MLP_START();
    if (PRISMA_TP_SET == 0) TP_START();
#if PRISMA_TIMING
    if constexpr (PRE) __builtin_amdgcn_s_waitcnt(0);     // the arrival's loads (probe only)
#endif
    TP0(0);
    const int deg = t_ovrow(S, v + 1) - t_ovrow(S, v);
    const uint32_t dst = rdl(obs_reg, 0);
    // layer-1 weights first (independent of the normalisation): one W1 row element and
    // b1 for the one-hot branch (lanes 0-31), the Wb chunks and bb for the buffers branch
    // (lanes 32-63; deg <= D, so at most ceil(D/4) chunks).  The row element is issued
    // before the layer 3-4 loads: the in-order load counter makes layer 1 wait for
    // everything issued before it.
    const int j32 = lane & 31;
    const int nck = (deg + 3) >> 2;
    const float4* __restrict__ Wb4 = (const float4*)RP1;
    float w1v;
    if (PRE && P1.has_w1) w1v = P1.w1v;
    else w1v = (lane < 32) ? W1[((int)v * N + (int)dst) * 32 + j32] : 0.0f;
    // buffer-branch chunks 4-7 (degrees 17-32) are loaded here, BEFORE
    // the layer 3-4 stream: the load counter is in order, so a chunk loaded inside layer 1
    // made layer 1 wait for the whole stream (and the compiler, unable to count the loop's
    // loads, waited for everything before layer 2)
    // (always issued, chunk 0 again past the node's degree: no branch for the scheduler to
    // hoist the stream's loads above)
    float4 wx[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wx[c] = Wb4[((c + 4 < nck) ? c + 4 : 0) * 32 + j32];
    __builtin_amdgcn_sched_barrier(0);
    MlpPre M;
    float b1v;
    float4 wb[4];
    if constexpr (PRE) {
        // layer 2 is issued here, and layers 3-4 in two halves inside the LayerNorm below, so
        // their issue overlaps its dependent chain instead of holding the wave in front of it
#pragma unroll
        for (int c = 0; c < 16; ++c) M.w2[c] = ((const float4*)RP)[c * 64 + lane];
        M.b2 = RP[64 * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
        b1v = P1.b1v;
#pragma unroll
        for (int c = 0; c < 4; ++c) wb[c] = P1.wb[c];
    } else {
        mlp_preload(M, RP, lane, D, deg);
        b1v = (lane < 32) ? RP1[128 * ((D + 3) / 4) + 32 + j32] : RP1[128 * ((D + 3) / 4) + j32];
#pragma unroll
        for (int c = 0; c < 4; ++c) wb[c] = (c < nck) ? Wb4[c * 32 + j32] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // LayerNormalization of the deg buffer values (population variance, epsilon 1e-3) from
    // LDS (lds_sum_ordered): lane k+1 holds buffer value k
    const float xf = (float)obs_reg;
    const float4* hb4 = (const float4*)S.hbuf;
    const bool inb = lane >= 1 && lane <= deg;
    const float fdeg = (float)deg;
    const float rdeg = __fdiv_rn(1.0f, fdeg);                       // off the sums' chain
    S.hbuf[(lane - 1) & 63] = inb ? xf : 0.0f;                      // value k at hbuf[k]
    __builtin_amdgcn_wave_barrier();
    const float sum = lds_sum_ordered(hb4, nck);
    TP0(1);
    if constexpr (PRE) {
        __builtin_amdgcn_sched_barrier(0);
        mlp_preload_w3(M, RP, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    TP0(2);
    const float mean = div_deg(sum, fdeg, rdeg);
    const float dv = __fsub_rn(xf, mean);
    const float sq = __fmul_rn(dv, dv);
    __builtin_amdgcn_wave_barrier();
    S.hbuf[(lane - 1) & 63] = inb ? sq : 0.0f;
    __builtin_amdgcn_wave_barrier();
    float var = lds_sum_ordered(hb4, nck);
    TP0(3);
    if constexpr (PRE) {
        __builtin_amdgcn_sched_barrier(0);
        mlp_preload_w4(M, RP, lane, D, deg);
        __builtin_amdgcn_sched_barrier(0);
    }
    TP0(4);
    var = div_deg(var, fdeg, rdeg);
    const float den = __fsqrt_rn(__fadd_rn(var, 1e-3f));
    const float xn = __fdiv_rn(dv, den);                          // lane k+1: normalised value k
    __builtin_amdgcn_wave_barrier();
    S.hbuf[(lane - 1) & 63] = inb ? xn : 0.0f;
    __builtin_amdgcn_wave_barrier();
    TP0(5);
    // layer 1: one-hot(dst) branch in lanes 0-31, buffers branch in lanes 32-63 (every lane
    // computes the buffers dot product, lanes 0-31 discard it): every term of a chunk (+0 past
    // the degree), the inputs as LDS broadcasts
    float acc = 0.0f;
    auto chunk4 = [&](const float4& x, const float4& w) {
        acc = __builtin_fmaf(x.x, w.x, acc);
        acc = __builtin_fmaf(x.y, w.y, acc);
        acc = __builtin_fmaf(x.z, w.z, acc);
        acc = __builtin_fmaf(x.w, w.w, acc);
    };
    float4 xh[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) xh[c] = hb4[c];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c >= nck) break;
        // chunks named at compile time (a runtime-indexed select over wb/wx put them on the stack)
        chunk4(xh[c], c < 4 ? wb[c & 3] : wx[c & 3]);
    }
    for (int c = 8; c < nck; ++c) chunk4(hb4[c], Wb4[c * 32 + j32]);
    TP0(6);
    // (det_elu_sel, the ELU without branches: +1.7 % here; the register-resident instances keep
    // det_elu)
    float h = det_elu_sel(__fadd_rn(lane < 32 ? w1v : acc, b1v));
    __builtin_amdgcn_wave_barrier();
    S.hbuf[lane] = h;
    __builtin_amdgcn_wave_barrier();
    TP0(7);
    TM_MLP(0);
    h = det_elu_sel(mlp_dense64_pre(S, M.w2, M.b2));
    __builtin_amdgcn_wave_barrier();
    S.hbuf[lane] = h;
    __builtin_amdgcn_wave_barrier();
    TP0(8);
    TM_MLP(1);
    h = det_elu_sel(mlp_dense64_pre(S, M.w3, M.b3));
    __builtin_amdgcn_wave_barrier();
    S.hbuf[lane] = h;
    __builtin_amdgcn_wave_barrier();
    TP0(9);
    TM_MLP(2);
    const float q4 = det_elu_sel(mlp_dense64_pre(S, M.w4, M.b4));
    const float q = lane < deg ? q4 : 0.0f;
    __builtin_amdgcn_wave_barrier();
    TP0(10);
    // tf.argmin: first minimum (learner.py:145), one DPP reduction (the register-resident
    // instances lost 1 % with it)
    const int best = lane_argmin_first(q, deg);
    TP0(11);
    TM_MLP(3);
    return best;
}

// wire_pop in the link's lane (lane-resident link handlers above): every lane advances ITS head
// and reads slot `its next head` of link l's wire -- in bounds for every lane, the owner's being
// the slot wanted -- and the owner commits; the arrival then needs only `head` uniform
template <int FS, int LS>
__device__ __forceinline__ void wire_pop_lane(const Sim& S, Regs<FS, LS>& R, uint32_t l) {
    const uint32_t WC = (uint32_t)S.lv.WCAP();
    const bool me = (uint32_t)S.lane == l;
    const uint32_t p0 = R.p0.v[0], p1 = R.p1.v[0];
    const uint32_t cap = S.lk_rinfo >> 16, head = p0 & 0xffffu;
    const uint32_t nh = (head + 1u == cap) ? 0u : head + 1u;
    const uint32_t w = l * WC + (nh & (WC - 1u));
    const uint32_t t = S.wt[w], s = S.wseq[w];
    R.p0.v[0] = me ? ((p0 & 0xffff0000u) | nh) : p0;
    R.p1.v[0] = me ? p1 - 0x10000u : p1;
    const bool next = me && (p1 >> 16) != 1u;                       // next packet on the wire
    R.wh_t.v[0] = next ? t : R.wh_t.v[0];
    R.wh_seq.v[0] = next ? s : R.wh_seq.v[0];
}

// the head packet leaves the wire of link l (arrival at the far end)
template <class RS>
__device__ __forceinline__ void wire_pop(const Sim& S, RS& R, const Hot& H, uint32_t l, LinkV& k) {
    const LV& L = S.lv;
    if constexpr (!RS::kMem && (PRISMA_LANE_LINKS & 4) != 0) {
        if (S.lanel) { wire_pop_lane(S, R, l); return; }
    }
    const uint32_t cap = ring_cap(S, l);
    k.head = (k.head + 1 == cap) ? 0 : k.head + 1;
    k.n_wire--;
    if (k.n_wire) {                                                 // next packet on the wire
        const uint32_t w = k.head & (uint32_t)(L.WCAP() - 1);
        wire_get(S, k, l, w, k.wh_t, k.wh_seq);
    }
    link_put<LP_WIRE>(S, R, H, l, k);
}

struct Decision {
    uint32_t x, dst, start, uid, v, d; double reward; int32_t prev; uint32_t obs, flags, last, ttl;
    int32_t r0, deg;             // register-resident engine: node v's row pointer and degree (r0 < 0: not read)
    uint32_t pact;               // a relayed packet's previous record's word 7 (its action byte: stoch_action)
};

// a control packet (or a data packet inside a tunnel) continues along the
// underlay route to `to` (Ipv4L3Protocol::IpForward through the patched
// Ipv4Interface::Send, ipv4-interface.cc:213-229)
template <class RS>
__device__ __forceinline__ void ctrl_forward(const Sim& S, RS& R, Hot& H, uint32_t v, uint32_t to,
                                             uint32_t x) {
    if (!link_send(S, R, H, ti_link(route(S, v, to)), x)) CNT_ADD(S, ctrl_dropped, 1u);
}

// PingBackPacketManager::receivePacket (ping-back-packet-manager.cc:120-144) on
// tunnel lt with the one-hop delay the ping-back carries
template <class RS>
__device__ __forceinline__ void ping_ack(const Sim& S, RS& R, Hot& H, uint32_t lt, uint32_t rnd,
                                         float delay) {
    const LV& L = S.lv;
    // the round itself (rounds in flight are less than 2^18 behind the last one sent)
    const uint32_t last = H.ping_rounds - 1u;
    const uint32_t k = last - ((last - rnd) & kRoundMask);
    // erase round k from the unacknowledged list (first match; none if already acked)
    const PingV pv = ping_get(S, R, lt);
    uint32_t lo = pv.lo;
    uint64_t mask = ((uint64_t)pv.mhi << 32) | pv.mlo;
    uint32_t pw = pv.win;
    if (k == lo) {
        if (pw >> 31) fail(H, PRISMA_EBIT_ACKORDER);               // acked bits were lost (see below)
        const uint32_t n = (uint32_t)__builtin_ctzll(~mask);       // rounds lo+1.. already acked
        lo += 1u + n;
        mask = (n >= 63u) ? 0ull : (mask >> (n + 1u));
        ping_set_lo(S, R, lt, lo, (uint64_t)__double_as_longlong(ping_send_s(L, lo)));
        ping_set_mask(S, R, lt, mask);
    } else if (k > lo) {
        const uint32_t b = k - lo - 1u;
        if (b < 64u) {
            mask |= 1ull << b;
            ping_set_mask(S, R, lt, mask);
        } else {
            pw |= 1u << 31;      // round lo is lost for good unless acked > 64 rounds late
        }
    }
    // tunnelsDelay window (MA newest delays, oldest first)
    const uint32_t MA = L.ma();
    uint32_t wn = pw & 0xffffu, wh = (pw >> 16) & 0x7fffu, slot;
    if (wn >= MA) {
        slot = wh;
        wh = (wh + 1 == MA) ? 0 : wh + 1;
    } else {
        slot = wh + wn;
        if (slot >= MA) slot -= MA;
        wn++;
    }
    const uint32_t pw_new = wn | (wh << 16) | (pw & (1u << 31));
    st_rep(S, &S.win[lt * MA + slot], delay);
    // refresh the cached window mean (data-packet-manager.cc:55-65), summed oldest first
    double sum = 0.0;
    uint32_t i = wh;
    if constexpr (RS::kMem) {
        // the memory-resident engine's windows are in HBM: one load of the whole window (lane m:
        // slot m), then the slots in order through readlanes -- one round trip instead of one per
        // slot (the loop had waited for each load in turn; round 5, config 5 +0.2 %)
        const uint32_t wl = ((uint32_t)S.lane < MA) ? ((const uint32_t*)S.win)[lt * MA + (uint32_t)S.lane] : 0u;
        for (uint32_t j = 0; j < wn; ++j) {
            const float w = (i == slot) ? delay : __uint_as_float(rdl(wl, i));
            sum += (double)w;
            i = (i + 1 == MA) ? 0 : i + 1;
        }
    } else {
        for (uint32_t j = 0; j < wn; ++j) {
            float w = (i == slot) ? delay : __uint_as_float(u_ld32((const uint32_t*)S.win + lt * MA + i));
            sum += (double)w;
            i = (i + 1 == MA) ? 0 : i + 1;
        }
    }
    ping_set_win(S, R, lt, pw_new, (uint64_t)__double_as_longlong(sum / (double)wn));
}

// ping-back delay slot of responder position pos on tunnel t (tunnelled overlays): one
// slot per overlay node on the tunnel
__device__ __forceinline__ uint32_t pbd_slot(const Sim& S, uint32_t t, uint32_t pos) {
    const uint32_t tr = S.T->tresp[t];
    return (tr & 0xffffu) + (uint32_t)__builtin_popcount((tr >> 16) & ((1u << pos) - 1u));
}

// returns 1 if a data decision needs an action
template <bool PRE = false, class RS>
__device__ __forceinline__ int on_arrive(const Sim& S, RS& R, Hot& H, uint32_t l, Decision& D, bool fused,
                                         MlpPre1& Mpre) {
    const LV& L = S.lv;
    if (S.mem) TP1_START();
    TP2_START();
    // lane-resident link handlers: the far end, its row and the ring offset are constants of link
    // l held in its lane (lane_links_bind), one v_readlane each instead of a scalar load and two
    // dependent on it
    bool topo_word = false;
    if constexpr (!RS::kMem && PRISMA_TOPO_WORD != 0) topo_word = S.lanel;
    const uint32_t tw = topo_word ? rdl(S.lk_acc, l) : 0u;
    const uint32_t v = topo_word ? (tw & 255u) : (uint32_t)t_ldst(S, l);
    LinkV k = link_get(R, l);
    const uint32_t wh = k.head & (uint32_t)(L.WCAP() - 1);
    const uint32_t x = S.mem ? wire_ent(S, k, wh)
                             : (S.tun ? u_ld32(&S.went[l * (uint32_t)L.WCAP() + wh])
                                      : u_ld32(&S.ring[(topo_word ? rdl(S.lk_rinfo, l) & 0xffffu : ring_off(S, l)) + k.head]));
    if (S.mem) TP1(0);
    TP2(0);
    const uint32_t type = ent_type(x);
    const bool tun = S.tun;
    if (relay_ip(S) && type == T_RELAY && rip_tgt(x) != v) {
        // a switch inside the packet's tunnel: IP-forwarded towards the tunnel's target
        // (packet-manager.cc:115 -> not valid, no Notify) on the entry alone
        wire_pop(S, R, H, l, k);
        const uint32_t d = H.dec, dist = relay_dist(S, d, x);
        // (a failing event consumes its packet and does nothing else: include/prisma.h)
        if (dist >= L.log_cap()) { fail(H, PRISMA_EBIT_LOGWRAP); return 0; }
        // IpForward decrements the TTL first and drops at 0 (no trace, no counter)
        const uint32_t tt = rip_ttl(x);
        if (tt == 1u) return 0;
        const uint32_t xf = tt == kRipTtlSat ? x : x - (1u << 20);
        if (!link_send(S, R, H, ti_link(route(S, v, rip_tgt(x))), xf))
            relay_dropped(S, d - dist, (record_word(S, d - dist, 24) >> 8) & 255u, v);
        return 0;
    }
    if (ent_is_data(x)) {
        // PacketRoutingEnv::NotifyPktRcv -> Notify (packet-routing-gym.cc:231-267)
        // A forwarded packet's previous decision record (t_ns, uid, dst,
        // start, deciding node + action, TTL) comes from the HBM log -- the
        // temp_obs entry of forwarder.py:153-159.  The load is issued first
        // and consumed after the link update and the observation, which do
        // not depend on it (and only on this path, so no load is ever left
        // in flight across loop iterations).
        // A fresh packet (off an access link) has no previous record: everything
        // it needs is in its ring entry.  On the register-resident engine a uniform
        // branch on the entry's type skips the two loads, and their consumers all
        // stand in the relay branch below, so a fresh arrival issues no load and
        // waits for none (skip_fresh).  Two instance sets keep the unconditional
        // load, of the slot the fresh entry's dst / parity / uid bits happen to
        // name, and ignore it: the memory-resident engine (the branch cost config 5
        // 1.3 % in alternating A/B) and the tunnelled --train instances (one of
        // them would spill 4 VGPRs).  profiles/fresh_arrival/README.md.
        const bool fresh = type == T_FRESH;
        const bool skip_fresh = !S.mem && !(S.tun && S.ctrl);      // (compile-time constants)
        const uint32_t d = H.dec;
        const uint32_t dist = relay_dist(S, d, x);
        // The previous decision is log_capacity or more decisions old: its record has been
        // overwritten.  The event consumes the packet and does nothing else -- no record, no hop,
        // no counter (include/prisma.h).  Here, ahead of the record's load: one site for every
        // instance, and no tunnel is ever picked from an overwritten record.  (The exit costs
        // the headline instance 1 to 2 % against setting the flag and executing the event, in
        // alternating A/B, wherever on this path it stands: after the link update, at the
        // record's first use, folded into the destination branch, or here.)
        if (type == T_RELAY &&__builtin_expect(dist >= L.log_cap(), 0)) {
            wire_pop(S, R, H, l, k);
            fail(H, PRISMA_EBIT_LOGWRAP);
            return 0;
        }
        const unsigned char* pr = S.logrep + (size_t)((d - dist) & (L.log_cap() - 1)) * L.rec_bytes();
        uint4 ph = make_uint4(0u, 0u, 0u, 0u);
        uint2 pw = make_uint2(0u, 0u);
        if (!skip_fresh || !fresh) {
            ph = *(const uint4*)pr;
            pw = *(const uint2*)(pr + 24);
        }
        if constexpr (PRE) {                                        // the decision's weights ride along
            if (S.ctrl) {
                mlp_preload_node(Mpre, S, v, 0u, false);
            } else {
                // the entry names the destination (engine_layout.h): no weights for a
                // packet that has arrived, the one-hot row element with the others
                const uint32_t dst_e = (type == T_FRESH) ? f_dst(x) : r_dst(x);
                if (dst_e != v) mlp_preload_node(Mpre, S, v, dst_e, true);
            }
        }
        // memory-resident engine: the observation's gather goes out with the record
        // load, before the arrival link's update (it reads node v's out-links, which
        // nothing touches before the decision)
        const uint32_t obs_early = S.mem ? observe_links(S, R, H, v, ns_to_sec(H.now)) : 0u;
        if (S.mem) TP1(1);
        TP2(1);
        wire_pop(S, R, H, l, k);
        if (S.mem) TP1(2);
        TP2(2);
        uint32_t ttl = 255u;                                        // SetIpTtl(255) (poisson-application.cc:330)
        if (tun && type == T_RELAY) {
            // Tunnelled overlay: the packet's next hop is the target of the tunnel
            // the previous decision picked; anywhere else it is only IP-forwarded
            // (packet-manager.cc:115 -> not valid, no Notify).
            const uint32_t w6p = rfl(pw.x), w7p = rfl(pw.y);
            const uint32_t u = w6p & 255u;
            const uint32_t ti = S.T->tinfo[(uint32_t)t_ovrow(S, u) + (w7p & 255u)];
            const uint32_t ttl_prev = (w7p >> 16) & 255u;
            if (ti_tgt(ti) != v) {
                // (relay_ip: the entry named this node as the target, so the record is not this
                // packet's -- the log wrapped past the 18-bit decision index)
                if (relay_ip(S)) { fail(H, PRISMA_EBIT_LOGWRAP); return 0; }
                // IpForward decrements the TTL first and drops at 0 (no trace, no counter)
                if (ttl_prev == (route(S, u, v) >> 8)) return 0;
                if (!link_send(S, R, H, ti_link(route(S, v, ti_tgt(ti))), x))
                    relay_dropped(S, d - dist, (w6p >> 8) & 255u, v);
                return 0;
            }
            ttl = ttl_prev - (ti_len(ti) - 1u);
        }
        H.dec = d + 1u;
        int r0 = -1, deg = 0;
        if (topo_word) { r0 = (int)((tw >> 8) & 255u); deg = (int)((tw >> 16) & 255u); }
        else if (!S.mem) { r0 = t_ovrow(S, v); deg = t_ovrow(S, v + 1) - r0; }
        const uint32_t obs_links = S.mem ? obs_early : observe_links(S, R, H, v, ns_to_sec(H.now), r0, deg);
        D.r0 = r0; D.deg = deg;
        int64_t t_prev = 0;
        uint32_t uid_prev = 0u, w_prev = 0u;
        if (!skip_fresh) {                                          // (the record is waited for here)
            t_prev = mk64(rfl(ph.x), rfl(ph.y));
            uid_prev = rfl(ph.z); w_prev = rfl(pw.x);
        }
        if (S.mem) TP1(3);
        TP2(3);
        double reward = 0.0;
        int32_t prev = -1;
        uint32_t dst, start, uid, last = 0u, pact = 0u;
        if (fresh) {
            // first notification: destination from the flow, uid and start
            // second rebuilt from their low bits (the packet left its app less
            // than 1 s and fewer than 2^20 injections ago)
            dst = f_dst(x);
            const uint32_t s0 = (uint32_t)(TSEC(H.now));
            start = s0 - ((s0 ^ f_parity(x)) & 1u);
            const uint32_t lu = H.uid - 1u;
            uid = lu - ((lu - f_uid(x)) & kUidMask);
        } else {
            prev = (int32_t)(d - dist);                             // (dist < log_cap: checked above)
            if (skip_fresh) {                                       // the record is first waited for here
                t_prev = mk64(rfl(ph.x), rfl(ph.y));
                uid_prev = rfl(ph.z); w_prev = rfl(pw.x);
            }
            pact = rfl(pw.y);
            uid = uid_prev;
            dst = (w_prev >> 8) & 255u;
            start = w_prev >> 16;
            last = w_prev & 255u;
            // reward = us_to_sec(py_micros(now)) - us_to_sec(py_micros(t_prev)) (forwarder.py:360):
            // the two clock terms in lanes 0 and 1 of one vector
            // evaluation -- now in even lanes, the previous decision's time in odd ones -- and
            // lane 0 takes the difference with lane 1's term brought over by a DPP move
            const uint32_t m = S.m1;                                      // -(lane & 1)
            const int64_t tt = mk64((lo32(t_prev) & m) | (lo32(H.now) & ~m), (hi32(t_prev) & m) | (hi32(H.now) & ~m));
            const double us = us_to_sec(py_micros(tt));
            const uint64_t ub = (uint64_t)__double_as_longlong(us);
            const double up = __longlong_as_double((long long)mk64(dpp_u32<0xB1, 0xF>((uint32_t)ub),
                                                                   dpp_u32<0xB1, 0xF>((uint32_t)(ub >> 32))));
            const uint64_t rb = (uint64_t)__double_as_longlong(us - up);
            reward = __longlong_as_double((long long)mk64(rfl((uint32_t)rb), rfl((uint32_t)(rb >> 32))));
            CNT_ADD(S, reward_sum, reward);
        }
        // obs[0] = m_map_overlay_array[dst] (the identity on identity overlays)
        const uint32_t o = (S.lane == 0) ? (tun ? (uint32_t)S.T->ovi[dst] : dst) : obs_links;
        CNT_ADD(S, decisions, 1u);
        // --train: the answer to this notification also echoes a small-signalling
        // packet to the last hop, unless this node is the packet's source (:303-306)
        const uint32_t echo = (S.ctrl && L.train() && v != ent_src(x, v)) ? PEND_ECHO : 0u;
        D.x = x; D.dst = dst; D.start = start; D.uid = uid; D.v = v; D.d = d; D.reward = reward; D.prev = prev;
        D.obs = o; D.flags = echo; D.last = last; D.ttl = ttl; D.pact = skip_fresh ? pact : rfl(pw.y);
        if (dst == v) {                                             // getGameOver
            write_record(S, H, d, reward, uid, prev, v, dst, start, -1, PRISMA_ST_DESTINATION, o, ttl);
            if (!fused && S.ctrl && L.notify_dest()) {              // the agent is notified (done=True)
                D.flags |= PEND_DEST;
                return 1;
            }
            if (echo) send_echo(S, R, H, (uint32_t)t_lrev(S, l), uid, last);
            receive_counters(S, R, H, x, true, start, 0u);
            return 0;
        }
        if (!fused) write_record(S, H, d, reward, uid, prev, v, dst, start, -1, PRISMA_ST_PENDING, o, ttl);
        if (S.mem) TP1(4);
        TP2(4);
        return 1;
    }
    wire_pop(S, R, H, l, k);
    if (S.mem) TP1(5);
    TP2(5);
    if (S.ctrl && ent_is_big(x)) {                                  // (only with --signaling and --train)
        const uint32_t bp = t_bpair(S, g_gen(x));
        const uint32_t src = bp_src(bp), dst = bp_dst(bp);
        if (v == src) {                  // from the traffic node: IP-forwarded towards its destination
            if (!link_send(S, R, H, bp_link(bp), x)) CNT_ADD(S, ctrl_dropped, 1u);
            return 0;
        }
        if (tun && v != dst) { ctrl_forward(S, R, H, v, dst, x); return 0; }
        // BigSignalingPacketManager::receivePacket (big-signaling-packet-manager.cc:93-108):
        // at its destination, not its source -> Notify; obs [1000] (+ NN / segment index, sender)
        if (!fused && L.notify_dest()) {
            const uint32_t n = g_n(x), ns = t_bs_nseg(S);
            const uint32_t nn = ns <= 1u ? n : n / ns, seg = ns <= 1u ? 0u : n % ns;
            const uint32_t so = 0x10000u | (tun ? (uint32_t)S.T->ovi[src] : src);
            D.x = x; D.v = v; D.uid = 0u; D.flags = PEND_CTRL; D.last = 0u;
            D.obs = (S.lane == 0) ? 1000u : ((S.lane == 1) ? nn : ((S.lane == 2) ? seg : ((S.lane == 3) ? so : 0u)));
            return 1;
        }
        receive_counters(S, R, H, x, false, 0u, l);
        return 0;
    }
    if (S.ctrl && ent_is_echo(x)) {                                 // (echoes exist only with --train)
        const uint32_t to = e_to(x);
        if (tun && to != v) { ctrl_forward(S, R, H, v, to, x); return 0; }
        // SmallSignalingPacketManager::receivePacket (small-signaling-packet-manager.cc:86-94):
        // addressed to this node, so valid -> Notify; the agent sees obs [1000]
        if (!fused && S.ctrl && L.notify_dest()) {
            D.x = x; D.v = v; D.uid = e_uid(x); D.flags = PEND_CTRL; D.last = 0u;
            const uint32_t sz = ent_size(S, x, l);
            D.obs = (S.lane == 0) ? 1000u : ((S.lane == 1) ? e_uid(x) : ((S.lane == 2) ? sz : 0u));
            return 1;
        }
        receive_counters(S, R, H, x, false, 0u, l);
        return 0;
    }
    // pings.  NotifyPktRcv hands every ping seen on an overlay node's devices to
    // its managers, addressed to it or not (packet-routing-gym.cc:254-259); the
    // packet itself continues to its addressee (IP forwarding).
    const uint32_t t = p_tunnel(x), rnd = p_round(x);
    const uint32_t ti = tun ? (uint32_t)S.T->tinfo[t] : 0u;
    const bool ovl = !tun || S.T->ovi[v] >= 0;
    if (type == T_PFWD) {                                           // ping-forward-packet-manager.cc:94-156
        const uint32_t tgt = tun ? ti_tgt(ti) : v;
        if (ovl) {
            // responder position on the tunnel: its own delay slot
            const uint32_t pos = tun ? (route(S, ti_org(ti), v) >> 8) - 1u : 0u;
            const float delay = (float)(ns_to_sec(H.now) - ping_send_s(L, rnd));
            const uint32_t slot = tun ? pbd_slot(S, t, pos) : t;
            st_rep(S, &S.pbd[slot * L.PBK() + (rnd & (L.PBK() - 1))], delay);
            if (!link_send(S, R, H, (uint32_t)t_lrev(S, l), p_make(T_PBACK, t, pos, rnd))) CNT_ADD(S, ctrl_dropped, 1u);
        }
        if (tgt != v) { ctrl_forward(S, R, H, v, tgt, x); return 0; }
    } else {                                                        // ping-back-packet-manager.cc:120-144
        const uint32_t org = tun ? ti_org(ti) : v;
        if (ovl) {
            const uint32_t slot = tun ? pbd_slot(S, t, p_pos(x)) : t;
            const float delay = __uint_as_float(u_ld32((const uint32_t*)S.pbd + slot * L.PBK() + (rnd & (L.PBK() - 1))));
            if (!tun) {
                ping_ack(S, R, H, t, rnd, delay);                  // identity: tunnel == link
            } else {
                // the ORIGIN's tunnel index applied to this node's own tunnel list
                const uint32_t idx = t - (uint32_t)t_ovrow(S, org);
                const uint32_t v0 = (uint32_t)t_ovrow(S, v);
                if (idx >= (uint32_t)t_ovrow(S, v + 1) - v0) fail(H, PRISMA_EBIT_PINGIDX);
                else ping_ack(S, R, H, v0 + idx, rnd, delay);
            }
        }
        if (org != v) { ctrl_forward(S, R, H, v, org, x); return 0; }
    }
    receive_counters(S, R, H, x, false, 0u, l);
    if (S.mem) TP1(6);
    TP2(6);
    return 0;
}

// ---------------------------------------------------------------------------
// replica (re)initialisation: LDS image zeroed, registers set (all lanes)
// ---------------------------------------------------------------------------
// keep_totals: carry the header's hops_total / events_total over (auto-reset)
template <int FS, int LS>
// rng / r: the ns-3 stream table and the replica's local index (null: Philox streams)
__device__ __forceinline__ void init_replica(Sim& S, Regs<FS, LS>& R, Hot& H, uint32_t episode, bool keep_totals,
                                             const uint32_t* rng, uint32_t r) {
    const LV& L = S.lv;
    const int lane = S.lane;
    uint32_t dec = H.dec, hl = H.hops_launch, el = H.ev_launch;
    const uint64_t ht = keep_totals ? (uint64_t)u_ld64((const int64_t*)&S.h->hops_total) : 0u;
    const uint64_t et = keep_totals ? (uint64_t)u_ld64((const int64_t*)&S.h->events_total) : 0u;
    __syncthreads();
    uint4* st4 = (uint4*)S.base;
    for (uint32_t i = (uint32_t)lane; i < L.lds_state_bytes() / 16u; i += kWave) st4[i] = make_uint4(0, 0, 0, 0);
    const uint32_t* rep = rng ? rng + 18u * kMrgPowers + kMrgRepWords * r : nullptr;
    if (rng) {
        __syncthreads();
        ns3_init_lds(S, rng, rep);
    }
    // big-signalling generators: flow slot F (on_bsig), each generator started right after its
    // flow (sim.cc:599-647: the start events in install order, fseq)
    const bool bsig = S.ctrl && !S.mem;
    const uint32_t nbs = bsig ? S.T->n_bsig : 0u;
#pragma unroll
    for (int j = 0; j < FS; ++j) {
        uint32_t f = (uint32_t)lane + 64u * j;
        int64_t t = INT64_MAX;
        uint32_t s = 0xffffffffu;
        if (f < (uint32_t)L.F()) {
            double U;
            if (rng) {
                U = ns3_start_u01(rng, rep, f);
            } else {
                uint32_t c[4] = { f, 0u, episode, 0u };
                philox4x32_10(c, L.seed_lo(), S.gid);
                uint64_t u53 = ((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6);
                U = (double)u53 * (1.0 / 9007199254740992.0);
            }
            t = sec_to_ns(0.0001 + U);                              // sim.cc:610-630
            s = bsig ? S.T->fseq[f] : (uint32_t)L.NO() + f;    // after the NO ping timers
        } else if (nbs && f == (uint32_t)L.F()) {
            t = sec_to_ns(0.0001);                                  // AppStartTime (sim.cc:244, 645)
            s = S.T->fseq[f];                                       // generator 0's start
        }
        R.fk_lo.v[j] = lo32(t); R.fk_hi.v[j] = hi32(t); R.fk_seq.v[j] = s; R.f_draw.v[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < LS; ++j) {
        R.cp_t.v[j] = 0; R.cp_seq.v[j] = 0; R.wh_t.v[j] = 0; R.wh_seq.v[j] = 0;
        R.p0.v[j] = 0; R.p1.v[j] = 0; R.p2.v[j] = 0; R.qb.v[j] = 0;
        R.pm_lo.v[j] = 0; R.pm_mlo.v[j] = 0; R.pm_mhi.v[j] = 0; R.pm_win.v[j] = 0;
        R.pav_lo.v[j] = 0; R.pav_hi.v[j] = 0;
        uint64_t od = __double_as_longlong(ping_send_s(L, 0));
        R.od_lo.v[j] = (uint32_t)od; R.od_hi.v[j] = (uint32_t)(od >> 32);
    }
    H.now = 0;
    H.ping_t = L.ping_period();                                       // data-packet-manager.cc:118-121
    H.ping_seq = 0;
    H.seq = (uint32_t)L.NO() + (uint32_t)L.F() + nbs;
    H.uid = 0; H.ping_rounds = 0; H.pend = 0; H.over = 0; H.error = 0; H.stop = 0;
    H.dec = dec; H.hops_launch = hl; H.ev_launch = el;
    H.episode = episode;
    if (lane == 0) {
        S.c->episode = episode;
        S.h->hops_total = ht;
        S.h->events_total = et;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// wave-wide reductions to lane 63 (DPP row/bank steps)
// ---------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int64_t dpp_min_i64(int64_t v) {
    uint32_t lo = dpp_u32<CTRL, ROW_MASK>(lo32(v));
    uint32_t hi = dpp_u32<CTRL, ROW_MASK>(hi32(v));
    int64_t o = mk64(lo, hi);
    return o < v ? o : v;
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
    v = dpp_min_i64<0xB1, 0xF>(v);      // quad_perm [1,0,3,2]
    v = dpp_min_i64<0x4E, 0xF>(v);      // quad_perm [2,3,0,1]
    v = dpp_min_i64<0x141, 0xF>(v);     // row_half_mirror
    v = dpp_min_i64<0x140, 0xF>(v);     // row_mirror
    v = dpp_min_i64<0x142, 0xA>(v);     // row_bcast:15
    v = dpp_min_i64<0x143, 0xC>(v);     // row_bcast:31
    return mk64(rdl(lo32(v), 63), rdl(hi32(v), 63));
}

// One DPP step of an unsigned min, folded by the compiler into v_min_u32
// with a DPP source: rows outside ROW_MASK see the identity (~0u).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_umin(uint32_t v) {
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xf, false);
    return o < v ? o : v;
}

__device__ __forceinline__ uint32_t wave_umin_fast(uint32_t v) {
    v = dpp_umin<0xB1, 0xF>(v);
    v = dpp_umin<0x4E, 0xF>(v);
    v = dpp_umin<0x141, 0xF>(v);
    v = dpp_umin<0x140, 0xF>(v);
    v = dpp_umin<0x142, 0xA>(v);
    v = dpp_umin<0x143, 0xC>(v);
    return rdl(v, 63);
}

// Next event = min (time, seq) over every source of the replica, as 32-bit
// offsets from the clock: each lane reduces the sources it owns
// lexicographically on (offset, seq), the wave reduces the lane minima with
// fused DPP min steps.  Link events are always < 2^31 ns ahead; a flow or the
// ping timer further than 2^32-2 ns ahead saturates, and if every source
// saturates the exact 64-bit reduction over flows and ping runs instead.
__device__ __forceinline__ void key_take(uint32_t k, uint32_t s, uint32_t c, uint32_t& bk, uint32_t& bs,
                                         uint32_t& bc) {
    // (offset, seq) as one 64-bit key: one compare and three selects.  Written as
    // `k < bk || (k == bk && s < bs)` the short-circuit became exec-mask branches, ~20 scalar
    // instructions per event selection (A/B: +3.7 % at the headline, +2.3 % at configs 3 and 4)
    const bool t = (((uint64_t)k << 32) | s) < (((uint64_t)bk << 32) | bs);
    bk = t ? k : bk;
    bs = t ? s : bs;
    bc = t ? c : bc;
}

__device__ __forceinline__ uint32_t sat_offset(int64_t t, int64_t now) {
    const uint64_t dt = (uint64_t)(t - now);
    return (dt >> 32) ? 0xffffffffu : (uint32_t)dt;
}

template <int FS, int LS>
__device__ __forceinline__ void select_event(const Sim& S, const Regs<FS, LS>& R, const Hot& H, int lane, int64_t& bt,
                                             uint32_t& bc, uint32_t& bs) {
    // flows and the ping timer: each lane's cached earliest (flow_min_refresh), then one offset
    int64_t ft = R.fm_t;
    uint32_t s = R.fm_s, c = R.fm_c;
    uint32_t k = sat_offset(ft, H.now);
    // links: 32-bit offsets
    const uint32_t n0 = lo32(H.now);
#pragma unroll
    for (int j = 0; j < LS; ++j) {
        // each lane derives its links' candidates from their state: the completion while
        // packets wait behind the transmitter (elided otherwise, lazy_due), the wire head's
        // arrival while the wire holds packets -- no stored key to maintain in link_put
        // (A/B: +5.4 % at the headline, +6 % at config 3)
        const uint32_t p2 = R.p2.v[j];
        const bool cpv = (p2 >> 16) != 0u && (p2 & 0xffffu) != 0u;
        const bool whv = (R.p1.v[j] >> 16) != 0u;
        const uint32_t oc = cpv ? R.cp_t.v[j] - n0 : 0xffffffffu;
        const uint32_t ow = whv ? R.wh_t.v[j] - n0 : 0xffffffffu;
        const uint32_t code = (uint32_t)(lane + 64 * j);
        key_take(oc, R.cp_seq.v[j], (K_COMPLETE << 28) | code, k, s, c);
        key_take(ow, R.wh_seq.v[j], (K_ARRIVE << 28) | code, k, s, c);
    }
    const uint32_t kmin = wave_umin_fast(k);
    if (kmin != 0xffffffffu) {
        bt = H.now + (int64_t)kmin;
        const bool tie = (k == kmin);
        const uint64_t tied = __ballot(tie);
        uint32_t win;
        if (__builtin_popcountll(tied) == 1) {
            win = (uint32_t)__builtin_ctzll(tied);
        } else {                                                    // same-ns events: ns-3 uid order
            const uint32_t smin = wave_umin_fast(tie ? s : 0xffffffffu);
            win = (uint32_t)__builtin_ctzll(__ballot(tie && s == smin));
        }
        bc = rdl(c, win);
        bs = rdl(s, win);
        return;
    }
    // every source is >= 2^32-1 ns away (or none is pending): exact 64-bit path
    int64_t t = INT64_MAX;
    uint32_t s2 = 0xffffffffu, c2 = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < FS; ++j) {
        int64_t tj = mk64(R.fk_lo.v[j], R.fk_hi.v[j]);
        uint32_t sj = R.fk_seq.v[j];
        if (key_less(tj, sj, t, s2)) { t = tj; s2 = sj; c2 = (K_FLOW << 28) | (uint32_t)(lane + 64 * j); }
    }
    if (lane == 0 && key_less(H.ping_t, H.ping_seq, t, s2)) { t = H.ping_t; s2 = H.ping_seq; c2 = K_PING << 28; }
    bt = wave_min_i64(t);
    const bool tie = (t == bt);
    const uint64_t tied = __ballot(tie);
    uint32_t win;
    if ((tied & (tied - 1)) == 0) {
        win = (uint32_t)__builtin_ctzll(tied);
    } else {
        const uint32_t smin = wave_umin_fast(tie ? s2 : 0xffffffffu);
        win = (uint32_t)__builtin_ctzll(__ballot(tie && s2 == smin));
    }
    bc = rdl(c2, win);
    bs = rdl(s2, win);
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// the [N][N] action table (table policy) sits in LDS after the state image, or in HBM
__device__ __forceinline__ int table_action(const Sim& S, uint32_t i) {
    return (int)rfl(S.tab_lds ? (uint32_t)S.table[i] : (uint32_t)S.table_g[i]);
}

__device__ __forceinline__ void stage_table(unsigned char* lds, const KParams& P, int lane) {
    CLayout& LC = *(CLayout*)P.lay;
    if (P.table && LC.table_in_lds) {
        uint8_t* dstp = lds + LC.lds_state_bytes;
        const uint32_t nt = (uint32_t)(LC.N * LC.N);
        for (uint32_t i = (uint32_t)lane; i < nt; i += kWave) dstp[i] = P.table[i];
    }
}

// Epsilon-greedy exploration (prisma_run_explore, the EXPL instances; include/prisma.h states
// the rule): data decision d of episode e at node v takes a uniform pick over v's deg overlay
// neighbours instead of the greedy action g when the top 24 bits of its Philox draw fall below
// thr[v].  Counter word 3 = 2 keeps the draw apart from the flow start offsets (0) and the send
// delays (1).  d, v and thr[v] are wave-uniform, so the branch is scalar; the rounds run on the
// vector unit as in flow_next (the values pass through VGPRs) and the two words used come back
// with readfirstlane.  A node with thr = 0 never explores and skips the draw.
__device__ __forceinline__ int explore_action(const Sim& S, const Hot& H, const uint32_t* __restrict__ thr,
                                              uint32_t d, uint32_t v, int g) {
    v = rfl(v);
    const uint32_t t = rfl(thr[v]);
    if (t == 0u) return g;
    uint32_t c[4] = { rfl(d), 0u, H.episode, 2u };
    uint32_t k0 = S.lv.seed_lo(), k1 = S.gid;
    asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(k0), "+v"(k1));
    philox4x32_10(c, k0, k1);
    const uint32_t c0 = rfl(c[0]), c1 = rfl(c[1]);
    if ((c0 >> 8) >= t) return g;
    const uint32_t deg = (uint32_t)(t_ovrow(S, v + 1) - t_ovrow(S, v));
    return (int)(uint32_t)(((uint64_t)c1 * deg) >> 32);
}

// History-weighted ("smart") exploration (prisma_run_explore_smart, the smart instances;
// include/prisma.h states the rule): the same draw and hit test as explore_action, but a hit
// picks action i with probability w_i / W, w_i = nb - h_i, nb = sum h, W = (deg - 1) nb, over the
// node's row of the caller's per-replica action counts, and every data decision with a valid
// action -- explored or greedy, thr = 0 included -- adds one to its count.
//
// The hit branch is scalar (d, v, thr[v] and the draw are wave-uniform), so all 64 lanes are
// active in it.  Lane i < deg loads h_i (one coalesced load; lanes >= deg load nothing and
// contribute 0); one inclusive 64-bit DPP scan of h gives P_i = h_0 + ... + h_i, whose last lane is
// nb (the reduction), and the prefix of the weights follows without a second scan:
// w_0 + ... + w_i = (i + 1) nb - P_i for i < deg, and W from lane deg - 1 on.  A ballot of
// prefix > u plus find-first is the pick: u < W, so a lane below deg always matches first.
//
// The count is bumped by lane a, with the address lane a also loads from, and both accesses are
// relaxed agent-scope atomics: the add is executed in L2 and the loads bypass the CU's L1, so a
// pick sees the wave's own earlier increments (same thread, same address: coherence order).
// Only replica r's wave touches hist[r].
template <class T> __device__ __forceinline__ T* rfl_ptr(T* p) {     // a wave-uniform pointer, into SGPRs
    return (T*)mk64(rfl(lo32((int64_t)p)), rfl(hi32((int64_t)p)));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp_scan_step_u64(uint64_t v) {
    // lanes with no source (row start, masked rows) take 0
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + (uint64_t)mk64(lo, hi);
}
// inclusive prefix sum over the 64 lanes (all active)
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v) {
    v = dpp_scan_step_u64<0x111, 0xF>(v);   // row_shr:1
    v = dpp_scan_step_u64<0x112, 0xF>(v);   // row_shr:2
    v = dpp_scan_step_u64<0x114, 0xF>(v);   // row_shr:4
    v = dpp_scan_step_u64<0x118, 0xF>(v);   // row_shr:8
    v = dpp_scan_step_u64<0x142, 0xA>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_scan_step_u64<0x143, 0xC>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}

__device__ __forceinline__ int smart_explore_action(const Sim& S, const Hot& H, const uint32_t* __restrict__ thr,
                                                    uint32_t* hist, int r, uint32_t d, uint32_t v, int g) {
    v = rfl(v);
    const uint32_t t = rfl(thr[v]);
    const uint32_t r0 = rfl((uint32_t)t_ovrow(S, v));
    const uint32_t deg = rfl((uint32_t)t_ovrow(S, v + 1)) - r0;
    const uint32_t lane = (uint32_t)S.lane;
    // the node's row of this replica's counts
    uint32_t* row = hist + (size_t)(uint32_t)r * rfl((uint32_t)t_ovrow(S, (uint32_t)S.lv.N())) + r0;
    uint32_t a = (uint32_t)g;
    if (t != 0u) {
        uint32_t c[4] = { rfl(d), 0u, H.episode, 2u };
        uint32_t k0 = S.lv.seed_lo(), k1 = S.gid;
        asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(k0), "+v"(k1));
        philox4x32_10(c, k0, k1);
        const uint32_t c0 = rfl(c[0]), c1 = rfl(c[1]), c2 = rfl(c[2]);
        if ((c0 >> 8) < t) {
            uint32_t h = 0u;
            if (lane < deg) h = __hip_atomic_load(row + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t ps = wave_scan_u64((uint64_t)h);
            const uint64_t nb = (uint64_t)mk64(rdl((uint32_t)ps, 63u), rdl((uint32_t)(ps >> 32), 63u));
            const uint64_t W = (uint64_t)(deg - 1u) * nb;
            if (W == 0u) {
                a = (uint32_t)(((uint64_t)c1 * deg) >> 32);
            } else {
                const uint64_t u = __umul64hi(((uint64_t)c1 << 32) | c2, W);
                const uint32_t n = lane < deg ? lane + 1u : deg;
                a = (uint32_t)__builtin_ctzll(__ballot((uint64_t)n * nb - ps > u));
            }
        }
    }
    if (lane == a && a < deg) (void)__hip_atomic_fetch_add(row + lane, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (int)a;
}

// Stochastic multipath routing (prisma_run_stochastic, the stoch instances; include/prisma.h
// states the rule): the reference's "opt" agent.  tab[s][t][:] holds, per overlay edge in the
// action-history order, a class in bits 24-31 and a 24-bit weight in bits 0-23.  A packet follows
// the first edge of the deciding node whose class equals that of the edge its previous decision
// took (the reference's per-packet tag, which is always that edge's fraction); otherwise it draws
// an edge by the weights of the node's row.
//
// Every operand is wave-uniform, so all 64 lanes are active throughout.  Lane i < deg loads its
// entry (one coalesced load; lanes >= deg contribute 0), the previous edge's entry is one uniform
// load, a ballot of class matches plus find-first is the follow branch, and the draw is one
// inclusive 32-bit DPP scan of the weights (W in lane 63; deg <= 55 weights below 2^24, so no
// carry) with a ballot of prefix > u plus find-first: u < W, so a lane below deg matches first.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_scan_step_u32(uint32_t v) {
    // lanes with no source (row start, masked rows) take 0
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// inclusive prefix sum over the 64 lanes (all active)
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v) {
    v = dpp_scan_step_u32<0x111, 0xF>(v);   // row_shr:1
    v = dpp_scan_step_u32<0x112, 0xF>(v);   // row_shr:2
    v = dpp_scan_step_u32<0x114, 0xF>(v);   // row_shr:4
    v = dpp_scan_step_u32<0x118, 0xF>(v);   // row_shr:8
    v = dpp_scan_step_u32<0x142, 0xA>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_scan_step_u32<0x143, 0xC>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}

// The source of the packet whose previous decision is record p, on the instances whose relay
// entries carry no source (relay_ip): the node of the first record of the packet's `prev` chain.
// Every link must point backwards and stay inside the log as seen from decision d; a chain that
// does not (its head has been overwritten) returns kNoLink.
__device__ __forceinline__ uint32_t stoch_chain_src(const Sim& S, uint32_t d, uint32_t p) {
    for (;;) {
        const uint32_t q = record_word(S, p, 12);
        if ((int32_t)q < 0) return record_word(S, p, 24) & 255u;
        if (q >= p || d - q >= S.lv.log_cap()) return kNoLink;
        p = q;
    }
}

// d, v, dst: the decision, its node and the packet's destination; x: the arriving entry; prev: the
// previous decision's record index, or < 0 for a fresh packet; pu, pa: that record's node and
// action byte (ignored when prev < 0)
__device__ __forceinline__ int stoch_action(const Sim& S, Hot& H, const uint32_t* __restrict__ tab, uint32_t d,
                                            uint32_t v, uint32_t dst, uint32_t x, int32_t prev, uint32_t pu,
                                            uint32_t pa) {
    v = rfl(v); dst = rfl(dst); x = rfl(x); pu = rfl(pu); pa = rfl(pa);
    const bool has_prev = (int32_t)rfl((uint32_t)prev) >= 0;
    const uint32_t lane = (uint32_t)S.lane;
    const uint32_t NN = (uint32_t)S.lv.N(), NO = (uint32_t)S.lv.NO();
    uint32_t src = ent_src(x, v);
    if (relay_ip(S) && has_prev) {
        src = stoch_chain_src(S, rfl(d), rfl((uint32_t)prev));
        if (src == kNoLink) { fail(H, PRISMA_EBIT_LOGWRAP); return -1; }
    }
    const uint32_t si = S.tun ? rfl((uint32_t)S.T->ovi[src & 255u]) : src;
    const uint32_t ti = S.tun ? rfl((uint32_t)S.T->ovi[dst & 255u]) : dst;
    const uint32_t r0 = rfl((uint32_t)t_ovrow(S, v));
    const uint32_t deg = rfl((uint32_t)t_ovrow(S, v + 1)) - r0;
    const bool ok = si < NO && ti < NO;             // (always: flows run between overlay nodes)
    const uint32_t* st = tab + (size_t)(si * NO + ti) * rfl((uint32_t)t_ovrow(S, NN));
    uint32_t e = 0u;
    if (ok && lane < deg) e = st[r0 + lane];
    uint32_t c_prev = 0u;
    if (ok && has_prev && pu < NN) {
        const uint32_t p0 = rfl((uint32_t)t_ovrow(S, pu));
        if (pa < rfl((uint32_t)t_ovrow(S, pu + 1)) - p0) c_prev = rfl(st[p0 + pa]) >> 24;
    }
    if (c_prev != 0u) {
        const uint64_t m = __ballot(lane < deg && (e >> 24) == c_prev);
        if (m) return (int)__builtin_ctzll(m);
    }
    uint32_t c[4] = { rfl(d), 0u, H.episode, 3u };
    uint32_t k0 = S.lv.seed_lo(), k1 = S.gid;
    asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(k0), "+v"(k1));
    philox4x32_10(c, k0, k1);
    const uint32_t c1 = rfl(c[1]);
    const uint32_t ps = wave_scan_u32(e & 0xffffffu);
    const uint32_t W = rdl(ps, 63u);
    if (W == 0u) return (int)(uint32_t)(((uint64_t)c1 * deg) >> 32);
    const uint32_t u = (uint32_t)(((uint64_t)c1 * W) >> 32);
    return (int)__builtin_ctzll(__ballot(ps > u));
}

template <int FS, int LS>
__device__ __forceinline__ void stage_in(unsigned char* lds, const KParams& P, int r, int lane, Regs<FS, LS>& R) {
    CLayout& LC = *(CLayout*)P.lay;
    stage_table(lds, P, lane);
    const unsigned char* img = P.state + (size_t)r * LC.state_bytes;
    const uint4* s4 = (const uint4*)img;
    uint4* d4 = (uint4*)lds;
    for (uint32_t i = (uint32_t)lane; i < LC.lds_state_bytes / 16u; i += kWave) d4[i] = s4[i];
    regs_io(R, (uint32_t*)(const_cast<unsigned char*>(img) + LC.s_regs), lane, false);
}

template <int FS, int LS>
__device__ __forceinline__ void stage_out(unsigned char* lds, const KParams& P, int r, int lane, Regs<FS, LS>& R) {
    CLayout& LC = *(CLayout*)P.lay;
    unsigned char* img = P.state + (size_t)r * LC.state_bytes;
    uint4* s4 = (uint4*)img;
    const uint4* d4 = (const uint4*)lds;
    for (uint32_t i = (uint32_t)lane; i < LC.lds_state_bytes / 16u; i += kWave) s4[i] = d4[i];
    regs_io(R, (uint32_t*)(img + LC.s_regs), lane, true);
}

__device__ __forceinline__ void publish_counters(const Sim& S, const KParams& P, int r, int lane) {
    const uint32_t* src = (const uint32_t*)S.c;
    uint32_t* dst = (uint32_t*)(P.cnt_out + r);
    if (lane < (int)(sizeof(prisma_counters_t) / 4)) dst[lane] = src[lane];
}

// ---------------------------------------------------------------------------
// Episode boundaries inside a fused launch (prisma_run with auto_reset, register-resident
// engine): main.py:111-114 runs the episodes back to back, so a replica whose episode ends
// (Simulator::Stop at simTime, sim.cc:703) with hop budget left starts its next episode in the
// same launch and spends the rest of its budget there.  The next episode's fresh image (LDS
// part + register part) is built ahead of time by the reset kernel into P.spare, so the restart
// is a copy: the LDS image and the registers are reloaded from it, and the log position and
// the running totals carried over.  The step kernel then runs a second inlined copy of the
// event loop (step_kernel.h).  Restarting inside the first loop instead -- its clock and
// sequence numbers then get a second incoming value -- cost the hot loop ~20 VGPRs and 13 %
// (A/B, profiles/r03a); so did Philox draws in the loop, an outer loop around it or an
// out-of-line call (scripts/asm_headline.sh: 24-60 VGPR spills).  Without a valid spare (a
// second episode end in one launch) the replica stops at the end and the reset kernel after
// the launch starts its next episode.
// ---------------------------------------------------------------------------
template <int FS, int LS>
__device__ __forceinline__ bool spare_restart(const KParams& P, Sim& S, Regs<FS, LS>& R, int r, uint32_t done,
                                              uint32_t& budget) {
    CLayout& LC = *(CLayout*)P.lay;
    if (!P.spare || !LC.auto_reset || (P.mode != 2 && P.mode != 4) || done >= budget) return false;
    if (!u_ld32(&S.h->over) || u_ld32(&S.h->error)) return false;
    const unsigned char* sp = P.spare + (size_t)r * LC.state_bytes;
    if (rfl(((const Hdr*)(sp + kOffHdr))->episode) != u_ld32(&S.h->episode) + 1u) return false;
    const int lane = S.lane;
    // carried over: the log position and the running totals (hot_store has added this launch's)
    const uint32_t dec = u_ld32(&S.h->dec_count);
    const uint64_t ht = (uint64_t)u_ld64((const int64_t*)&S.h->hops_total);
    const uint64_t et = (uint64_t)u_ld64((const int64_t*)&S.h->events_total);
    __syncthreads();
    const uint4* s4 = (const uint4*)sp;
    uint4* d4 = (uint4*)S.base;
    for (uint32_t i = (uint32_t)lane; i < LC.lds_state_bytes / 16u; i += kWave) d4[i] = s4[i];
    regs_io(R, (uint32_t*)(const_cast<unsigned char*>(sp) + LC.s_regs), lane, false);
    __syncthreads();
    if (lane == 0) {
        S.h->dec_count = dec; S.h->hops_total = ht; S.h->events_total = et;
        S.c->dec_count = dec; S.c->hops_total = ht; S.c->events_total = et;
    }
    __syncthreads();
    budget -= done;
    return true;
}
template <class RS>
__device__ __forceinline__ bool spare_restart(const KParams&, Sim&, RS&, int, uint32_t, uint32_t&) { return false; }

// ---------------------------------------------------------------------------
// the event loop of one launch (both engines): finish the pending decision,
// then one discrete event per iteration until max_hops hops, a decision that
// needs an external action, or the end of the episode; publish the outputs.
// ---------------------------------------------------------------------------
// EXPL: the fused policy's action goes through explore_action (1) or smart_explore_action (2)
// at both decision sites; 3: the action is stoch_action's (P.stoch_tab) and no table is read
// MB: mlp_action_reg's batch (the memory-resident engine passes 0)
// LQ: the MLP is one of the reduced DQN-buffer models (lightq_action_reg with P.lq_dims;
// register-resident instances of their own)
// FUSED: the launch is a fused table run (P.mode == 2) of an env whose table sits in LDS, known
// at compile time (step_kernel.h prisma_step_kernel_fused_t): the external-policy exit of an
// arrival, the PENDING record, the P.actions branch and the table's HBM pointer are compiled out
template <bool MLP, int MB, int EXPL = 0, bool LQ = false, bool FUSED = false, class RS>
__device__ __forceinline__ uint32_t event_loop(const KParams& P, Sim& S, RS& R, int r, uint32_t max_hops) {
    const int lane = S.lane;
    const LV& L = S.lv;
    const bool mlp_mode = MLP;
    S.mlp_inst = MLP;
    static_assert(!FUSED || (!MLP && !RS::kMem), "the fused-only instances are register-engine table instances");
    const bool table_mode = FUSED || (P.mode == 2) || mlp_mode;   // fused in-kernel policy
    S.mlp = P.mlp;
    S.mlp_rp = P.mlp_rp;
    S.table_g = FUSED ? nullptr : P.table;
    S.tab_lds = FUSED || (S.tab_lds && ((CLayout*)P.lay)->table_in_lds != 0u);
    const uint32_t NN = (uint32_t)L.N();
    Hot H;
    hot_load(S, H);
    flow_min_refresh(S, R, H);

    H.stop = 0;
    H.hops_launch = 0;
    if (S.prio_total) prio_update(S, 0u);
    if (H.pend && !H.over) {
        if (table_mode) {
            uint32_t pn = u_ld32(&S.h->pend_node), pd = u_ld32(&S.h->pend_ent[1]);
            int a;
            if constexpr (EXPL == 3) {
                // (the previous decision's record through the pending entry, as the arrival found it)
                const uint32_t px = u_ld32(&S.h->pend_ent[0]), pdec = u_ld32(&S.h->pend_dec);
                const int32_t pp = ent_type(px) == T_FRESH ? -1 : (int32_t)(pdec - relay_dist(S, pdec, px));
                const uint32_t w6 = pp < 0 ? 0u : record_word(S, (uint32_t)pp, 24);
                const uint32_t w7 = pp < 0 ? 0u : record_word(S, (uint32_t)pp, 28);
                a = stoch_action(S, H, P.stoch_tab, pdec, pn, pd, px, pp, w6 & 255u, w7 & 255u);
            } else if (!mlp_mode) {
                a = table_action(S, pn * NN + pd);
            } else if constexpr (RS::kMem) {
                MlpPre1 M0;                              // (no arrival came before: nothing prefetched)
                a = mlp_action_mem<false>(S, pn, (lane < L.W()) ? S.obs[lane] : 0u, M0);
            } else if constexpr (LQ) {
                a = lightq_action_reg<MB>(S, pn, (lane < L.W()) ? S.obs[lane] : 0u, P.lq_dims);
            } else {
                MlpPre1 M0;                              // (never used: see mlp_action_reg)
                a = mlp_action_reg<MB>(S, pn, (lane < L.W()) ? S.obs[lane] : 0u, M0);
            }
            // (the instances without the ctrl paths: every pending notification is a data decision)
            if (EXPL == 1) a = explore_action(S, H, P.explore_thr, u_ld32(&S.h->pend_dec), pn, a);
            if (EXPL == 2) a = smart_explore_action(S, H, P.explore_thr, P.action_hist, r, u_ld32(&S.h->pend_dec), pn, a);
            H.hops_launch += finish_pending(S, R, H, a);
        } else if (P.actions) {
            // (counted like a fused hop: hops_total is the hops since reset on every path)
            H.hops_launch += finish_pending(S, R, H, (int)rfl((uint32_t)P.actions[r]));
        } else {
            H.stop = 1;                                // nothing to apply: re-emit the pending obs
        }
    }
    if (H.over || (table_mode && H.hops_launch >= max_hops)) H.stop = 1;

    // Drain the stage-in loads here: otherwise the waitcnt pass keeps them
    // "possibly pending" at the loop header and emits vmcnt waits there that,
    // on every later iteration, also wait for the previous event's record
    // stores.
    __builtin_amdgcn_s_waitcnt(0);
#if PRISMA_TIMING
    uint64_t tm_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t tm_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tm_a = 0, tm_b = 0;
    S.tsub[0] = 0; S.tsub[1] = 0; S.tlast = 0;
    S.tmlp[0] = 0; S.tmlp[1] = 0; S.tmlp[2] = 0; S.tmlp[3] = 0;
    S.tflow[0] = 0; S.tflow[1] = 0; S.tflow[2] = 0; S.tflow[3] = 0; S.tfl = 0;
    for (int i = 0; i < 16; ++i) { S.tp[i] = 0; S.tpn[i] = 0; }
    S.tpl = 0;
#define TM_MARK(i) do { tm_b = TM_NOW(); tm_acc[i] += tm_b - tm_a; tm_cnt[i]++; tm_a = tm_b; } while (0)
#else
#define TM_MARK(i) do { } while (0)
#endif
    constexpr bool kPre = MLP && RS::kMem;               // memory-resident engine + MLP: weights prefetched
    while (!H.stop) {
        int64_t bt;
        uint32_t bc, bs;
#if PRISMA_TIMING
        tm_a = TM_NOW();
#endif
        select_event(S, R, H, lane, bt, bc, bs);
        if (bt >= L.t_end()) {                           // Simulator::Stop(simTime) (sim.cc:703)
            lazy_resolve(S, R, H, true);                 // here, not after the loop: there it costs registers
            H.over = 1;
            H.stop = 1;
            break;
        }
        H.now = bt;
        H.cur_seq = bs;
#if PRISMA_TRACE
        if (lane == 0 && r < 8 && g_prisma_trace) {
            const unsigned int i = g_prisma_trace_n[r]++;
            if (i < g_prisma_trace_cap) {
                long long* q = g_prisma_trace + ((size_t)r * g_prisma_trace_cap + i) * 3;
                q[0] = bt; q[1] = bc >> 28; q[2] = bc & 0x0fffffffu;
            }
        }
#endif
        H.ev_launch++;                                   // added to the events counter at exit
        const uint32_t kind = bc >> 28, id = bc & 0x0fffffffu;
        TM_MARK(0);
        if (kind == K_ARRIVE) {
            Decision D;
            D.r0 = -1; D.deg = 0;
            MlpPre1 Mp;                                  // (kPre) the decision's first weights, fetched on arrival
            const int need = on_arrive<kPre>(S, R, H, id, D, table_mode, Mp);
            TM_MARK(1);
            if (need) {
                if (table_mode) {
                    int a;
                    if constexpr (EXPL == 3) a = stoch_action(S, H, P.stoch_tab, D.d, D.v, D.dst, D.x, D.prev, D.last, D.pact & 255u);
                    else if (!mlp_mode) a = table_action(S, D.v * NN + D.dst);
                    else if constexpr (RS::kMem) a = mlp_action_mem<true>(S, D.v, D.obs, Mp);
                    else if constexpr (LQ) a = lightq_action_reg<MB>(S, D.v, D.obs, P.lq_dims);
                    else a = mlp_action_reg<MB>(S, D.v, D.obs, Mp);
                    if (EXPL == 1) a = explore_action(S, H, P.explore_thr, D.d, D.v, a);
                    if (EXPL == 2) a = smart_explore_action(S, H, P.explore_thr, P.action_hist, r, D.d, D.v, a);
                    // (the row handoff: headline +2.1 % in A/B; config 4's MLP instance -2 %, so
                    // the MLP instances read the row again)
                    apply_decision<!RS::kMem && !MLP>(S, R, H, D.x, D.dst, D.start, D.uid, D.v, D.d, a, true,
                                   D.reward, D.prev, D.obs,
                                   (D.flags & PEND_ECHO) ? (uint32_t)t_lrev(S, id) : kNoLink, D.last, D.ttl,
                                   D.r0, D.deg);
                    H.hops_launch++;
                    if (H.hops_launch >= max_hops) H.stop = 1;
                    // (>=, not ==: finish_pending's hop before the loop can step over a boundary)
                    if (H.hops_launch >= S.prio_next) prio_update(S, H.hops_launch);
                    TM_MARK(2);
                } else {
                    if (lane == 0) {
                        Hdr& h = *S.h;
                        h.pend_link = id; h.pend_node = D.v; h.pend_dec = D.d;
                        h.pend_ent[0] = D.x; h.pend_ent[1] = D.dst; h.pend_ent[2] = D.start; h.pend_ent[3] = D.flags;
                        h.pend_uid = D.uid; h.pend_last = D.last;
                    }
                    if (lane < L.W()) S.obs[lane] = D.obs;
                    H.pend = 1;
                    H.stop = 1;
                }
            }
        } else if (kind == K_COMPLETE) {
            on_complete(S, R, H, id);
            TM_MARK(3);
        } else if (kind == K_FLOW) {
            on_flow(S, R, H, id);
            TM_MARK(4);
        } else {
            on_ping_round(S, R, H);
            TM_MARK(5);
        }
        if (H.error) { H.over = 1; H.stop = 1; }
        if (!MLP) {
            // the loop's exit flags as provably uniform values: the loop then exits with a
            // scalar branch instead of exec-mask bookkeeping (A/B: table instances +0.6 %, the
            // MLP instances -1 %, so only the former)
            H.stop = rfl(H.stop); H.over = rfl(H.over); H.error = rfl(H.error);
        }
    }
#if PRISMA_TIMING
    tm_acc[6] = S.tsub[0]; tm_acc[7] = S.tsub[1];
    if (lane == 0) {
        for (int i = 0; i < 8; ++i) {
            atomicAdd(&g_prisma_timing[i], (unsigned long long)tm_acc[i]);
            atomicAdd(&g_prisma_timing[8 + i], (unsigned long long)tm_cnt[i]);
        }
        for (int i = 0; i < 4; ++i) atomicAdd(&g_prisma_timing[16 + i], (unsigned long long)S.tmlp[i]);
        for (int i = 0; i < 4; ++i) atomicAdd(&g_prisma_timing[20 + i], (unsigned long long)S.tflow[i]);
        for (int i = 0; i < 16; ++i) {
            atomicAdd(&g_prisma_timing[24 + i], (unsigned long long)S.tp[i]);
            atomicAdd(&g_prisma_timing[40 + i], (unsigned long long)S.tpn[i]);
        }
    }
#endif
    // elided completions up to where the launch stopped -- after a failure too: the reference has
    // executed them before the failing event, and `events` counts them (include/prisma.h)
    lazy_resolve(S, R, H, false);

    hot_store(S, R, H);
    __syncthreads();
    const bool pending = H.pend && !H.over;
    if (P.mask_out && lane == 0) P.mask_out[r] = pending ? 1 : 0;
    if (P.node_out && lane == 0) P.node_out[r] = pending ? (int32_t)S.h->pend_node : -1;
    if (P.obs_out && lane < L.W()) P.obs_out[(size_t)r * L.W() + lane] = pending ? (int32_t)S.obs[lane] : 0;
    publish_counters(S, P, r, lane);
    return H.hops_launch;
}
