// prisma_engine_targets.hip — the bootstrap targets of a sampled replay batch against every stored
// weight generation (prisma_replay_targets, include/prisma.h): what ReplayBuffers.sample_full()
// followed by QRoutingTrainer.targets() computes with three host reads and one torch forward pass
// per generation, as one launch on the caller's stream with no host read.
//
// One wave per sample, four waves per workgroup, each wave with its own LDS slice for the
// activations; lane j is unit j of a layer.  Rows are ordered by node (row i = u * batch + b), so
// neighbouring waves evaluate the same few next nodes and their weights stay in L2.  The weights
// are read straight from the packed row-major layout: W[i][j] over the lanes j is one coalesced
// row, so no generation is repacked.
//
// The operation order is DESIGN.md §2's, the one mlp_action_reg (engine_core.h) runs and
// or_mlp_q / tests/lightq_util.HostMLP restate: LayerNorm with sequential __fadd_rn sums in k
// order, __fdiv_rn and the correctly rounded sqrt(var + 1e-3f); the one-hot row plus its bias; every dense unit one
// fmaf chain from +0 in input order (the one-hot branch first, then the buffers branch), the bias
// added last with a plain add; det_elu on every layer.  The widths (B, H, NH) and the presence of
// the buffers branch are wave-uniform values, as lightq_action_reg has them.  Degrees up to 55:
// the LayerNorm and the buffers branch take their inputs from LDS, not from a half wave.
//
// Every index is checked before an address is formed from it (the rule's "not evaluable" cases).
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC (buildid.HIPCC_FLAGS)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/prisma.h"
#include "numerics.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerGroup = 4;
constexpr int kUnroll = 8;                   // weight loads in flight per lane in a dense layer

struct TargetsParams {
    prisma_replay_t rings;
    const int64_t* idx;                      // [N][batch]
    const float* const* weights;             // [n_gen]
    const int32_t* gen_of;                   // [R][T] or null
    const int32_t* row;                      // [N + 1] overlay CSR rows by underlay id
    const int32_t* nxt;                      // [T] next node of (u, a)
    const int32_t* back;                     // [T] the next node's action leading back, or -1
    int32_t batch, n_gen, R, N, D, T;
    int32_t B, H, NH, buffers;               // widths; buffers = 0: the routing model
    float gamma;
    int32_t* obs_out;                        // [N * batch][W] or null
    int64_t* action_out;                     // [N * batch] or null
    float* target_out;                       // [N * batch]
    uint8_t* status_out;                     // [N * batch] or null
};

__device__ __forceinline__ int rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }

// One dense layer's fmaf chains before the bias: unit j (clamped by the caller to a valid column)
// over inputs h[0 .. in) in input order from +0; W is [in][stride] row-major.
__device__ __forceinline__ float dense_chain(const float* __restrict__ W, int in, int stride, int j, const float* h) {
    float acc = 0.0f;
    int i = 0;
    for (; i + kUnroll <= in; i += kUnroll) {
        float w[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) w[k] = W[(size_t)(i + k) * stride + j];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) acc = __builtin_fmaf(h[i + k], w[k], acc);
    }
    for (; i < in; ++i) acc = __builtin_fmaf(h[i], W[(size_t)i * stride + j], acc);
    return acc;
}

__global__ void __launch_bounds__(kWave * kWavesPerGroup) prisma_replay_targets_kernel(TargetsParams P) {
    __shared__ float lds[kWavesPerGroup][3][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x / kWave));
    const int64_t rows = (int64_t)P.N * P.batch;
    const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + wave;
    if (i >= rows) return;                   // (no workgroup barrier below: the waves are independent)
    float* xs = lds[wave][0];                // buffer values, their squares, the normalised values; Q
    float* ha = lds[wave][1];
    float* hb = lds[wave][2];
    const prisma_replay_t& G = P.rings;
    const int W = G.obs_width;
    const int u = (int)(i / P.batch);
    const int64_t s = P.idx[i];
    if (s < 0 || s >= G.size) {              // no ring address is formed from a slot outside the ring
        if (P.obs_out && lane < W) P.obs_out[i * W + lane] = 0;
        if (lane == 0) {
            if (P.action_out) P.action_out[i] = 0;
            P.target_out[i] = 0.0f;
            if (P.status_out) P.status_out[i] = 2u;
        }
        return;
    }
    const size_t q = (size_t)u * (size_t)G.size + (size_t)s;
    const int64_t a64 = G.action[q];
    const float rew = G.reward[q];
    const bool done = G.done[q] != 0u;
    const int64_t r64 = G.replica[q];
    const uint32_t nobs = lane < W ? (uint32_t)G.next_obs[q * W + lane] : 0u;
    if (P.obs_out && lane < W) P.obs_out[i * W + lane] = G.obs[q * W + lane];
    if (lane == 0 && P.action_out) P.action_out[i] = a64;
    const int degu = P.row[u + 1] - P.row[u];
    int g = -1, t = 0;
    if (a64 >= 0 && a64 < degu && r64 >= 0 && r64 < P.R) {
        t = P.row[u] + (int)a64;
        g = P.gen_of ? P.gen_of[(size_t)r64 * P.T + t] : 0;
    }
    const uint32_t dst = (uint32_t)rfl((int)nobs);           // lane 0: next_obs[0], the destination's overlay index
    // (the done test comes after the not-evaluable ones, as in the rule; a destination index past the
    // one-hot input is only met when the network would be evaluated)
    const bool bad = g < 0 || g >= P.n_gen || (!done && dst >= (uint32_t)P.N);
    if (bad || done) {
        if (lane == 0) {
            P.target_out[i] = rew;
            if (P.status_out) P.status_out[i] = bad ? 2u : 1u;
        }
        return;
    }
    const int v = rfl(P.nxt[t]), bk = rfl(P.back[t]);
    const int deg = rfl(P.row[v + 1] - P.row[v]);
    const int N = P.N, D = P.D, B = P.B, H = P.H;
    // sections of the packed generation (include/prisma.h)
    const float* __restrict__ Wg = P.weights[g];
    const float* __restrict__ W1 = Wg;
    const float* __restrict__ b1 = W1 + (size_t)N * N * B;
    const float* __restrict__ Wb = b1 + (size_t)N * B;
    const float* __restrict__ bb = Wb + (P.buffers ? (size_t)N * D * B : 0);
    const float* __restrict__ W2 = bb + (P.buffers ? (size_t)N * B : 0);
    const int in2 = P.buffers ? 2 * B : B;
    const float* __restrict__ b2 = W2 + (size_t)N * in2 * H;
    const float* __restrict__ W3 = b2 + (size_t)N * H;
    const float* __restrict__ b3 = W3 + (P.NH == 2 ? (size_t)N * H * H : 0);
    const float* __restrict__ W4 = b3 + (P.NH == 2 ? (size_t)N * H : 0);
    const float* __restrict__ b4 = W4 + (size_t)N * H * D;

    // layer 1, one-hot branch: lanes [0, B)
    if (lane < B)
        ha[lane] = det_elu(__fadd_rn(W1[((size_t)v * N + dst) * B + lane], b1[(size_t)v * B + lane]));
    if (P.buffers) {
        // LayerNormalization of the deg buffer values: lane k + 1 holds value k, the sums run in k
        // order over LDS in every lane
        const float xf = (float)nobs;
        xs[lane] = xf;
        __builtin_amdgcn_wave_barrier();
        float sum = 0.0f;
        for (int k = 0; k < deg; ++k) sum = __fadd_rn(sum, xs[k + 1]);
        const float mean = __fdiv_rn(sum, (float)deg);
        const float dv = __fsub_rn(xf, mean);
        __builtin_amdgcn_wave_barrier();
        xs[lane] = __fmul_rn(dv, dv);
        __builtin_amdgcn_wave_barrier();
        float var = 0.0f;
        for (int k = 0; k < deg; ++k) var = __fadd_rn(var, xs[k + 1]);
        var = __fdiv_rn(var, (float)deg);
        // (the correctly rounded square root: __builtin_sqrtf compiles to v_sqrt_f32 plus its fix-up
        // steps, where this toolchain's __fsqrt_rn is the native 1-ulp instruction alone -- enough
        // for an argmin, not for targets held to the host's IEEE sqrt bit for bit)
        const float den = __builtin_sqrtf(__fadd_rn(var, 1e-3f));
        __builtin_amdgcn_wave_barrier();
        xs[lane] = __fdiv_rn(dv, den);       // xs[k + 1]: normalised value k
        __builtin_amdgcn_wave_barrier();
        // buffers branch: lanes [B, 2B), inputs k < deg (deg <= D rows of Wb[v])
        const int jb = (lane >= B && lane < 2 * B) ? lane - B : 0;
        const float acc = dense_chain(Wb + (size_t)v * D * B, deg, B, jb, xs + 1);
        if (lane >= B && lane < 2 * B) ha[lane] = det_elu(__fadd_rn(acc, bb[(size_t)v * B + jb]));
    }
    __builtin_amdgcn_wave_barrier();
    // layer 2: in2 inputs, H units
    {
        const int j = lane < H ? lane : 0;
        const float acc = dense_chain(W2 + (size_t)v * in2 * H, in2, H, j, ha);
        if (lane < H) hb[lane] = det_elu(__fadd_rn(acc, b2[(size_t)v * H + j]));
    }
    __builtin_amdgcn_wave_barrier();
    const float* hin = hb;
    if (P.NH == 2) {
        const int j = lane < H ? lane : 0;
        const float acc = dense_chain(W3 + (size_t)v * H * H, H, H, j, hb);
        if (lane < H) ha[lane] = det_elu(__fadd_rn(acc, b3[(size_t)v * H + j]));
        __builtin_amdgcn_wave_barrier();
        hin = ha;
    }
    // output layer: H inputs, the node's deg units of the D stored
    {
        const int j = lane < deg ? lane : 0;
        const float acc = dense_chain(W4 + (size_t)v * H * D, H, D, j, hin);
        xs[lane] = det_elu(__fadd_rn(acc, b4[(size_t)v * D + j]));
    }
    __builtin_amdgcn_wave_barrier();
    // the filtered minimum: the first-listed order, a NaN never wins, an empty set gives +inf
    float best = __builtin_inff();
    for (int j = 0; j < deg; ++j) {
        const float qj = xs[j];
        if (j != bk && qj < best) best = qj;
    }
    if (lane == 0) {
        P.target_out[i] = __fadd_rn(rew, __fmul_rn(P.gamma, best));
        if (P.status_out) P.status_out[i] = 0u;
    }
}

}  // namespace

// The launch (prisma_engine.hip's prisma_replay_targets validates and owns the topology table:
// tab = row[N + 1], nxt[T], back[T]).  dims = (B, H, NH), buffers = 0 for the routing model.
hipError_t prisma_targets_launch(const prisma_replay_t* rings, const int64_t* idx, int32_t batch,
                                 const prisma_qnets_t* nets, const int32_t* tab, int32_t R, int32_t N, int32_t D,
                                 int32_t T, int32_t B, int32_t H, int32_t NH, int32_t buffers, float gamma,
                                 int32_t* obs_out, int64_t* action_out, float* target_out, uint8_t* status_out,
                                 hipStream_t stream) {
    TargetsParams P;
    P.rings = *rings;
    P.idx = idx;
    P.weights = nets->weights;
    P.gen_of = nets->gen_of;
    P.row = tab;
    P.nxt = tab + N + 1;
    P.back = P.nxt + T;
    P.batch = batch;
    P.n_gen = nets->n_gen;
    P.R = R;
    P.N = N;
    P.D = D;
    P.T = T;
    P.B = B;
    P.H = H;
    P.NH = NH;
    P.buffers = buffers;
    P.gamma = gamma;
    P.obs_out = obs_out;
    P.action_out = action_out;
    P.target_out = target_out;
    P.status_out = status_out;
    const int64_t rows = (int64_t)N * batch;
    const unsigned grid = (unsigned)((rows + kWavesPerGroup - 1) / kWavesPerGroup);
    hipLaunchKernelGGL(prisma_replay_targets_kernel, dim3(grid), dim3(kWave * kWavesPerGroup), 0, stream, P);
    return hipGetLastError();
}
