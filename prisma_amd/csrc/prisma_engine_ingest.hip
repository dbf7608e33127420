// prisma_engine_ingest.hip — the decision log straight into the trainer's per-node replay rings
// (prisma_ingest_transitions, include/prisma.h): what VecRoutingEnv.transitions() followed by
// ReplayBuffers.add() computes with a chain of torch ops, as three launches on the caller's
// stream with no host read.
//
//   count    one wave per replica walks its window of new records, 64 at a time, and histograms
//            the hop items (by the predecessor's node) and the loss items (by the record's node)
//            in LDS: cnt[kind][u][r].
//   scan     one workgroup per node u: the exclusive prefix over the replicas of the hop counts,
//            then of the loss counts from the node's hop total on, which is the batch order of
//            the torch path (all hop items in (r, d) order, then all loss items) restricted to
//            u; base[kind][u][r].  It also fixes the node's part of the ring arithmetic -- how
//            many leading items an overflowing batch drops, the slot of the first kept one --
//            and moves next_idx / count / total (only this workgroup touches node u's counters,
//            and the scatter reads what it saved, not next_idx).
//   scatter  one wave per replica walks the window again.  A lane's rank among the chunk's lower
//            lanes with the same node comes from ballots (one round per distinct node in the
//            chunk); added to the node's running count in LDS, which started at base[kind][u][r],
//            it is the item's rank among the node's items of the whole batch.  Kept items copy
//            their rows with 16-B loads and stores.
//
// No atomic decides a slot: placement follows from the prefix sums alone, so the result is
// deterministic and equals the stable sort of ReplayBuffers.add.
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC (buildid.HIPCC_FLAGS)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/prisma.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxNodes = 256;               // record.node is one byte (both engines: <= 256 nodes)
constexpr int kScanThreads = 1024;

struct IngestParams {
    const unsigned char* log;                // [R][cap][rec_bytes]
    const prisma_counters_t* cnt;            // [R]
    int64_t* consumed;                       // [R]
    int32_t R, N, W;
    uint32_t cap, rec_bytes;
    float loss_penalty;
    // scratch (library-owned)
    uint32_t* counts;                        // [2][N][R]: hop, loss
    uint64_t* bases;                         // [2][N][R]
    uint64_t* skip;                          // [N]: leading items of the node's batch that overflow the ring
    int64_t* start;                          // [N]: slot of the node's first kept item
    prisma_replay_t rings;
};

// the window of replica r: records [lo, dec)
__device__ __forceinline__ void window(const IngestParams& P, int r, int64_t& lo, int64_t& dec) {
    dec = (int64_t)P.cnt[r].dec_count;
    const int64_t c = P.consumed[r], w = dec - (int64_t)P.cap + 1;
    lo = c > w ? c : w;
}

struct Item {
    bool hop, loss, pending;
    uint32_t node_p, node_d;                 // the hop item's node (predecessor's) and the loss item's
    const unsigned char* rec;                // record d
    const unsigned char* prec;               // record p (hop only)
    uint32_t w7;                             // action | status << 8 | ttl << 16 | episode << 24 of d
    double reward;
};

// Lane's record d of replica r (valid: d < dec), classified.  Items of a node id >= N are dropped
// here, for every pass alike (the engines write none).
__device__ __forceinline__ Item classify(const IngestParams& P, const unsigned char* logrep, int64_t d, bool valid) {
    Item it;
    it.hop = it.loss = it.pending = false;
    it.node_p = it.node_d = 0u;
    it.rec = it.prec = logrep;
    it.w7 = 0u;
    it.reward = 0.0;
    if (valid) {
        it.rec = logrep + (size_t)((uint32_t)d & (P.cap - 1u)) * P.rec_bytes;
        const uint4 h0 = *(const uint4*)it.rec;              // t_ns, uid, prev
        const uint4 h1 = *(const uint4*)(it.rec + 16);       // reward, node | dst | start_s, w7
        const int32_t prev = (int32_t)h0.w;
        const uint32_t status = (h1.w >> 8) & 0xFFu;
        it.w7 = h1.w;
        it.reward = __longlong_as_double((long long)(((uint64_t)h1.y << 32) | h1.x));
        it.node_d = h1.z & 0xFFu;
        it.pending = status == (uint32_t)PRISMA_ST_PENDING;
        if (!it.pending && prev >= 0) {
            it.prec = logrep + (size_t)((uint32_t)prev & (P.cap - 1u)) * P.rec_bytes;
            it.node_p = *(const uint32_t*)(it.prec + 24) & 0xFFu;
            it.hop = it.node_p < (uint32_t)P.N;
        }
        it.loss = status == (uint32_t)PRISMA_ST_DROPPED && it.node_d < (uint32_t)P.N;
    }
    return it;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ void __launch_bounds__(kWave) prisma_ingest_count_kernel(IngestParams P) {
    __shared__ uint32_t hist[2][kMaxNodes];
    const int r = blockIdx.x, lane = threadIdx.x;
    for (int u = lane; u < kMaxNodes; u += kWave) hist[0][u] = hist[1][u] = 0u;
    __syncthreads();
    int64_t lo, dec;
    window(P, r, lo, dec);
    const unsigned char* logrep = P.log + (size_t)r * P.cap * P.rec_bytes;
    for (int64_t c = lo; c < dec; c += kWave) {
        const int64_t d = c + lane;
        const Item it = classify(P, logrep, d, d < dec);
        if (it.hop) atomicAdd(&hist[0][it.node_p], 1u);
        if (it.loss) atomicAdd(&hist[1][it.node_d], 1u);
    }
    __syncthreads();
    for (int u = lane; u < P.N; u += kWave) {
        P.counts[(size_t)u * P.R + r] = hist[0][u];
        P.counts[((size_t)P.N + u) * P.R + r] = hist[1][u];
    }
}

// inclusive prefix sum over the 64 lanes (all active): row_shr 1, 2, 4, 8 within the rows of 16,
// then row_bcast 15 / 31 across them; lanes with no source take 0
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint64_t scan_step(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return v + (((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t wave_scan(uint64_t v) {
    v = scan_step<0x111, 0xF>(v);
    v = scan_step<0x112, 0xF>(v);
    v = scan_step<0x114, 0xF>(v);
    v = scan_step<0x118, 0xF>(v);
    v = scan_step<0x142, 0xA>(v);
    v = scan_step<0x143, 0xC>(v);
    return v;
}

__global__ void __launch_bounds__(kScanThreads) prisma_ingest_scan_kernel(IngestParams P) {
    __shared__ uint64_t wsum[kScanThreads / kWave];
    const int u = blockIdx.x;
    const uint32_t tid = threadIdx.x, wave = tid / kWave;
    uint64_t carry = 0;                      // the node's items before this chunk, hop items first
    for (int kind = 0; kind < 2; ++kind) {
        const size_t row = ((size_t)kind * P.N + u) * P.R;
        for (int32_t c = 0; c < P.R; c += kScanThreads) {
            const int32_t i = c + (int32_t)tid;
            const uint64_t v = i < P.R ? (uint64_t)P.counts[row + i] : 0u;
            const uint64_t incl = wave_scan(v);
            if ((tid & (kWave - 1)) == kWave - 1) wsum[wave] = incl;
            __syncthreads();
            uint64_t off = 0, total = 0;
            for (uint32_t w = 0; w < kScanThreads / kWave; ++w) {
                const uint64_t s = wsum[w];
                off += w < wave ? s : 0u;
                total += s;
            }
            if (i < P.R) P.bases[row + i] = carry + off + incl - v;
            carry += total;
            __syncthreads();                 // wsum is rewritten by the next chunk
        }
    }
    if (tid == 0) {
        const prisma_replay_t& B = P.rings;
        const uint64_t size = (uint64_t)B.size, n = carry;
        const uint64_t sk = n > size ? n - size : 0u;          // an overflowing batch keeps its last `size`
        const uint64_t next = (uint64_t)B.next_idx[u];
        P.skip[u] = sk;
        P.start[u] = (int64_t)((next + sk % size) % size);
        B.next_idx[u] = (int64_t)((next + n % size) % size);
        const uint64_t have = (uint64_t)B.count[u] + n;
        B.count[u] = (int64_t)(have > size ? size : have);
        B.total[u] += (int64_t)n;
    }
}

// ranks of the flagged lanes among the chunk's lower flagged lanes with the same node: one round
// per distinct node (the first remaining lane's), a ballot of its lanes, their count below each.
// -> rank (node's running count included); the running count moves on by the group's size.
__device__ __forceinline__ uint64_t chunk_rank(bool flag, uint32_t node, uint64_t* run) {
    uint32_t below = 0u, group = 0u;
    bool todo = flag;
    while (todo) {
        const uint32_t u = __builtin_amdgcn_readfirstlane(node);
        const uint64_t m = __ballot(node == u);
        if (node == u) {
            below = lanes_below(m);
            group = (uint32_t)__builtin_popcountll(m);
            todo = false;
        }
    }
    uint64_t rank = 0;
    if (flag) rank = run[node] + below;
    __syncthreads();                         // every lane has read the running counts
    if (flag && below == 0u) run[node] = rank + group;
    __syncthreads();
    return rank;
}

__device__ __forceinline__ void copy_row(int32_t* dst, const unsigned char* src, int W) {
    uint4* d4 = (uint4*)dst;
    const uint4* s4 = (const uint4*)src;
    for (int k = 0; k < W / 4; ++k) d4[k] = s4[k];
}

// ring slot of the node's item of rank `rank`, or -1 if the batch overflows the ring past it
__device__ __forceinline__ int64_t ring_slot(const IngestParams& P, uint32_t u, uint64_t rank) {
    const uint64_t sk = P.skip[u];
    if (rank < sk) return -1;
    int64_t s = P.start[u] + (int64_t)(rank - sk);
    if (s >= P.rings.size) s -= P.rings.size;
    return s;
}

__global__ void __launch_bounds__(kWave) prisma_ingest_scatter_kernel(IngestParams P) {
    __shared__ uint64_t run[2][kMaxNodes];
    const int r = blockIdx.x, lane = threadIdx.x;
    const prisma_replay_t& B = P.rings;
    const int W = P.W;
    for (int u = lane; u < kMaxNodes; u += kWave) {
        run[0][u] = u < P.N ? P.bases[(size_t)u * P.R + r] : 0u;
        run[1][u] = u < P.N ? P.bases[((size_t)P.N + u) * P.R + r] : 0u;
    }
    __syncthreads();
    int64_t lo, dec;
    window(P, r, lo, dec);
    const unsigned char* logrep = P.log + (size_t)r * P.cap * P.rec_bytes;
    bool last_pending = false;
    for (int64_t c = lo; c < dec; c += kWave) {
        const int64_t d = c + lane;
        const Item it = classify(P, logrep, d, d < dec);
        last_pending = __ballot(d == dec - 1 && it.pending) != 0u;   // (meaningful in the last chunk)
        const uint64_t rank_h = chunk_rank(it.hop, it.node_p, run[0]);
        const uint64_t rank_l = chunk_rank(it.loss, it.node_d, run[1]);
        if (it.hop) {
            const int64_t s = ring_slot(P, it.node_p, rank_h);
            if (s >= 0) {
                const size_t q = (size_t)it.node_p * (size_t)B.size + (size_t)s;
                copy_row(B.obs + q * W, it.prec + 32, W);
                copy_row(B.next_obs + q * W, it.rec + 32, W);
                B.action[q] = (int64_t)(int8_t)(*(const uint32_t*)(it.prec + 28) & 0xFFu);
                B.reward[q] = (float)it.reward;
                B.done[q] = ((it.w7 >> 8) & 0xFFu) == (uint32_t)PRISMA_ST_DESTINATION ? 1u : 0u;
                B.replica[q] = (int64_t)r;
            }
        }
        if (it.loss) {
            const int64_t s = ring_slot(P, it.node_d, rank_l);
            if (s >= 0) {
                const size_t q = (size_t)it.node_d * (size_t)B.size + (size_t)s;
                copy_row(B.obs + q * W, it.rec + 32, W);
                uint4* n4 = (uint4*)(B.next_obs + q * W);
                n4[0] = make_uint4(*(const uint32_t*)(it.rec + 32), 0u, 0u, 0u);
                for (int k = 1; k < W / 4; ++k) n4[k] = make_uint4(0u, 0u, 0u, 0u);
                B.action[q] = (int64_t)(int8_t)(it.w7 & 0xFFu);
                B.reward[q] = P.loss_penalty;
                B.done[q] = 1u;
                B.replica[q] = (int64_t)r;
            }
        }
    }
    if (lane == 0 && dec > lo) P.consumed[r] = dec - (last_pending ? 1 : 0);
}

}  // namespace

// Scratch bytes prisma_ingest_launch needs for an env of R replicas and N nodes.
size_t prisma_ingest_scratch_bytes(int32_t R, int32_t N) {
    const size_t rn = (size_t)R * (size_t)N;
    return 2 * rn * sizeof(uint64_t) + 2 * (size_t)N * sizeof(uint64_t) + 2 * rn * sizeof(uint32_t);
}

// The three launches (prisma_engine.hip's prisma_ingest_transitions validates and owns the scratch).
hipError_t prisma_ingest_launch(const unsigned char* log, const prisma_counters_t* cnt, int64_t* consumed, int32_t R,
                                int32_t N, int32_t W, uint32_t cap, uint32_t rec_bytes, float loss_penalty,
                                void* scratch, const prisma_replay_t* rings, hipStream_t stream) {
    IngestParams P;
    P.log = log;
    P.cnt = cnt;
    P.consumed = consumed;
    P.R = R;
    P.N = N;
    P.W = W;
    P.cap = cap;
    P.rec_bytes = rec_bytes;
    P.loss_penalty = loss_penalty;
    const size_t rn = (size_t)R * (size_t)N;
    P.bases = (uint64_t*)scratch;
    P.skip = P.bases + 2 * rn;
    P.start = (int64_t*)(P.skip + N);
    P.counts = (uint32_t*)(P.start + N);
    P.rings = *rings;
    hipLaunchKernelGGL(prisma_ingest_count_kernel, dim3((unsigned)R), dim3(kWave), 0, stream, P);
    hipLaunchKernelGGL(prisma_ingest_scan_kernel, dim3((unsigned)N), dim3(kScanThreads), 0, stream, P);
    hipLaunchKernelGGL(prisma_ingest_scatter_kernel, dim3((unsigned)R), dim3(kWave), 0, stream, P);
    return hipGetLastError();
}
