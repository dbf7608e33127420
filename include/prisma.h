/*
 * prisma.h — C-ABI of the MI355X-native PRISMA packet-hop engine.
 *
 * One shared library (libprisma_amd.so, built from prisma_amd/csrc/) holds
 * R independent topology replicas of PRISMA's ns-3 routing scenario as
 * structure-of-arrays state in HBM and advances them with hand-written
 * gfx950 kernels.  Plain C types only: pointers, sizes, status codes.
 * Device pointers are HIP device addresses (e.g. torch.Tensor.data_ptr()).
 *
 * Each entry point replaces one piece of the reference's per-node
 * ns3-gym path (all citations relative to the reference repo root):
 *
 *   prisma_create      sim.cc:274-683 (topology, links, flows, per-node envs)
 *                      + ns3env.py:378-403 (Ns3Env.__init__ / SimInitMsg)
 *   prisma_reset       sim.cc:253-261 (SetSeed/SetRun) + Simulator start,
 *                      ns3env.py:426-445 (Ns3Env.reset)
 *   prisma_step        ns3env.py:420-423 (Ns3Env.step) ==
 *                      packet-routing-gym.cc:197-213 (ExecuteActions) then
 *                      Simulator::Run until the next
 *                      packet-routing-gym.cc:231-267 (NotifyPktRcv -> Notify)
 *                      with the observation of data-packet-manager.cc:171-206
 *   prisma_run         the same loop with the forwarding decision fused
 *                      in-kernel (forwarder.py:149-195 for table policies:
 *                      SP next-hop table, DQ-routing argmin table)
 *   prisma_read_counters  compute-stats-v2.cc:87-266 (ComputeStats) and the
 *                      forwarder.py:308-431 per-episode trackers
 *   prisma_log_view    the per-hop replay transitions of forwarder.py:352-379
 *                      and the loss transitions of forwarder.py:214-244
 *   prisma_destroy     ns3env.py:452-455 (Ns3Env.close) /
 *                      Ns3ZmqBridge.send_close_command
 *
 * Error behaviour: every call returns PRISMA_OK (0) or a negative status;
 * prisma_last_error() returns a static description of the last failure in
 * the calling thread.  The library never calls exit() (the reference
 * NS_FATAL_ERRORs on bad matrices, sim.cc:310-313; here that is
 * PRISMA_ERR_CONFIG).  Per-replica runtime faults (a ring or wire overflow
 * that the host-side sizing should have excluded) set bits in
 * prisma_counters_t.error and stop that replica; they never touch memory
 * outside the replica's own state.
 */
#ifndef PRISMA_AMD_PRISMA_H
#define PRISMA_AMD_PRISMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRISMA_ABI_VERSION 10

/* status codes */
#define PRISMA_OK              0
#define PRISMA_ERR_CONFIG     -1   /* invalid topology / parameters        */
#define PRISMA_ERR_NOMEM      -2   /* hipMalloc failed                     */
#define PRISMA_ERR_DEVICE     -3   /* no HIP device / wrong architecture   */
#define PRISMA_ERR_LAUNCH     -4   /* kernel launch failed                 */
#define PRISMA_ERR_ARG        -5   /* null handle / bad pointer / bad size */
#define PRISMA_ERR_STATE      -6   /* call not valid in current state      */

/* policy modes for prisma_run (fused decision) */
#define PRISMA_POLICY_TABLE    1   /* action = table[node * n_nodes + dst]
                                      (underlay ids)                       */
#define PRISMA_POLICY_DQN_BUFFER 2 /* in-kernel DQN_buffer_model (models.py:258-306)
                                      over packed fp32 weights, D = max_deg:
                                      W1[N][N][32] b1[N][32] Wb[N][D][32] bb[N][32]
                                      W2[N][64][64] b2[N][64] W3[N][64][64] b3[N][64]
                                      W4[N][64][D] b4[N][D]; x @ W convention;
                                      N = n_nodes, rows by underlay id; the
                                      one-hot input is obs[0] (the overlay
                                      index of the destination)               */
/* The reduced DQN-buffer models: DQN_buffer_model's structure with both
   first-layer branches B wide, NH hidden layers H wide and the deg outputs,
   the same fixed fp32 operation order with 32 -> B and 64 -> H.  Packed fp32
   weights, row-major, x @ W, N = n_nodes, D = max_deg, rows by underlay id:
     W1[N][N][B] b1[N][B] Wb[N][D][B] bb[N][B] W2[N][2B][H] b2[N][H]
     W3[N][H][H] b3[N][H]   (only when NH = 2)
     Wo[N][H][D] bo[N][D]
   Register-resident engine without the ctrl paths only (prisma_run below). */
#define PRISMA_POLICY_DQN_LITE      3 /* DQN_buffer_lite_model (models.py:184-227):
                                         B 16, H 32, NH 2                      */
#define PRISMA_POLICY_DQN_LIGHTER   4 /* DQN_buffer_lighter_model (models.py:39-85):
                                         B 16, H 32, NH 1                      */
#define PRISMA_POLICY_DQN_LIGHTER_2 5 /* DQN_buffer_lighter_2_model (models.py:87-133):
                                         B 8, H 16, NH 1                       */
#define PRISMA_POLICY_DQN_LIGHTER_3 6 /* DQN_buffer_lighter_3_model (models.py:135-181):
                                         B 4, H 8, NH 1                        */

/* engine selection (prisma_params_t.engine).  Either engine: overlay degree
   <= 55 (obs_width <= 56; prisma_record_t), else PRISMA_ERR_CONFIG */
#define PRISMA_ENGINE_AUTO     0   /* register-resident when the topology fits it */
#define PRISMA_ENGINE_REGISTER 1   /* replica state in VGPRs + LDS: <= 255 nodes,
                                      256 links / tunnels / big-signalling
                                      generators, 512 flows                      */
#define PRISMA_ENGINE_MEMORY   2   /* replica state in HBM under an event tree:
                                      <= 256 nodes, links + flows <= 262 144,
                                      <= 4 096 generators, identity overlays
                                      (ER-256); every signalling type            */

/* signalling type (prisma_params_t.signaling_type, argument_parser.py:72 /
   sim.cc:142, 373-392): the payload of the --train small-signalling echo a node
   sends, 0 B ("ideal"), 8 + 8 (overlay degree + 1) B ("NN") or 24 B ("target") */
#define PRISMA_SIGNALING_IDEAL  0
#define PRISMA_SIGNALING_NN     1
#define PRISMA_SIGNALING_TARGET 2

/* random streams (prisma_params_t.rng_mode) */
#define PRISMA_RNG_PHILOX 0        /* counter-based Philox4x32-10 per (seed, replica, flow,
                                      draw, episode): replicas and episodes independent [default] */
#define PRISMA_RNG_NS3    1        /* ns-3's RngStream MRG32k3a (rng-stream.cc): one stream per
                                      RandomVariable object in creation order -- a Uniform per flow
                                      for its start offset (sim.cc:610-620), then per packet the
                                      Uniform of SendPacket (poisson-application.cc:311) and the
                                      Exponential of ScheduleNextTx (:281); simSeed = seed +
                                      replica id as seed and run (sim.cc:253-254), the same streams
                                      every episode (run_ns3.py restarts ns-3 with the same seed) */

/* per-decision status (prisma_record_t.status) */
#define PRISMA_ST_PENDING      0   /* waiting for an action (prisma_step)  */
#define PRISMA_ST_ENQUEUED     1   /* forwarded; a later record has prev==d */
#define PRISMA_ST_DROPPED      2   /* output FIFO overflow: loss transition */
#define PRISMA_ST_DESTINATION  3   /* packet reached its destination       */
#define PRISMA_ST_DISCARDED    4   /* action >= degree: silently discarded  */

/* runtime error bits (prisma_counters_t.error)
 *
 * A failure is a defined return, not a fault.  The event that raises a bit ends the replica's
 * episode there: error |= bit, episode_over = 1, and the launch's other replicas run on.
 *  - LOGWRAP is raised by the arrival of a forwarded data packet (at its next overlay node, or
 *    at a switch inside its tunnel) whose previous decision is log_capacity or more decisions
 *    old.  That event consumes the packet and does nothing else: no record, no hop, no
 *    forward, no counter but `events`.  dec_count is the index the refused record would have
 *    had, so records [max(0, dec_count - log_capacity), dec_count) are all valid and unchanged.
 *  - PINGIDX: the ping-back skips the acknowledgement; the packet is still forwarded or
 *    received and counted like any other.
 *  - now_ns is the time of the failing event; events counts every event up to and including
 *    it; hops_total, dec_count and the other counters are those of the events before it.
 *  - The bits are sticky until prisma_reset: later prisma_step / prisma_run calls execute
 *    nothing for the replica and leave its counters and its log as they are.
 *  - auto_reset leaves a failed replica alone: neither the in-launch restart nor the reset
 *    after a launch starts its next episode.
 */
#define PRISMA_EBIT_RING       1u  /* link ring overflow                   */
#define PRISMA_EBIT_WIRE       2u  /* more packets on a wire than sized    */
#define PRISMA_EBIT_ACKORDER   4u  /* ping-back acknowledging a round more
                                      than 64 rounds behind a lost one     */
#define PRISMA_EBIT_TIME       8u  /* time beyond the representable range  */
#define PRISMA_EBIT_LOGWRAP   16u  /* a hop outlived log_capacity decisions */
#define PRISMA_EBIT_PINGIDX   32u  /* a ping-back crossing an overlay node
                                      carried a tunnel index beyond that
                                      node's degree (out of range of the
                                      reference's vectors: undefined there) */

/*
 * Topology of one replica.  Directed switch links (the PHYSICAL underlay)
 * are numbered in CSR order: links row_ptr[u] .. row_ptr[u+1]-1 leave node
 * u towards link_dst[] in ascending neighbour id.  link_rev[l] is the
 * opposite direction of l.  Flows are listed in (src, dst) lexicographic
 * order of underlay ids, overlay pairs only, with their load-scaled integer
 * bit rate ceil(trunc_parse(TM[s][d]) * load_factor) (sim.cc:494-514,
 * 599-631, ns-3 DataRate parse).
 *
 * Overlay (sim.cc:455-476): n_overlay = 0 means the identity overlay (every
 * node is an overlay node, overlay adjacency == physical adjacency, the
 * abilene / geant examples).  Otherwise overlay_nodes[i] is the underlay id
 * of overlay node i (the inverse of map_overlay.txt) and overlay_adj the
 * [n_overlay][n_overlay] 0/1 overlay adjacency.  The actions of overlay node
 * u are its overlay neighbours in ascending overlay index; an action is a
 * TUNNEL along the underlay route ns-3 global routing installs (unit
 * metrics: at every hop the lowest-id neighbour on a shortest path, computed
 * by the library).  max_deg is the largest overlay degree.
 */
typedef struct prisma_topology {
    int32_t n_nodes;
    int32_t n_links;            /* directed switch links E                 */
    int32_t n_flows;
    int32_t max_deg;
    const int32_t*  row_ptr;    /* [n_nodes + 1]                           */
    const int32_t*  link_dst;   /* [n_links]                               */
    const int32_t*  link_rev;   /* [n_links]                               */
    const int32_t*  flow_src;   /* [n_flows]                               */
    const int32_t*  flow_dst;   /* [n_flows]                               */
    const uint64_t* flow_rate_bps; /* [n_flows], > 0                       */
    int32_t n_overlay;          /* 0: identity overlay                     */
    const int32_t* overlay_nodes;  /* [n_overlay] underlay ids            */
    const int32_t* overlay_adj;    /* [n_overlay * n_overlay] 0/1         */
} prisma_topology_t;

/* scenario parameters (argument_parser.py:34-94 defaults in brackets) */
typedef struct prisma_params {
    uint64_t link_bps;          /* switch link rate            [500000]    */
    int64_t  link_delay_ns;     /* propagation delay           [1 ms]      */
    uint32_t max_buffer_bytes;  /* DropTail byte limit         [16260]     */
    uint32_t packet_size;       /* UDP payload bytes           [512]       */
    double   sim_time_s;        /* episode length              [60]        */
    float    ping_interval_s;   /* pingPacketIntervalTime      [0.2f]      */
    uint32_t ma_size;           /* movingAverageObsSize        [5]         */
    uint32_t ping_as_obs;       /* pingAsObs                   [1]         */
    uint32_t auto_reset;        /* start next episode when one ends        */
    double   loss_penalty;      /* ((16260+542)*8/cap+0.001)*N             */
    uint64_t seed;              /* simSeed                     [100]       */
    uint32_t replica_base;      /* global id of replica 0 (multi-GPU)      */
    uint32_t log_capacity;      /* records kept per replica (power of 2 in
                                   [1024, 2^21]: queue entries keep 22 bits
                                   of a decision's index, so every age up
                                   to log_capacity stays distinguishable;
                                   must exceed the decisions made while one
                                   packet crosses one link: else
                                   PRISMA_EBIT_LOGWRAP)                    */
    uint32_t notify_dest;       /* prisma_step also stops at arrivals at the
                                   destination (done=True notifications) and
                                   at control arrivals, obs [1000, a, b, c]:
                                   small-signalling echo: a = signalled uid,
                                   b = its size on the wire, c = 0; big
                                   signalling: a = NN index, b = segment
                                   index, c = 0x10000 | overlay index of the
                                   signalling node; the action given for
                                   them is ignored                          */
    uint32_t train;             /* --train: every data notification at a
                                   non-source node echoes a small-signalling
                                   packet to its last hop
                                   (data-packet-manager.cc:301-347)        */
    uint32_t engine;            /* PRISMA_ENGINE_* (0 = auto)              */
    /* ---- ABI 7 ---- */
    uint32_t signaling_type;    /* PRISMA_SIGNALING_*          ["ideal"]   */
    uint32_t big_signaling;     /* --signaling (signalingSim) with "NN" and
                                   --train: per flow between overlay
                                   neighbours, a BigSignalingGenerator-
                                   Application sending 512-B NN-weight
                                   segments to the neighbour from AppStartTime
                                   on (sim.cc:634-647, big-signaling-
                                   application.cc:224-309)                 */
    float    sync_step_s;       /* syncStep: seconds per NN copy   [1.0]   */
    uint32_t big_signaling_bytes; /* bigSignalingSize: NN bytes; sim.cc's own
                                     default is 35328, the CLI's (argument_parser.py:74)
                                     512 = one segment per NN; prisma_amd's
                                     config.engine_params passes 512 */
    /* ---- ABI 8 ---- */
    uint32_t rng_mode;          /* PRISMA_RNG_*                    [0]     */
    uint32_t rng_stream_offset; /* PRISMA_RNG_NS3: streams ns-3 itself
                                   creates before sim.cc's flow loop (ARP,
                                   ICMPv6, global routing of every node;
                                   version-dependent, so a parameter)      */
} prisma_params_t;

/*
 * One decision record = one data-packet notification of the reference
 * (PacketRoutingEnv::Notify for a valid DATA packet), i.e. one row the
 * reference Forwarder turns into a replay transition.  The transition of
 * decision d is (obs_d, action_d, r, obs_{d'}, done_{d'}) where d' is the
 * record with prev == d and r = reward_{d'}; or, if status_d == DROPPED,
 * (obs_d, action_d, loss_penalty, [dst, 0...], true) (forwarder.py:226-240).
 * reward is the reference's hop_time_real = curr_time - t_decision computed
 * on the microsecond-formatted times (packet-manager.cc:127-128 ->
 * forwarder.py:208,360), bit-identical to the Python float.
 * Record size is 32 + 4 * obs_width bytes (obs_width = 1 + max_deg rounded up
 * to a multiple of 4, so records are whole 16-byte rows).  The engines write
 * a record as one 64-lane store of its 8 header words and obs_width
 * observation words, so obs_width <= 56: max_deg <= 55, record size <= 256.
 */
typedef struct prisma_record {
    int64_t  t_ns;
    uint32_t uid;
    int32_t  prev;
    double   reward;
    uint8_t  node;
    uint8_t  dst;
    uint16_t start_s;           /* whole second the packet was sent (its
                                   start-time tag, packet-manager.cc)       */
    int8_t   action;
    uint8_t  status;
    uint8_t  ttl;               /* IP TTL the packet arrived with (255 from
                                   its app; -1 per intermediate underlay hop
                                   of a tunnel, Ipv4L3Protocol::IpForward)  */
    uint8_t  episode;           /* episode index mod 256                   */
    uint32_t obs[];             /* [obs_width]                             */
} prisma_record_t;

/* Per-replica counters: ComputeStats (compute-stats-v2.cc) + engine stats */
typedef struct prisma_counters {
    uint64_t events;            /* discrete events executed                */
    uint64_t hops;              /* decisions resulting in enqueue or drop  */
    uint64_t decisions;         /* all data notifications (incl. dest)     */
    uint64_t hop_deg_sum;       /* sum of deg(u) over executed hops        */
    int64_t  now_ns;            /* simulation clock                        */
    double   reward_sum;        /* sum of completed hop rewards + penalties*/
    int32_t  ov_injected;       /* compute-stats-v2.cc:131-134             */
    int32_t  ov_arrived;
    int32_t  ov_lost;
    int32_t  un_injected;
    int32_t  un_arrived;
    int32_t  un_lost;
    int32_t  bytes_data;        /* addGlobalBytesData                      */
    int32_t  bytes_signaling;   /* addGlobalBytesSignaling                 */
    float    cost_sum;          /* running float sum of m_globalCost       */
    float    e2e_sum;           /* running float sum of m_globalE2eDelay   */
    int32_t  cost_n;
    int32_t  e2e_n;
    uint32_t episode;
    uint32_t ping_rounds;
    uint32_t seq;               /* events scheduled (ns-3 uid analogue)    */
    uint32_t uid;               /* data packets created                    */
    uint32_t dec_count;         /* records written (monotonic)             */
    uint32_t ctrl_dropped;      /* ping packets lost on full FIFOs         */
    uint32_t error;             /* PRISMA_EBIT_* bits                      */
    uint32_t episode_over;      /* 1 once the current episode ended        */
    uint64_t hops_total;        /* hops over all episodes since reset      */
    uint64_t events_total;      /* events over all episodes since reset    */
    float    un_cost_sum;       /* running float sum of m_globalUnderlayCost
                                   (loss penalties of data packets dropped
                                   at their own destination node, which a
                                   tunnel can cross)                       */
    int32_t  un_cost_n;
} prisma_counters_t;

/* library-owned device buffers (valid until prisma_destroy) */
typedef struct prisma_log_view {
    void*     records;          /* [n_replicas][log_capacity] records      */
    uint32_t  record_bytes;
    uint32_t  log_capacity;
    int32_t   obs_width;
    int32_t   n_replicas;
} prisma_log_view_t;

typedef struct prisma_env prisma_env_t;

int         prisma_abi_version(void);
const char* prisma_last_error(void);
/* 12 hex digits: hash of the sources + compile flags this library was built
 * from (prisma_amd/buildid.py); loaders refuse a library whose id differs
 * from the sources beside it. */
const char* prisma_build_id(void);

/* Size the per-replica state for this topology and allocate it on
 * `device`.  Validates shapes and ids up front. */
int prisma_create(const prisma_topology_t* topo, const prisma_params_t* params,
                  int32_t n_replicas, int32_t device, prisma_env_t** out);

/* Start episode `episode` of every replica (replica r uses Philox key
 * (seed, replica_base + r)).  Asynchronous on `stream` (hipStream_t). */
int prisma_reset(prisma_env_t* env, uint32_t episode, void* stream);

/* Apply one action per replica to its pending decision (actions may be
 * NULL on the first call after reset), then advance every replica to its
 * next pending decision.  obs_out: device int32 [n_replicas][obs_width];
 * mask_out: device uint8 [n_replicas] (1 = a decision is pending, 0 =
 * episode over); node_out: device int32 [n_replicas], the node deciding
 * (-1 if none).  Any output may be NULL.  A launch never crosses an episode
 * boundary: a replica whose episode ends reports mask 0, and with
 * params.auto_reset it starts its next episode before the call returns (on
 * `stream`), so its next step continues there. */
int prisma_step(prisma_env_t* env, const int32_t* actions, int32_t* obs_out,
                uint8_t* mask_out, int32_t* node_out, void* stream);

/* Fused policy: advance every replica by up to max_hops hops, deciding
 * in-kernel: PRISMA_POLICY_TABLE with `policy_data` = device uint8
 * [n_nodes][n_nodes] action table (SP, DQ-routing argmin), or
 * PRISMA_POLICY_DQN_BUFFER with `policy_data` = device packed fp32 weights
 * (row-major, as StackedQNet.pack() lays them out; the library copies them
 * into an interleaved per-node layout on `stream` before each such launch,
 * so weights updated in place between calls take effect on the next call;
 * calls on one env are ordered by their streams: keep one stream per env),
 * or PRISMA_POLICY_DQN_LITE, _DQN_LIGHTER, _DQN_LIGHTER_2, _DQN_LIGHTER_3 with
 * the packed fp32 weights of that reduced model (the same repack per launch).
 * The reduced models' kernels exist for the register-resident engine without
 * the ctrl paths, as the exploring ones: an env whose prisma_kernel_info
 * reports ctrl = 1 (train, notify_dest, PRISMA_RNG_NS3, a tunnelled overlay
 * with log_capacity >= 2^18) or the memory-resident engine gets
 * PRISMA_ERR_CONFIG for these ids (they were PRISMA_ERR_ARG before they
 * existed; the ABI version is unchanged: no struct or signature moved).
 * A replica stops early at the end of its episode; with params.auto_reset
 * it starts the next episode before the call returns (one launch never
 * crosses an episode boundary). */
int prisma_run(prisma_env_t* env, int32_t policy, const void* policy_data,
               int32_t max_hops, void* stream);

/* prisma_run with epsilon-greedy exploration: the same contract (policies,
 * the DQN-buffer repack, auto_reset, the next-episode restart), but every
 * data decision may replace the policy's action by a uniform pick over the
 * deciding node's neighbours.  The rule is exact, so a host can restate it:
 * for the decision with log index d (the numbering of the records' `prev`,
 * which carries over episode ends), in episode e, at node v of overlay
 * degree deg, with policy action g, in replica r:
 *
 *   c = philox4x32_10(ctr = {d, 0, e, 2}, key = {seed & 0xffffffff, replica_base + r})
 *   a = ((c[0] >> 8) < explore_thr[v]) ? (uint32)(((uint64)c[1] * deg) >> 32) : g
 *
 * explore_thr: device uint32 [n_nodes], indexed by underlay node id,
 * floor(eps[v] * 2^24 + 0.5) clamped to [0, 2^24]: 0 never explores, 2^24
 * always does.  It is read during the launch and constant over it; refresh
 * an epsilon schedule between launches.  Counter word 3 = 2 keeps the draw
 * apart from the flow start offsets (0) and the send delays (1).
 * Destination arrivals and control packets draw nothing.  NULL explore_thr:
 * PRISMA_ERR_ARG.  The exploring kernels exist for the register-resident
 * engine without the ctrl paths: an env whose prisma_kernel_info reports
 * ctrl = 1 (train, notify_dest, PRISMA_RNG_NS3, a tunnelled overlay with
 * log_capacity >= 2^18) or the memory-resident engine gets
 * PRISMA_ERR_CONFIG. */
int prisma_run_explore(prisma_env_t* env, int32_t policy, const void* policy_data,
                       int32_t max_hops, const uint32_t* explore_thr, void* stream);

/* The layout of an action history (prisma_run_explore_smart): one uint32
 * count per (node, action), T = the sum of the overlay degrees per replica.
 * row_out (host int32 [n_nodes + 1], or NULL): row[v] is the offset of node
 * v's first action, by underlay id, row[v + 1] - row[v] its overlay degree
 * (empty for a node outside the overlay), row[n_nodes] = T.  total_out: T.
 * Works for every env, whichever engine it runs on. */
int prisma_action_history_layout(prisma_env_t* env, int32_t* row_out, int32_t* total_out);

/* prisma_run_explore with history-weighted ("smart") exploration: the same
 * contract in every respect (policies, the repack, auto_reset, the
 * next-episode restart, explore_thr, the draw and the hit test), but an
 * exploring decision picks action i with probability proportional to
 * 1 - hist[i] / sum(hist) over the deciding node's row of a caller-owned
 * count of the actions taken, instead of uniformly, and every data decision
 * counts its action.  action_hist: device uint32 [n_replicas][T], laid out by
 * prisma_action_history_layout; the library never initialises it (the
 * reference starts at ones) and keeps no copy: it lives as long as the
 * caller's buffer, over launches and episodes.  For the decision of
 * prisma_run_explore's rule (d, e, v, deg, g, r, c as there):
 *
 *   hit  = (c[0] >> 8) < explore_thr[v]
 *   h_i  = action_hist[r][row[v] + i], i in [0, deg);  nb = sum h_i (uint64)
 *   w_i  = nb - h_i;  W = (deg - 1) * nb
 *   pick = W == 0 ? (uint32)(((uint64)c[1] * deg) >> 32)
 *                 : min { i : w_0 + ... + w_i > u },
 *          u = (uint64)(((unsigned __int128)(((uint64)c[1] << 32) | c[2]) * W) >> 64)
 *   a    = hit ? pick : g
 *   then, if 0 <= a < deg:  action_hist[r][row[v] + a] += 1
 *
 * w_i / W = (1 - h_i / nb) / (deg - 1).  W == 0 (deg = 1, or a row of zeros)
 * is prisma_run_explore's uniform pick.  The count is taken at every data
 * decision, explored or greedy, also where explore_thr[v] = 0 skips the
 * draw; a policy action outside [0, deg) (the packet is discarded) counts
 * nothing, and neither do destination arrivals and control packets.  The
 * counts are uint32 and wrap: with deg <= 55, W < 2^38, and the caller must
 * re-base a row (e.g. halve it) before one of its counts reaches 2^32.  Only
 * replica r's wave touches action_hist[r] during a launch; a host or another
 * stream must not write the buffer while a launch that uses it is in flight.
 * NULL explore_thr or action_hist, or hist_words != n_replicas * T:
 * PRISMA_ERR_ARG.  The kernels exist where prisma_run_explore's do: an env
 * whose prisma_kernel_info reports ctrl = 1 or the memory-resident engine
 * gets PRISMA_ERR_CONFIG.  (Added without an ABI version change: no struct or
 * signature moved.) */
int prisma_run_explore_smart(prisma_env_t* env, int32_t policy, const void* policy_data,
                             int32_t max_hops, const uint32_t* explore_thr,
                             uint32_t* action_hist, uint64_t hist_words, void* stream);

/* Fused stochastic multipath routing: the reference's "opt" agent
 * (forwarder.py:87-88, 192-194; utils.py:161-199 optimal_routing_decision),
 * whose action depends on the packet's source, on the flow fraction the
 * packet was assigned at its previous hop (its `tag`) and on a random draw.
 * The same contract as prisma_run (hop budget, auto_reset, the next-episode
 * restart), with a routing matrix in place of a policy.
 *
 * The tag.  The reference's tag is always routing[src][dst][the edge the
 * previous decision took] (both branches of optimal_routing_decision return
 * the fraction of the edge they chose; a new packet carries None), so it
 * needs no per-packet state: it follows from the previous decision record's
 * (node, action) and the packet's source.
 *
 * The float test made integer.  The reference's `tag in prob_to_neighbors and
 * tag < 1` compares float64 values.  The host gives every entry of
 * routing[s][t][:] a class: the distinct values x with 0 < x < 1 in ascending
 * order get classes 1, 2, ...; the value 0 and values >= 1 get class 0.  Two
 * entries are equal as float64 and below 1 exactly when their classes are
 * equal and non-zero.  At most 255 classes per (s, t).
 *
 * The table.  tab: device uint32 [NO][NO][T], s and t overlay indices (NO
 * overlay nodes; the node ids themselves on an identity overlay), T and
 * row[] those of prisma_action_history_layout (overlay CSR order: node
 * ascending, neighbour ascending -- list(G.edges) of the reference's
 * DiGraph).  Bits 24-31 of an entry hold the class, bits 0-23 the weight
 * wt = min(floor(p / rowsum * 2^24 + 0.5), 2^24 - 1), rowsum the float64 sum
 * of node v's deg entries for (s, t); 0 where rowsum == 0.
 *
 * The decision.  For data decision d (the numbering of the records' `prev`)
 * of episode e at node v of overlay degree deg, in replica r, for a packet
 * with source s, destination t and previous decision (u, a_u) or none:
 *
 *   c_prev = (prev exists and 0 <= a_u < deg(u)) ? cls(tab[s][t][row[u] + a_u]) : 0
 *   M      = { i < deg : cls(tab[s][t][row[v] + i]) == c_prev }
 *   if c_prev != 0 and M not empty:   a = min M                      (no draw)
 *   else:  c = philox4x32_10(ctr = {d, 0, e, 3}, key = {seed & 0xffffffff, replica_base + r})
 *          W = sum_i wt_i  (< 2^30 since deg <= 55)
 *          a = W == 0 ? (uint32)(((uint64)c[1] * deg) >> 32)
 *                     : min { i : wt_0 + ... + wt_i > u },  u = (uint32)(((uint64)c[1] * W) >> 32)
 *
 * Counter word 3 = 3 keeps the draw apart from the flow start offsets (0),
 * the send delays (1) and exploration (2).  Destination arrivals and control
 * packets draw nothing.  Defined, not copied: Philox replaces numpy's global
 * stream; probabilities are quantised to 24 bits (an edge below 2^-25 of its
 * row is never drawn); an all-zero row (a NaN and a crash in the reference)
 * takes the uniform pick.
 *
 * The source is the source of the arriving relay entry, or the arrival node
 * for a fresh packet.  On a tunnelled overlay the relay entries carry no
 * source: there it is the node of the first record of the packet's `prev`
 * chain, and a packet whose chain no longer lies within the last
 * log_capacity decisions sets PRISMA_EBIT_LOGWRAP (its decision is recorded
 * with action -1).
 *
 * `tab` is read during the launch and constant over it.  The kernels exist
 * for the register-resident engine without the ctrl paths: an env whose
 * prisma_kernel_info reports ctrl = 1 or the memory-resident engine gets
 * PRISMA_ERR_CONFIG; a NULL tab or tab_words != NO * NO * T is
 * PRISMA_ERR_ARG.  (Added without an ABI version change: no struct or
 * signature moved.) */
int prisma_run_stochastic(prisma_env_t* env, const uint32_t* tab, uint64_t tab_words,
                          int32_t max_hops, void* stream);

/* Copy per-replica counters (n_replicas entries) to host memory.
 * Synchronises `stream`. */
int prisma_read_counters(prisma_env_t* env, prisma_counters_t* host_out,
                         void* stream);

/* Device pointer to the per-replica counters array (prisma_counters_t
 * [n_replicas]), for device-side reductions / collectives. */
int prisma_counters_device(prisma_env_t* env, void** dev_ptr);

int prisma_log_view(prisma_env_t* env, prisma_log_view_t* out);

/* Device-to-device copy of the whole log ring ([n_replicas][log_capacity]
 * records) into caller memory of at least `bytes` bytes, on `stream`. */
int prisma_copy_log(prisma_env_t* env, void* dst_device, uint64_t bytes, void* stream);

/* Device-to-device copy of the counters (prisma_counters_t [n_replicas]). */
int prisma_copy_counters(prisma_env_t* env, void* dst_device, void* stream);

/* Gather n decision records, record dec[i] of replica replica[i] (both
 * device arrays), into dst_device (n * record_bytes bytes).  The caller
 * keeps dec[i] within the last log_capacity decisions of that replica. */
int prisma_gather_records(prisma_env_t* env, const int32_t* replica, const uint32_t* dec,
                          int32_t n, void* dst_device, void* stream);

/*
 * Per-node replay rings of a trainer (prisma_ingest_transitions): one FIFO ring of `size`
 * transitions per node (replay_buffer.py:29-37), as contiguous device arrays in the layouts of
 * prisma_amd.trainer.ReplayBuffers; N = n_nodes, W = obs_width, rows by underlay node id.
 */
typedef struct prisma_replay {
    int32_t* obs;               /* [N][size][W]                            */
    int32_t* next_obs;          /* [N][size][W]                            */
    int64_t* action;            /* [N][size]                               */
    float*   reward;            /* [N][size]                               */
    uint8_t* done;              /* [N][size], 0 / 1                        */
    int64_t* replica;           /* [N][size]: the replica an item came from */
    int64_t* next_idx;          /* [N]: the slot the node's next item takes */
    int64_t* count;             /* [N]: items in the ring, <= size         */
    int64_t* total;             /* [N]: items ever added                   */
    int64_t  size;
    int32_t  n_nodes;
    int32_t  obs_width;
} prisma_replay_t;

/*
 * The replay transitions completed since the previous call, from the decision log straight into
 * the rings: three launches on `stream`, no host read, no atomic deciding a slot (placement
 * follows from prefix sums, so the result is deterministic).  It has exactly the effect of
 * VecRoutingEnv.transitions() followed by ReplayBuffers.add() on a non-prioritized buffer,
 * together with the update of the caller's progress mark: consumed, device int64 [n_replicas],
 * the index of each replica's first record not yet turned into transitions (zeros after a reset).
 *
 * The rule per replica r, with dec its dec_count and cap = log_capacity:
 *   Window.    The new records are d in [lo, dec), lo = max(consumed[r], dec - cap + 1).  A
 *              record is final if its status is not PRISMA_ST_PENDING.
 *   Consumed.  If the window is non-empty, consumed[r] = dec - (1 if the window's last record
 *              is pending else 0); otherwise consumed[r] is unchanged.
 *   Hop item.  A final record d with prev >= 0 yields (obs_p, action_p, (float)reward_d, obs_d,
 *              status_d == PRISMA_ST_DESTINATION, node_p, r), p being the record at slot
 *              prev mod cap of the same replica.
 *   Loss item. A final record d with status PRISMA_ST_DROPPED yields (obs_d, action_d,
 *              (float)loss_penalty, [obs_d[0], 0, ...], true, node_d, r).
 *   Batch order.  All hop items first, in (r, d) ascending order; all loss items follow, in
 *              (r, d) ascending order.
 *   Rank.      Within that order, an item's rank among the items of its node u gives slot
 *              (next_idx[u] + rank) mod size.
 *   Overflow.  An item is written only if rank >= count_u - size, count_u being the node's items
 *              in this call: an overflowing batch keeps its last `size` items.
 *   Ring counters.  Afterwards next_idx[u] = (next_idx[u] + count_u) mod size, count[u] =
 *              min(count[u] + count_u, size), total[u] += count_u.
 *   Field encoding.  The action is the record's sign-extended int8; the reward conversion is
 *              round-to-nearest-even.
 * An item whose node id is >= n_nodes is skipped in every pass (the engines write none).
 * Either engine's log.  Null env, consumed, rings or ring pointer, size < 1, or rings->obs_width /
 * rings->n_nodes different from the env's: PRISMA_ERR_ARG, nothing is launched.  The per-(replica,
 * node) counts and offsets live in library-owned scratch, allocated at the first call and freed
 * by prisma_destroy; calls on one env are ordered by their stream.  (Added without an ABI
 * version change: no struct or signature moved.)
 */
int prisma_ingest_transitions(prisma_env_t* env, int64_t* consumed, const prisma_replay_t* rings,
                              void* stream);

/*
 * The stored Q networks a replay batch's bootstrap targets are computed against
 * (prisma_replay_targets): n_gen weight generations of one model, each a packed fp32 network set
 * (row-major, x @ W, N = n_nodes, D = max_deg, rows by underlay id, (B, H, NH) as in the table
 * above).  The DQN-buffer kinds take exactly the layouts of PRISMA_POLICY_DQN_BUFFER ...
 * _DQN_LIGHTER_3 (StackedQNet.pack()).  PRISMA_QMODEL_ROUTING is DQN_routing_model
 * (models.py:360-392), the 64-wide layout without the buffers branch:
 *   W1[N][N][32] b1[N][32] W2[N][32][64] b2[N][64] W3[N][64][64] b3[N][64] W4[N][64][D] b4[N][D]
 */
#define PRISMA_QMODEL_ROUTING  0
typedef struct prisma_qnets {
    const float* const* weights;  /* device array [n_gen] of device pointers, one packed network set each */
    int32_t  n_gen;               /* >= 1 */
    int32_t  model;               /* PRISMA_QMODEL_ROUTING (0), or PRISMA_POLICY_DQN_BUFFER ... _DQN_LIGHTER_3 */
    const int32_t* gen_of;        /* device int32 [n_replicas][T], T and row[] of prisma_action_history_layout:
                                     the generation that (replica r, node u, action a) reads, at
                                     gen_of[r][row[u] + a]; NULL = generation 0 everywhere */
} prisma_qnets_t;

/*
 * The bootstrap targets of a sampled replay batch against every stored generation: what
 * ReplayBuffers.sample_full() followed by QRoutingTrainer.targets() computes, as one launch on
 * `stream` with no host read.  idx: device int64 [N][batch], a ring slot per (node, batch
 * position).  Outputs are device arrays with row i = u * batch + b: obs_out int32 [N * batch][W],
 * action_out int64 [N * batch], target_out float [N * batch], status_out uint8 [N * batch];
 * obs_out, action_out and status_out may be NULL.  Either engine: the call reads only the rings,
 * the weights and the env's overlay CSR (row[], the next node and the back action per (u, a), a
 * small device table built from the env's host topology at the first call and freed by
 * prisma_destroy).
 *
 * The rule, for row i = (u, b) with s = idx[u][b]:
 *   Slot.      s outside [0, rings->size): obs_out[i] = zeros, action_out[i] = 0, target = +0,
 *              status = 2; nothing of the rings is read.
 *   Gather.    a = rings->action[u][s], rew, done, r = rings->replica[u][s], next_obs[u][s][:];
 *              obs_out[i] = rings->obs[u][s][:], action_out[i] = a.
 *   Not evaluable.  a outside [0, deg(u)) (every node without an agent), r outside
 *              [0, n_replicas), or the generation g = gen_of[r][row[u] + a] outside [0, n_gen); or,
 *              for an item that is not done, next_obs[0] (the one-hot input) outside [0, N):
 *              target = rew, status = 2.  No out-of-range address is ever formed, and the value
 *              is whatever finite reward the ring holds, never a NaN of the call's making.
 *   Done.      target = rew, status = 1.
 *   Otherwise  (status = 0): v = the a-th overlay neighbour of u, bk = the action of v that leads
 *              back to u (or none); q[0 .. deg(v)) = the fp32 Q values of generation g's network
 *              at node v on next_obs in the fixed operation order of the in-kernel DQN-buffer
 *              decision (the routing model takes the same order with the one-hot
 *              branch alone feeding layer 2);
 *                best = +inf; for j in 0 .. deg(v) - 1: if j != bk and q[j] < best: best = q[j]
 *                target = fadd_rn(rew, fmul_rn(gamma, best))
 *              An empty candidate set gives +inf; a NaN Q never wins (defined, not copied:
 *              torch's min would propagate it).
 * Null env, rings, idx, nets, nets->weights or target_out, a null ring array the rule reads,
 * batch < 1, n_gen < 1, rings->size < 1, model == PRISMA_POLICY_TABLE or unknown, or rings->n_nodes /
 * rings->obs_width different from the env's: PRISMA_ERR_ARG, nothing is launched.  The arguments
 * that need no env are checked first.  (Added without an ABI version change: no struct or
 * signature moved.)
 */
int prisma_replay_targets(prisma_env_t* env, const prisma_replay_t* rings, const int64_t* idx,
                          int32_t batch, const prisma_qnets_t* nets, float gamma,
                          int32_t* obs_out, int64_t* action_out, float* target_out,
                          uint8_t* status_out, void* stream);

/* Active-replica compaction (ABI 9) for a batched external policy, which then
 * evaluates only the replicas with a pending decision -- the reference's
 * Forwarder steps only the nodes that were notified (ns3env.py:417-423,
 * forwarder.py:135-195).  From the outputs of a prisma_step (mask [R], obs
 * [R][obs_width], node [R]; obs / node may be NULL): ids_out[0..count) = the
 * replica ids with mask 1 in ascending order, obs_packed[i] = obs row of
 * ids_out[i], node_packed[i] = its deciding node, count_out[0] = count (all
 * device int32; obs_packed / node_packed may be NULL).  A wavefront ballot and
 * a prefix sum of the wave totals; one launch on `stream`, no host sync. */
int prisma_compact_pending(prisma_env_t* env, const uint8_t* mask, const int32_t* obs,
                           const int32_t* node, int32_t* ids_out, int32_t* obs_packed,
                           int32_t* node_packed, int32_t* count_out, void* stream);

/* The inverse for the actions: actions_out[r] = fill for every replica, then
 * actions_out[ids[i]] = packed_actions[i] for i < count[0] (device arrays);
 * actions_out then feeds prisma_step. */
int prisma_expand_actions(prisma_env_t* env, const int32_t* ids, const int32_t* count,
                          const int32_t* packed_actions, int32_t fill, int32_t* actions_out,
                          void* stream);

/* The step-kernel instances prisma_create picked for this env (ABI 10), as
 * the library decided, for profiles and tests (the demangled kernel name is
 * prisma_step_kernel_t<flow_slots, link_slots, MLP, tunnels, ctrl> on the
 * register engine, prisma_mem_step_kernel<MLP, ctrl> on the memory engine). */
typedef struct prisma_kernel_info {
    uint32_t engine;            /* PRISMA_ENGINE_REGISTER or _MEMORY       */
    int32_t  flow_slots;        /* template slots (register engine; else 0) */
    int32_t  link_slots;
    uint32_t tunnels;           /* tunnelled-overlay instances              */
    uint32_t ctrl;              /* --train / notify_dest / ns-3 stream paths
                                   compiled in (also: tunnelled overlays with
                                   log_capacity >= 2^18)                    */
    uint32_t relay_ip;          /* relay entries carry (decision, TTL, tunnel
                                   target) and FIFO windows sit in LDS       */
    uint32_t relay_dec_bits;    /* decision-index bits of a relay entry (18
                                   with relay_ip, 22 otherwise; 0 without
                                   tunnels): the log-wrap check sees ages up
                                   to 2^bits                               */
} prisma_kernel_info_t;
int prisma_kernel_info(prisma_env_t* env, prisma_kernel_info_t* out);

/* Bytes of per-replica state (the LDS image) and LDS bytes per workgroup. */
int prisma_state_bytes(prisma_env_t* env, uint32_t* state_bytes,
                       uint32_t* lds_bytes);

/* Sizing without a device: validates topo/params exactly as prisma_create
 * does and reports the per-replica footprint (any pointer may be NULL). */
typedef struct prisma_plan {
    uint32_t state_bytes;       /* HBM state image per replica             */
    uint32_t lds_bytes;         /* LDS per workgroup (= per replica)       */
    uint32_t lds_state_bytes;   /* LDS part of the image                   */
    uint32_t ring_entries;      /* packet slots over all link FIFOs        */
    uint32_t record_bytes;      /* decision record size                    */
    int32_t  obs_width;
    int32_t  flow_slots;        /* register slots per lane (64 flows each) */
    int32_t  link_slots;        /* register slots per lane (64 links each) */
    uint32_t engine;            /* PRISMA_ENGINE_REGISTER or _MEMORY       */
} prisma_plan_t;
int prisma_plan(const prisma_topology_t* topo, const prisma_params_t* params, prisma_plan_t* out);

/*
 * Traffic scenarios: replicas of one env that differ in their flow rates (traffic matrix, load
 * factor), advanced by the same launches.  The flow LIST (n_flows, flow_src, flow_dst) and the rest
 * of the topology are those of `topo` for every scenario; scenario s gives flow f the bit rate
 * flow_rate_bps[s * n_flows + f], and replica r (local index, 0 .. n_replicas - 1) runs scenario
 * scenario_of[r].  Everything else of a replica -- its Philox key (seed, replica_base + r), its
 * ns-3 streams, sizing, kernels -- is what prisma_create gives it, so replica r equals the replica
 * with the same global id of a single-scenario env on scenario_of[r]'s rates.
 *
 * With a scenario set the rates come from it: topo->flow_rate_bps is not read, but must still be
 * non-null, as prisma_create requires.  prisma_create(topo, ...) IS prisma_create_scenarios with
 * n_scenarios = 1, row 0 = topo->flow_rate_bps and every replica in scenario 0 (one code path:
 * state, log and counters are byte-identical either way).
 *
 * The device holds one read-only topology image per scenario, back to back, and a replica binds
 * its scenario's image by a 32-bit byte offset: n_scenarios <= PRISMA_MAX_SCENARIOS and
 * n_scenarios * (image bytes rounded up to 256) < 2^32 (prisma_scenario_plan_t.topo_bytes), else
 * PRISMA_ERR_CONFIG.
 *
 * PRISMA_ERR_ARG: a null scenarios / flow_rate_bps / scenario_of, n_scenarios < 1 (and what
 * prisma_create refuses); PRISMA_ERR_CONFIG: a zero rate, a scenario_of entry outside
 * [0, n_scenarios), too many scenarios.  The message names the argument.  Both arrays are host
 * memory, copied by the call.  (Added without an ABI version change: no struct or signature moved.)
 */
#define PRISMA_MAX_SCENARIOS 65535
typedef struct prisma_scenarios {
    int32_t n_scenarios;            /* S >= 1 */
    const uint64_t* flow_rate_bps;  /* [S][topo->n_flows], every entry > 0 */
    const int32_t*  scenario_of;    /* [n_replicas], each in [0, S); local replica index */
} prisma_scenarios_t;

int prisma_create_scenarios(const prisma_topology_t* topo, const prisma_params_t* params,
                            const prisma_scenarios_t* scenarios, int32_t n_replicas, int32_t device,
                            prisma_env_t** out);

/* prisma_plan for a scenario set: the same validation as prisma_create_scenarios, no device; `out`
 * reports what prisma_plan does (the per-replica footprint does not depend on the rates). */
int prisma_plan_scenarios(const prisma_topology_t* topo, const prisma_params_t* params,
                          const prisma_scenarios_t* scenarios, int32_t n_replicas, prisma_plan_t* out);

/* ... and the read-only topology images of the set, which prisma_plan_t has no room for
 * (its size is fixed): the same validation once more. */
typedef struct prisma_scenario_plan {
    uint64_t topo_bytes;        /* device bytes of all scenarios' topology images */
    uint32_t image_bytes;       /* one image                                       */
    int32_t  n_scenarios;
} prisma_scenario_plan_t;
int prisma_plan_scenario_images(const prisma_topology_t* topo, const prisma_params_t* params,
                                const prisma_scenarios_t* scenarios, int32_t n_replicas,
                                prisma_scenario_plan_t* out);

/* The env's scenario count and (scenario_of_out non-null: host int32 [n_replicas]) each replica's
 * scenario; 1 and zeros for an env made by prisma_create.  Either pointer may be NULL. */
int prisma_scenario_info(prisma_env_t* env, int32_t* n_scenarios, int32_t* scenario_of_out);

/*
 * Per-scenario sums of the replicas' counters: one launch on `stream`, no host read.  out_device:
 * device prisma_scenario_stats_t [n_scenarios].  One wavefront per scenario walks that scenario's
 * replicas in ascending replica index (a host-built CSR that prisma_create / prisma_create_scenarios
 * put on the device, so the call itself allocates and copies nothing).
 *
 * Integer fields are exact sums (uint64 / int64; the 32-bit counters widened first).  n_error counts
 * the replicas with error != 0, n_over those with episode_over != 0.
 *
 * The f64 sums are in a fixed order, independent of the launch shape, so a host can restate them
 * bit for bit (prisma_amd/scenarios.py stats_sum): with x_0 .. x_{n-1} the scenario's values in
 * ascending replica index (the float counters converted to double, which is exact),
 *     lane l (0 <= l < 64):  a_l = +0.0;  for p = l, l + 64, l + 128, ... < n:  a_l = a_l + x_p
 *     for h = 32, 16, 8, 4, 2, 1:  for l < h:  a_l = a_l + a_{l + h}       (all l of a level at once)
 *     sum = a_0
 * every addition an IEEE-754 binary64 round-to-nearest-even add, none fused or reassociated.
 */
typedef struct prisma_scenario_stats {
    uint64_t n_replicas;        /* replicas of the scenario                 */
    uint64_t n_error;           /* ... with error != 0                      */
    uint64_t n_over;            /* ... with episode_over != 0               */
    uint64_t events, hops, decisions, hop_deg_sum;
    int64_t  now_ns;
    int64_t  ov_injected, ov_arrived, ov_lost, un_injected, un_arrived, un_lost;
    int64_t  bytes_data, bytes_signaling, cost_n, e2e_n, un_cost_n;
    uint64_t episode, ping_rounds, seq, uid, dec_count, ctrl_dropped;
    uint64_t hops_total, events_total;
    double   reward_sum, cost_sum, e2e_sum, un_cost_sum;
} prisma_scenario_stats_t;
int prisma_scenario_stats(prisma_env_t* env, prisma_scenario_stats_t* out_device, void* stream);

void prisma_destroy(prisma_env_t* env);

#ifdef __cplusplus
}
#endif
#endif /* PRISMA_AMD_PRISMA_H */
