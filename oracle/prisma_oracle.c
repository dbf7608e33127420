/*
 * prisma_oracle.c — TEST INFRASTRUCTURE ONLY (see prisma_oracle.h).
 *
 * Literal single-replica restatement of the reference's ns-3 scenario for
 * identity and tunnelled overlays.  Every handler cites the reference callback it
 * restates (paths relative to the reference root, prisma/ns3/ unless
 * noted).  ns-3 upstream semantics that are not in the reference tree are
 * stated from the ns-3 API:
 *   - Time is int64 nanoseconds; Seconds(x) is restated as
 *     (int64)(x * 1e9 + 0.5) for x >= 0 (round-to-nearest);
 *   - Time::GetSeconds() is restated as (double)t / 1e9;
 *   - DataRate::CalculateBytesTxTime(b) = Seconds((double)b * 8 / bps);
 *   - byte-mode Queue::DoEnqueue drops iff nbytes + size > max;
 *   - PointToPointChannel delivers at start + txTime + delay;
 *   - the scheduler runs events in (time, insertion uid) order.
 * RNG: ns-3's MRG32k3a streams are replaced by a counter-based
 * Philox4x32-10 (Salmon et al., SC'11 / Random123), keyed by
 * (seed, replica) with counter (flow, draw, episode, purpose); parity with
 * real ns-3 draws is unpinned.
 *
 * Build: cc -O2 -std=c11 -ffp-contract=off -fPIC -shared (oracle/Makefile).
 */
#include "prisma_oracle.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* RNG + numeric helpers                                               */
/* ------------------------------------------------------------------ */
void or_philox4x32_10(const uint32_t ctr_in[4], const uint32_t key_in[2], uint32_t out[4]) {
    uint32_t c0 = ctr_in[0], c1 = ctr_in[1], c2 = ctr_in[2], c3 = ctr_in[3];
    uint32_t k0 = key_in[0], k1 = key_in[1];
    for (int round = 0; round < 10; ++round) {
        uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
        uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        uint32_t n0 = hi1 ^ c1 ^ k0;
        uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* Natural log by range reduction + atanh series; only + - * / so the
 * result is identical on every IEEE-754 double implementation. */
double or_det_log(double x) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    int e = (int)((bits >> 52) & 0x7ff) - 1023;
    bits = (bits & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL;
    double m;
    memcpy(&m, &bits, 8);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    double f = m - 1.0;
    double s = f / (2.0 + f);
    double z = s * s;
    double p = 2.0 / 19.0;
    p = p * z + 2.0 / 17.0;
    p = p * z + 2.0 / 15.0;
    p = p * z + 2.0 / 13.0;
    p = p * z + 2.0 / 11.0;
    p = p * z + 2.0 / 9.0;
    p = p * z + 2.0 / 7.0;
    p = p * z + 2.0 / 5.0;
    p = p * z + 2.0 / 3.0;
    double logm = 2.0 * s + s * (z * p);
    double de = (double)e;
    return de * 6.93147180369123816490e-01 + (de * 1.90821492927058770002e-10 + logm);
}

int64_t or_seconds_to_ns(double s) { return (int64_t)(s * 1e9 + 0.5); }

static double get_seconds(int64_t t) { return (double)t / 1e9; }

/* Microseconds that Python reads back from std::to_string(GetSeconds())
 * ("%f": the double rounded to 6 decimals, ties to even on the exact
 * binary value) — packet-manager.cc:127-128 -> forwarder.py:208. */
uint64_t or_py_micros(int64_t t) {
    uint64_t u = (uint64_t)(t / 1000);
    int64_t r = t % 1000;
    if (r < 500) return u;
    if (r > 500) return u + 1;
    double x = get_seconds(t);
    uint64_t b;
    memcpy(&b, &x, 8);
    int ex = (int)((b >> 52) & 0x7ff);
    uint64_t mant = b & 0x000fffffffffffffULL;
    if (ex == 0) ex = 1; else mant |= 0x0010000000000000ULL;
    int sh = -(ex - 1075);               /* x = mant * 2^-(sh) */
    unsigned __int128 lhs = (unsigned __int128)mant * 2000000u;
    unsigned __int128 rhs = (unsigned __int128)(2 * u + 1);
    if (sh >= 0) rhs <<= sh; else lhs <<= -sh;
    if (lhs > rhs) return u + 1;
    if (lhs < rhs) return u;
    return (u & 1) ? u + 1 : u;
}

static double py_reward(int64_t t1, int64_t t0) {
    return (double)or_py_micros(t1) / 1e6 - (double)or_py_micros(t0) / 1e6;
}

/* ------------------------------------------------------------------ */
/* record / counter layouts (byte-identical to include/prisma.h)       */
/* ------------------------------------------------------------------ */
typedef struct {
    int64_t t_ns; uint32_t uid; int32_t prev; double reward;
    uint8_t node; uint8_t dst; uint16_t start_s; int8_t action; uint8_t status; uint8_t ttl; uint8_t episode;
} rec_head_t;

typedef struct {
    uint64_t events, hops, decisions, hop_deg_sum;
    int64_t now_ns;
    double reward_sum;
    int32_t ov_injected, ov_arrived, ov_lost, un_injected, un_arrived, un_lost;
    int32_t bytes_data, bytes_signaling;
    float cost_sum, e2e_sum;
    int32_t cost_n, e2e_n;
    uint32_t episode, ping_rounds, seq, uid, dec_count, ctrl_dropped, error, episode_over;
    uint64_t hops_total, events_total;
    float un_cost_sum; int32_t un_cost_n;
} counters_t;

enum { ST_PENDING = 0, ST_ENQUEUED = 1, ST_DROPPED = 2, ST_DEST = 3, ST_DISCARDED = 4 };
enum { DATA_PACKET = 0, BIG_SIGN_PACKET = 1, SMALL_SIGN_PACKET = 2, PING_FORWARD_PACKET = 3, PING_BACK_PACKET = 4 };   /* enum-and-constants.h:5-11 */
enum { EV_PING = 0, EV_START = 1, EV_SEND = 2, EV_COMPLETE = 3, EV_RECEIVE = 4, EV_BSTART = 5, EV_BSEND = 6 };

/* ------------------------------------------------------------------ */
/* simulation objects                                                  */
/* ------------------------------------------------------------------ */
typedef struct {              /* MyTag (my-tag.h:49-65) + size */
    int type, src, dst, next_hop, last_hop;
    uint64_t start_time;      /* data: whole seconds; ping: ms          */
    int valable;
    uint32_t uid, ping_idx;   /* big signalling: ping_idx = send index n of its generator */
    int tunnel;               /* ping: the origin's local tunnel index      */
    int ttl;                  /* IP TTL (data: 255 at the app, :330)       */
    float one_hop_delay;
    uint32_t size;            /* bytes incl. PPP header                 */
    int next_free;
} pkt_t;

typedef struct { int64_t t; uint64_t seq; int kind, id, pkt; } ev_t;

typedef struct {              /* PointToPointNetDevice + DropTailQueue   */
    int busy;
    int *q; int q_cap, q_head, q_len;
    uint32_t nbytes;
    uint64_t bps;
    int64_t delay;
    uint32_t max_bytes;       /* byte mode if > 0                       */
    uint32_t max_pkts;        /* packet mode otherwise                  */
    int from_node, to_node, is_access;
    int wire;                 /* or_diag: packets between transmit_start and their receive */
} netdev_t;

typedef struct { uint32_t idx; uint64_t ms; } sent_t;
typedef struct { sent_t* a; int n, cap; } sentvec_t;
typedef struct { float* a; int n, cap; } fvec_t;
typedef struct { uint32_t* a; int n, cap; } uvec_t;

typedef struct {              /* temp_obs entry (forwarder.py:153-159) */
    int64_t dec; int64_t t_ns; int active;
} temp_t;

/* ---- ns-3 random streams (rng_mode 1): RngStream, rng-stream.cc --------------------------
 * MRG32k3a (L'Ecuyer 1999) with the package's stream construction: a RandomVariableStream
 * created k-th in a run draws from RngStream(seed, k, run): all six state words = seed, then
 * AdvanceNthBy(k, 127) and AdvanceNthBy(run, 76), i.e. for every set bit i of k the state is
 * multiplied by A^(2^(127+i)) (and likewise for the run with 76).  RandU01 is the package's
 * double arithmetic. */
static const uint64_t or_m1 = 4294967087ull, or_m2 = 4294944443ull;

static void mrg_matmul(const uint64_t* X, const uint64_t* Y, uint64_t* Z) {   /* [18] each */
    uint64_t t[18];
    for (int c = 0; c < 2; ++c) {
        const uint64_t m = c ? or_m2 : or_m1;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                uint64_t acc = 0;
                for (int k = 0; k < 3; ++k) acc = (acc + X[9 * c + 3 * i + k] * Y[9 * c + 3 * k + j] % m) % m;
                t[9 * c + 3 * i + j] = acc;
            }
    }
    memcpy(Z, t, sizeof(t));
}

void or_mrg_pow2(int e, uint64_t out[18]) {
    uint64_t A[18] = { 0, 1, 0, 0, 0, 1, or_m1 - 810728u, 1403580u, 0,
                       0, 1, 0, 0, 0, 1, or_m2 - 1370589u, 0, 527612u };
    for (int i = 0; i < e; ++i) mrg_matmul(A, A, A);
    memcpy(out, A, sizeof(A));
}

static void mrg_matvec(const uint64_t* M, uint64_t* v) {
    uint64_t r[6];
    for (int c = 0; c < 2; ++c) {
        const uint64_t m = c ? or_m2 : or_m1;
        for (int i = 0; i < 3; ++i) {
            uint64_t acc = 0;
            for (int k = 0; k < 3; ++k) acc = (acc + M[9 * c + 3 * i + k] * v[3 * c + k] % m) % m;
            r[3 * c + i] = acc;
        }
    }
    memcpy(v, r, sizeof(r));
}

static double mrg_rand_u01(uint64_t* st) {                      /* RngStream::RandU01 */
    double p1 = 1403580.0 * (double)st[1] - 810728.0 * (double)st[0];
    int64_t k = (int64_t)(p1 / 4294967087.0);
    p1 -= (double)k * 4294967087.0;
    if (p1 < 0.0) p1 += 4294967087.0;
    st[0] = st[1]; st[1] = st[2]; st[2] = (uint64_t)p1;
    double p2 = 527612.0 * (double)st[5] - 1370589.0 * (double)st[3];
    k = (int64_t)(p2 / 4294944443.0);
    p2 -= (double)k * 4294944443.0;
    if (p2 < 0.0) p2 += 4294944443.0;
    st[3] = st[4]; st[4] = st[5]; st[5] = (uint64_t)p2;
    return (p1 > p2) ? (p1 - p2) * 2.328306549295727688e-10 : (p1 - p2 + 4294967087.0) * 2.328306549295727688e-10;
}

/* A^(2^(127+i)) for i < 64 and A^(2^(76+i)) for i < 64, built once */
static uint64_t g_mrg_p127[64][18], g_mrg_p76[64][18];
static int g_mrg_ready = 0;
static void mrg_tables(void) {
    if (g_mrg_ready) return;
    uint64_t A[18];
    or_mrg_pow2(76, A);
    for (int i = 0; i < 51 + 64; ++i) {         /* A = A^(2^(76+i)); 76 + 51 = 127 */
        if (i < 64) memcpy(g_mrg_p76[i], A, sizeof(A));
        if (i >= 51) memcpy(g_mrg_p127[i - 51], A, sizeof(A));
        mrg_matmul(A, A, A);
    }
    g_mrg_ready = 1;
}

static void mrg_stream_state(uint32_t seed, uint64_t stream, uint64_t run, uint64_t st[6]) {
    mrg_tables();
    for (int i = 0; i < 6; ++i) st[i] = seed;
    for (int i = 0; i < 64; ++i) if ((stream >> i) & 1u) mrg_matvec(g_mrg_p127[i], st);   /* AdvanceNthBy(stream, 127) */
    for (int i = 0; i < 64; ++i) if ((run >> i) & 1u) mrg_matvec(g_mrg_p76[i], st);       /* AdvanceNthBy(run, 76) */
}

double or_mrg_first_u01(uint32_t seed, uint64_t stream, uint64_t run) {
    uint64_t st[6];
    mrg_stream_state(seed, stream, run, st);
    return mrg_rand_u01(st);
}

struct or_sim {
    or_config_t c;
    uint64_t rv_next;           /* rng_mode 1: stream of the next RandomVariable object created */
    int N, E, F, W;
    int64_t t_end, ping_period, now;
    uint64_t seq;
    /* heap */
    ev_t* heap; int hn, hcap;
    /* packets */
    pkt_t* pk; int pk_cap, pk_free;
    netdev_t* dev;                 /* E switch devices + N access devices   */
    int* flow_draws;
    double* flow_mean;
    uint32_t* ping_index;       /* per node m_pingPacketIndex            */
    sentvec_t* unacked;         /* per tunnel (node, local index)        */
    fvec_t* delays;
    uvec_t* lost;               /* per node m_lostPackets (uids)         */
    uint32_t* echo_payload;     /* per node: small-signalling payload (sim.cc:373-392) */
    int G;                      /* big-signalling generators (sim.cc:634-647), flow order */
    int *g_src, *g_dst, *g_draws;
    int64_t bs_period;          /* ScheduleNextTx delay (big-signaling-application.cc:247-250) */
    uint32_t bs_nseg;           /* segments per NN copy: m_pktSizeMean / m_segSize      */
    temp_t* temp; int64_t temp_cap;
    uint32_t next_uid;
    counters_t cnt;
    /* records */
    unsigned char* rec; int64_t rec_n, rec_cap; int rec_bytes;
    /* pending decision */
    int pend; int pend_pkt, pend_node, pend_link; int64_t pend_rec; int pend_dest; int pend_ctrl;
    int over;
    /* trace */
    int trace_on; int64_t* tr; int64_t tr_n, tr_cap;
    /* last info string */
    char info[4096];
    /* test diagnostics (or_diag): data packets dropped on a FIFO inside a tunnel */
    int64_t relay_drops;
    /* the most packets at once between transmit_start and their channel receive on one switch
     * link (max_wire), and the most queued + on the wire there (peak_ring: what a ring holds) */
    int64_t max_wire, peak_ring;
};

static void* xrealloc(void* p, size_t n) {
    void* q = realloc(p, n);
    if (!q && n) { fprintf(stderr, "oracle: out of memory\n"); abort(); }
    return q;
}

static int ev_less(const ev_t* a, const ev_t* b) {
    return a->t < b->t || (a->t == b->t && a->seq < b->seq);
}

static void schedule(or_sim_t* s, int64_t t, int kind, int id, int pkt) {
    if (s->hn == s->hcap) { s->hcap = s->hcap ? 2 * s->hcap : 256; s->heap = xrealloc(s->heap, sizeof(ev_t) * s->hcap); }
    ev_t e = { t, s->seq++, kind, id, pkt };
    int i = s->hn++;
    while (i > 0) {
        int p = (i - 1) / 2;
        if (!ev_less(&e, &s->heap[p])) break;
        s->heap[i] = s->heap[p];
        i = p;
    }
    s->heap[i] = e;
}

static ev_t heap_pop(or_sim_t* s) {
    ev_t top = s->heap[0];
    ev_t last = s->heap[--s->hn];
    int i = 0;
    for (;;) {
        int l = 2 * i + 1, r = l + 1, m = i;
        const ev_t* mv = &last;
        if (l < s->hn && ev_less(&s->heap[l], mv)) { m = l; mv = &s->heap[l]; }
        if (r < s->hn && ev_less(&s->heap[r], mv)) { m = r; mv = &s->heap[r]; }
        if (m == i) break;
        s->heap[i] = s->heap[m];
        i = m;
    }
    if (s->hn > 0) s->heap[i] = last;
    return top;
}

static int pkt_alloc(or_sim_t* s) {
    if (s->pk_free < 0) {
        int old = s->pk_cap;
        s->pk_cap = old ? old * 2 : 1024;
        s->pk = xrealloc(s->pk, sizeof(pkt_t) * s->pk_cap);
        for (int i = old; i < s->pk_cap; ++i) s->pk[i].next_free = (i + 1 < s->pk_cap) ? i + 1 : -1;
        s->pk_free = old;
    }
    int i = s->pk_free;
    s->pk_free = s->pk[i].next_free;
    memset(&s->pk[i], 0, sizeof(pkt_t));
    s->pk[i].next_free = -2;
    return i;
}

static void pkt_free(or_sim_t* s, int i) { s->pk[i].next_free = s->pk_free; s->pk_free = i; }

static void q_push(netdev_t* d, int p) {
    if (d->q_len == d->q_cap) {
        int nc = d->q_cap ? d->q_cap * 2 : 64;
        int* nq = xrealloc(NULL, sizeof(int) * nc);
        for (int i = 0; i < d->q_len; ++i) nq[i] = d->q[(d->q_head + i) % d->q_cap];
        free(d->q);
        d->q = nq; d->q_cap = nc; d->q_head = 0;
    }
    d->q[(d->q_head + d->q_len) % d->q_cap] = p;
    d->q_len++;
}

static int q_pop(netdev_t* d) {
    int p = d->q[d->q_head];
    d->q_head = (d->q_head + 1) % d->q_cap;
    d->q_len--;
    return p;
}

#define VEC_PUSH(v, x) do { if ((v)->n == (v)->cap) { (v)->cap = (v)->cap ? 2 * (v)->cap : 8; \
    (v)->a = xrealloc((v)->a, sizeof(*(v)->a) * (v)->cap); } (v)->a[(v)->n++] = (x); } while (0)

static void vec_erase(void* base, int* n, int elem, int i) {
    unsigned char* b = (unsigned char*)base;
    memmove(b + (size_t)i * elem, b + (size_t)(i + 1) * elem, (size_t)(*n - i - 1) * elem);
    (*n)--;
}

static temp_t* temp_of(or_sim_t* s, uint32_t uid) {
    if ((int64_t)uid >= s->temp_cap) {
        int64_t nc = s->temp_cap ? s->temp_cap : 1024;
        while (nc <= (int64_t)uid) nc *= 2;
        s->temp = xrealloc(s->temp, sizeof(temp_t) * nc);
        memset(s->temp + s->temp_cap, 0, sizeof(temp_t) * (nc - s->temp_cap));
        s->temp_cap = nc;
    }
    return &s->temp[uid];
}

static rec_head_t* rec_at(or_sim_t* s, int64_t d) { return (rec_head_t*)(s->rec + (size_t)d * s->rec_bytes); }

static int64_t rec_new(or_sim_t* s) {
    if (s->rec_n == s->rec_cap) {
        s->rec_cap = s->rec_cap ? 2 * s->rec_cap : 4096;
        s->rec = xrealloc(s->rec, (size_t)s->rec_cap * s->rec_bytes);
    }
    int64_t d = s->rec_n++;
    memset(s->rec + (size_t)d * s->rec_bytes, 0, s->rec_bytes);
    return d;
}

/* ------------------------------------------------------------------ */
/* ComputeStats (compute-stats-v2.cc:87-217) as running sums           */
/* ------------------------------------------------------------------ */
static void add_loss_penalty_to_cost(or_sim_t* s) {                /* :123-126 */
    s->cnt.cost_sum += (float)s->c.loss_penalty;
    s->cnt.cost_n++;
}

/* ------------------------------------------------------------------ */
/* PointToPointNetDevice (point-to-point-net-device.cc)                 */
/* ------------------------------------------------------------------ */
static int64_t tx_time(const netdev_t* d, uint32_t bytes) {           /* :289 */
    return or_seconds_to_ns((double)bytes * 8 / (double)d->bps);
}

static void transmit_start(or_sim_t* s, int di, int p) {            /* :273-302 */
    netdev_t* d = &s->dev[di];
    d->busy = 1;
    int64_t tx = tx_time(d, s->pk[p].size);
    schedule(s, s->now + tx, EV_COMPLETE, di, -1);                   /* :295 */
    schedule(s, s->now + tx + d->delay, EV_RECEIVE, di, p);           /* :296 (channel) */
    if (++d->wire > s->max_wire && !d->is_access) s->max_wire = d->wire;
}

static void transmit_complete(or_sim_t* s, int di) {                /* :305-336 */
    netdev_t* d = &s->dev[di];
    d->busy = 0;
    if (d->q_len == 0) return;
    int p = q_pop(d);
    d->nbytes -= s->pk[p].size;
    transmit_start(s, di, p);
}

/* DataPacketManager::dropPacket (data-packet-manager.cc:88-98), connected
 * to MacTxDrop of every switch-switch device (:100-106). */
static void mac_tx_drop(or_sim_t* s, int di, int p) {
    if (s->dev[di].is_access) return;
    const pkt_t* k = &s->pk[p];
    for (int w = 0; w < s->N; ++w) {
        if (k->type == DATA_PACKET && k->valable && k->dst != w && k->last_hop == w) {
            VEC_PUSH(&s->lost[w], k->uid);
            /* forwarder.py:214-244: loss transition of the dropping node */
            temp_t* tp = temp_of(s, k->uid);
            if (tp->active) {
                rec_at(s, tp->dec)->status = ST_DROPPED;
                s->cnt.reward_sum += s->c.loss_penalty;
                tp->active = 0;
            }
        }
    }
}

static int dev_send(or_sim_t* s, int di, int p) {                   /* :595-666 */
    netdev_t* d = &s->dev[di];
    pkt_t* k = &s->pk[p];
    int ok;
    if (d->max_bytes > 0) ok = (d->nbytes + k->size <= d->max_bytes);
    else ok = ((uint32_t)d->q_len + 1 <= d->max_pkts);
    if (ok) {
        q_push(d, p);
        d->nbytes += k->size;
        if (!d->is_access && d->q_len + d->wire > s->peak_ring) s->peak_ring = d->q_len + d->wire;
        if (!d->busy) {                                              /* :643-650 */
            int h = q_pop(d);
            d->nbytes -= s->pk[h].size;
            transmit_start(s, di, h);
        }
        return 1;
    }
    if (k->type == DATA_PACKET) {                                    /* :655-664 */
        if (!d->is_access && k->last_hop != d->from_node) s->relay_drops++;
        if (k->valable && k->dst != d->from_node) {
            s->cnt.ov_lost++;
            add_loss_penalty_to_cost(s);
        } else {                      /* e.g. a tunnel crossing the packet's destination */
            s->cnt.un_lost++;
            s->cnt.un_cost_sum += (float)s->c.loss_penalty;      /* addLossPenaltyToUnderlayCost */
            s->cnt.un_cost_n++;
        }
        mac_tx_drop(s, di, p);
    } else {
        s->cnt.ctrl_dropped++;
    }
    pkt_free(s, p);
    return 0;
}

/* ------------------------------------------------------------------ */
/* DataPacketManager::getObservation (data-packet-manager.cc:171-206)  */
/* ------------------------------------------------------------------ */
static uint32_t ping_obs_value(or_sim_t* s, int l) {
    const fvec_t* dv = &s->delays[l];
    double avg = 0.0;                                                /* :55-65 */
    if (dv->n > 0) {
        double sum = 0.0;
        for (int i = 0; i < dv->n; ++i) sum += (double)dv->a[i];
        avg = sum / (double)dv->n;
    }
    float mt = 0.0f;                                                 /* ping-back-packet-manager.cc:110-116 */
    const sentvec_t* uv = &s->unacked[l];
    if (uv->n > 0) {
        double a = get_seconds(s->now) - (double)uv->a[0].ms * 0.001;
        double b = 2.60;
        mt = (float)((b < a) ? b : a);
    }
    double m = ((avg < (double)mt) ? (double)mt : avg);
    return (uint32_t)(1000 * m);
}

static void observation(or_sim_t* s, int v, int dst, uint32_t* obs) {
    for (int i = 0; i < s->W; ++i) obs[i] = 0;
    obs[0] = (uint32_t)s->c.overlay_index[dst];      /* m_map_overlay_array[m_destination] */
    for (int t = s->c.ov_row_ptr[v]; t < s->c.ov_row_ptr[v + 1]; ++t) {
        /* the device RouteOutput picks for 10.2.2.(nbr+1): the tunnel's first link */
        uint32_t val = s->c.ping_as_obs ? ping_obs_value(s, t) : s->dev[s->c.tun_link[t]].nbytes;
        obs[1 + t - s->c.ov_row_ptr[v]] = val;
    }
}

/* ------------------------------------------------------------------ */
/* info string (packet-manager.cc:119-176, data-packet-manager.cc:230-248) */
/* ------------------------------------------------------------------ */
static void build_info(or_sim_t* s, const pkt_t* k, int v) {
    char* b = s->info;
    size_t cap = sizeof(s->info), n = 0;
    double now = get_seconds(s->now);
    float avg_e2e = s->cnt.e2e_n ? s->cnt.e2e_sum / (float)s->cnt.e2e_n : 0.0f;
    float avg_cost = s->cnt.cost_n ? s->cnt.cost_sum / (float)s->cnt.cost_n : 0.0f;
    float sig = s->cnt.bytes_data ? (float)s->cnt.bytes_signaling / (float)s->cnt.bytes_data : 0.0f;
    n += snprintf(b + n, cap - n, "End to End Delay=%f, Packet Size=%u, Current sim time =%f, Pkt ID =%u, packetType =%d",
                  now - (double)k->start_time, k->size, now, k->uid, k->type);
    n += snprintf(b + n, cap - n, ", Avg End to End Delay =%f, Avg Cost =%f, Avg Underlay End to End Delay =%f, Avg Underlay Cost =%f",
                  (double)avg_e2e, (double)avg_cost, 0.0, 0.0);
    n += snprintf(b + n, cap - n, ", Packets dropped =%d, Packets delivered =%d, Packets injected =%d,Packets Buffered =%d",
                  s->cnt.ov_lost, s->cnt.ov_arrived, s->cnt.ov_injected,
                  s->cnt.ov_injected - (s->cnt.ov_arrived + s->cnt.ov_lost));
    n += snprintf(b + n, cap - n, ", Packets dropped Underlay =%d, Packets delivered Underlay=%d, Packets injected Underlay=%d,Packets Buffered Underlay=%d",
                  s->cnt.un_lost, s->cnt.un_arrived, s->cnt.un_injected,
                  s->cnt.un_injected - (s->cnt.un_arrived + s->cnt.un_lost));
    n += snprintf(b + n, cap - n, ",Signaling overhead =%f, Packet Lost=", (double)sig);
    uvec_t* lv = &s->lost[v];
    while (lv->n > 0 && n < cap - 16) {
        n += snprintf(b + n, cap - n, "%u;", lv->a[lv->n - 1]);
        lv->n--;
    }
    snprintf(b + n, cap - n, ", Source=%d, Destination=%d, node=%d", k->src, k->dst, v);
}

/* small-signalling info: PacketManager::getInfo (tokens 0-17) +
 * SmallSignalingPacketManager::getInfo (small-signaling-packet-manager.cc:104-114).
 * Token 3 (the ns-3 packet uid of the echo) is not modelled: it carries the
 * signalled data packet's uid, as token 18 does. */
static void build_ctrl_info(or_sim_t* s, const pkt_t* k, int v) {
    char* b = s->info;
    size_t cap = sizeof(s->info), n = 0;
    double now = get_seconds(s->now);
    float avg_e2e = s->cnt.e2e_n ? s->cnt.e2e_sum / (float)s->cnt.e2e_n : 0.0f;
    float avg_cost = s->cnt.cost_n ? s->cnt.cost_sum / (float)s->cnt.cost_n : 0.0f;
    float sig = s->cnt.bytes_data ? (float)s->cnt.bytes_signaling / (float)s->cnt.bytes_data : 0.0f;
    n += snprintf(b + n, cap - n, "End to End Delay=%f, Packet Size=%u, Current sim time =%f, Pkt ID =%u, packetType =%d",
                  now - (double)k->start_time, k->size, now, k->uid, k->type);
    n += snprintf(b + n, cap - n, ", Avg End to End Delay =%f, Avg Cost =%f, Avg Underlay End to End Delay =%f, Avg Underlay Cost =%f",
                  (double)avg_e2e, (double)avg_cost, 0.0, 0.0);
    n += snprintf(b + n, cap - n, ", Packets dropped =%d, Packets delivered =%d, Packets injected =%d,Packets Buffered =%d",
                  s->cnt.ov_lost, s->cnt.ov_arrived, s->cnt.ov_injected,
                  s->cnt.ov_injected - (s->cnt.ov_arrived + s->cnt.ov_lost));
    n += snprintf(b + n, cap - n, ", Packets dropped Underlay =%d, Packets delivered Underlay=%d, Packets injected Underlay=%d,Packets Buffered Underlay=%d",
                  s->cnt.un_lost, s->cnt.un_arrived, s->cnt.un_injected,
                  s->cnt.un_injected - (s->cnt.un_arrived + s->cnt.un_lost));
    n += snprintf(b + n, cap - n, ",Signaling overhead =%f", (double)sig);
    snprintf(b + n, cap - n, ", PacketIdSignaled=%u, Arrived at final dest=%d", k->uid, (int)(k->dst == v));
}

static void bsig_index(const or_sim_t* s, uint32_t n, uint32_t* nn, uint32_t* seg);

/* big-signalling info: PacketManager::getInfo (tokens 0-17) + BigSignalingPacketManager::getInfo
 * (big-signaling-packet-manager.cc:111-123).  Token 3 (the segment's ns-3 packet uid) is not
 * modelled: 0; the start-time tag is never set, so token 0 is the current time. */
static void build_big_info(or_sim_t* s, const pkt_t* k, int v) {
    char* b = s->info;
    size_t cap = sizeof(s->info), n = 0;
    double now = get_seconds(s->now);
    float avg_e2e = s->cnt.e2e_n ? s->cnt.e2e_sum / (float)s->cnt.e2e_n : 0.0f;
    float avg_cost = s->cnt.cost_n ? s->cnt.cost_sum / (float)s->cnt.cost_n : 0.0f;
    float sig = s->cnt.bytes_data ? (float)s->cnt.bytes_signaling / (float)s->cnt.bytes_data : 0.0f;
    uint32_t nn, seg;
    bsig_index(s, k->ping_idx, &nn, &seg);
    (void)v;
    n += snprintf(b + n, cap - n, "End to End Delay=%f, Packet Size=%u, Current sim time =%f, Pkt ID =%u, packetType =%d",
                  now - (double)k->start_time, k->size, now, k->uid, k->type);
    n += snprintf(b + n, cap - n, ", Avg End to End Delay =%f, Avg Cost =%f, Avg Underlay End to End Delay =%f, Avg Underlay Cost =%f",
                  (double)avg_e2e, (double)avg_cost, 0.0, 0.0);
    n += snprintf(b + n, cap - n, ", Packets dropped =%d, Packets delivered =%d, Packets injected =%d,Packets Buffered =%d",
                  s->cnt.ov_lost, s->cnt.ov_arrived, s->cnt.ov_injected,
                  s->cnt.ov_injected - (s->cnt.ov_arrived + s->cnt.ov_lost));
    n += snprintf(b + n, cap - n, ", Packets dropped Underlay =%d, Packets delivered Underlay=%d, Packets injected Underlay=%d,Packets Buffered Underlay=%d",
                  s->cnt.un_lost, s->cnt.un_arrived, s->cnt.un_injected,
                  s->cnt.un_injected - (s->cnt.un_arrived + s->cnt.un_lost));
    n += snprintf(b + n, cap - n, ",Signaling overhead =%f", (double)sig);
    snprintf(b + n, cap - n, ", NN Index=%u, segment Index=%u, NodeId Signaled=%d", nn, seg,
             s->c.overlay_index[k->src]);
}

/* ------------------------------------------------------------------ */
/* event handlers                                                      */
/* ------------------------------------------------------------------ */
static void send_ping_packets(or_sim_t* s, int u) {                 /* data-packet-manager.cc:350-357 */
    uint32_t idx = s->ping_index[u];
    uint64_t ms = (uint64_t)(s->now / 1000000);                       /* GetMilliSeconds */
    const int t0 = s->c.ov_row_ptr[u], t1 = s->c.ov_row_ptr[u + 1];
    for (int t = t0; t < t1; ++t) {                                    /* addSentPingForwardPacket */
        sent_t e = { idx, ms };
        VEC_PUSH(&s->unacked[t], e);
    }
    for (int t = t0; t < t1; ++t) {                                    /* sendPingForwardPacket :360-413 */
        int p = pkt_alloc(s);
        pkt_t* k = &s->pk[p];
        k->type = PING_FORWARD_PACKET;
        k->dst = k->next_hop = s->c.tun_dst[t];
        k->last_hop = k->src = u;
        k->start_time = ms;
        k->tunnel = t - t0;
        k->ping_idx = idx;
        k->ttl = 64;                                  /* Ipv4Header default */
        k->size = 8 + 8 + 20 + 2;
        dev_send(s, s->c.tun_link[t], p);             /* RouteOutput(10.2.2.(nbr+1)) */
    }
    s->ping_index[u] = idx + 1;
    if (u == s->c.overlay_nodes[0]) s->cnt.ping_rounds++;
    schedule(s, s->now + s->ping_period, EV_PING, u, -1);
}

/* PingForwardPacketManager::receivePacket (ping-forward-packet-manager.cc:94-156) at overlay
 * node v -- the addressee, or any overlay node the ping crosses (NotifyPktRcv hands every
 * PING_FORWARD seen on an overlay node's devices to its manager, packet-routing-gym.cc:254-256):
 * a ping-back to the ping's last hop, on the device it arrived on. */
static void ping_forward_receive(or_sim_t* s, int v, int l_in, int p) {
    const pkt_t* k = &s->pk[p];
    float delay = (float)(get_seconds(s->now) - ((double)k->start_time * 0.001));
    int q = pkt_alloc(s);
    pkt_t* b = &s->pk[q];
    k = &s->pk[p];
    b->type = PING_BACK_PACKET;
    b->dst = b->next_hop = k->last_hop;
    b->last_hop = b->src = v;
    b->one_hop_delay = delay;
    b->ping_idx = k->ping_idx;
    b->tunnel = k->tunnel;
    b->ttl = 64;
    b->size = 8 + 8 + 20 + 2;
    dev_send(s, s->c.link_rev[l_in], q);          /* m_receivingNetDev->Send */
}

/* PingBackPacketManager::receivePacket (ping-back-packet-manager.cc:120-144) at overlay node
 * v, the addressee or a node the ping-back crosses (packet-routing-gym.cc:257-259): the
 * tunnel index is the ORIGIN's, applied to v's own tunnel list.  An index past v's overlay
 * degree is out of range of the reference's vectors (undefined behaviour there): flagged
 * as an error and ignored. */
static void ping_back_receive(or_sim_t* s, int v, int p) {
    const pkt_t* k = &s->pk[p];
    const int deg = s->c.ov_row_ptr[v + 1] - s->c.ov_row_ptr[v];
    if (k->tunnel >= deg) { s->cnt.error |= 32u; s->over = 1; return; }   /* PRISMA_EBIT_PINGIDX */
    int l = s->c.ov_row_ptr[v] + k->tunnel;
    sentvec_t* uv = &s->unacked[l];
    for (int i = 0; i < uv->n; ++i) {
        if (uv->a[i].idx == k->ping_idx) { vec_erase(uv->a, &uv->n, sizeof(sent_t), i); break; }
    }
    fvec_t* dv = &s->delays[l];
    if ((uint32_t)dv->n >= s->c.ma_size) vec_erase(dv->a, &dv->n, sizeof(float), 0);
    VEC_PUSH(dv, k->one_hop_delay);
}

/* Ipv4L3Protocol::IpForward along the global-routing host route to the packet's next hop
 * (its IP destination 10.2.2.(nextHop+1)) through the patched Ipv4Interface::Send
 * (ipv4-interface.cc:213-229).  The TTL is decremented first; at 0 the packet is dropped
 * without any MacTxDrop / counter (the ICMP time-exceeded reply is not modelled). */
static void ip_forward(or_sim_t* s, int v, int p) {
    pkt_t* k = &s->pk[p];
    if (k->type == DATA_PACKET) {
        k->ttl -= 1;
        if (k->ttl == 0) { pkt_free(s, p); return; }
    }
    dev_send(s, s->c.next_link[(size_t)v * s->N + k->next_hop], p);
}

/* DataPacketManager::sendSmallSignalingPacket (data-packet-manager.cc:301-347),
 * called from ExecuteActions before sendPacket when --train (packet-routing-gym.cc:203-206):
 * a 0-B payload (30 B on the wire, signalling type "ideal") back on the device the data
 * packet arrived on, to its last hop; not sent at the packet's source node. */
static void send_small_signaling(or_sim_t* s, const pkt_t* data, int v, int l_in) {
    if (!s->c.train || data->src == v) return;
    int q = pkt_alloc(s);
    pkt_t* e = &s->pk[q];
    e->type = SMALL_SIGN_PACKET;
    e->dst = e->next_hop = data->last_hop;
    e->last_hop = e->src = v;
    e->uid = data->uid;                               /* SetIdValue(m_packetUid) */
    e->start_time = 0;
    e->valable = 0;
    e->ttl = 64;
    e->size = s->echo_payload[v] + 8 + 20 + 2;          /* m_signPacketSize (sim.cc:373-392) */
    dev_send(s, s->c.link_rev[l_in], q);               /* m_receivingNetDev->Send */
}

/* BigSignalingGeneratorApplication (big-signaling-application.cc:224-309): StartSending at
 * AppStartTime schedules the first SendPacket one period later; every SendPacket hands a
 * 512-B segment (tag: type 1, source/nextHop/destination, lastHop 1000, segment and NN index)
 * to the UDP socket of the traffic node -- its access link -- and schedules the next. */
static void bsig_send_packet(or_sim_t* s, int g) {
    uint32_t n = (uint32_t)++s->g_draws[g];                         /* ScheduleNextTx counted it */
    int p = pkt_alloc(s);
    pkt_t* k = &s->pk[p];
    k->type = BIG_SIGN_PACKET;
    k->src = s->g_src[g];
    k->dst = k->next_hop = s->g_dst[g];
    k->last_hop = 1000;
    k->start_time = 0;
    k->valable = 0;
    k->uid = 0;                                                       /* ns-3 packet uid: not modelled */
    k->ping_idx = n;
    k->ttl = 255;                                                     /* SetIpTtl(255) :282 */
    k->size = 512 + 8 + 20 + 2;
    dev_send(s, s->E + s->g_src[g], p);
    schedule(s, s->now + s->bs_period, EV_BSEND, g, -1);
}
/* segment / NN index of the n-th segment (ScheduleNextTx :241-246: the index is bumped
 * before each send and wraps to 0 -- next NN copy -- at m_pktSizeMean / m_segSize) */
static void bsig_index(const or_sim_t* s, uint32_t n, uint32_t* nn, uint32_t* seg) {
    if (s->bs_nseg <= 1) { *nn = n; *seg = 0; return; }
    *nn = n / s->bs_nseg; *seg = n % s->bs_nseg;
}

/* rng_mode 1: simSeed of this replica (sim.cc:253-254 set it as seed and run) */
static uint32_t ns3_sim_seed(const or_sim_t* s) { return (uint32_t)(s->c.seed + s->c.replica); }

static void flow_schedule_next(or_sim_t* s, int f) {                /* poisson-application.cc:265-295 */
    double U;
    if (s->c.rng_mode == 1) {
        /* a new ExponentialRandomVariable per packet (:281-284): its stream's first value */
        const uint32_t sd = ns3_sim_seed(s);
        U = or_mrg_first_u01(sd, s->rv_next++, sd);
    } else {
        uint32_t key[2] = { (uint32_t)s->c.seed, s->c.replica };
        uint32_t ctr[4] = { (uint32_t)f, (uint32_t)s->flow_draws[f], s->c.episode, 1u };
        uint32_t x[4];
        or_philox4x32_10(ctr, key, x);
        uint64_t u53 = ((uint64_t)(x[0] >> 5) << 26) | (uint64_t)(x[1] >> 6);
        U = ((double)u53 + 1.0) * (1.0 / 9007199254740992.0);
    }
    double delay = -s->flow_mean[f] * or_det_log(U);
    s->flow_draws[f]++;
    schedule(s, s->now + or_seconds_to_ns(delay), EV_SEND, f, -1);
}

static void flow_send_packet(or_sim_t* s, int f) {                  /* poisson-application.cc:297-358 */
    int p = pkt_alloc(s);
    pkt_t* k = &s->pk[p];
    k->type = DATA_PACKET;
    k->dst = s->c.flow_dst[f];
    k->src = k->next_hop = s->c.flow_src[f];
    k->last_hop = 1000;
    k->start_time = (uint64_t)get_seconds(s->now);                    /* :310 */
    k->valable = 1;                                                   /* overlay pair: p = 1.0 */
    if (s->c.rng_mode == 1) s->rv_next++;       /* the UniformRandomVariable of :311-314 (its value: the tag above) */
    k->uid = s->next_uid++;
    k->ttl = 255;                                                     /* SetIpTtl(255) :330 */
    k->size = s->c.packet_size + 8 + 20 + 2;
    dev_send(s, s->E + s->c.flow_src[f], p);                          /* UDP socket -> access link */
    flow_schedule_next(s, f);
}

/* Receive tail after the MacRx trace (point-to-point-net-device.cc:430-463) */
static void receive_counters(or_sim_t* s, const pkt_t* k, int v) {
    if (k->type == DATA_PACKET && k->dst == v) {
        if (k->valable) {
            if (k->next_hop == k->dst) {
                s->cnt.ov_arrived++;
                float x = (float)(get_seconds(s->now) - (double)k->start_time);
                s->cnt.cost_sum += x; s->cnt.cost_n++;
                s->cnt.e2e_sum += x; s->cnt.e2e_n++;
            }
        } else {
            s->cnt.un_arrived++;
        }
    }
    if (k->type > 0 && k->dst == v) s->cnt.bytes_signaling += (int32_t)(k->size - 2);
    if (k->type == DATA_PACKET && k->last_hop == 1000) {
        if (k->valable) { s->cnt.ov_injected++; s->cnt.bytes_data += (int32_t)(k->size - 2); }
        else s->cnt.un_injected++;
    }
}

/* DataPacketManager::sendPacket (data-packet-manager.cc:251-299) */
static void finish_data_decision(or_sim_t* s, int action) {
    int p = s->pend_pkt, v = s->pend_node;
    int64_t d = s->pend_rec;
    if (s->pend_ctrl) {                 /* control notification: ExecuteActions sends nothing */
        receive_counters(s, &s->pk[p], v);
        pkt_free(s, p);
        s->pend = 0;
        s->pend_ctrl = 0;
        return;
    }
    if (s->pend_dest) {                 /* done=True notification: sendPacket does nothing (:256-260) */
        pkt_t orig = s->pk[p];
        send_small_signaling(s, &orig, v, s->pend_link);
        receive_counters(s, &orig, v);
        pkt_free(s, p);
        s->pend = 0;
        s->pend_dest = 0;
        return;
    }
    pkt_t orig = s->pk[p];
    send_small_signaling(s, &orig, v, s->pend_link);
    const int t0 = s->c.ov_row_ptr[v], deg = s->c.ov_row_ptr[v + 1] - t0;
    rec_head_t* r = rec_at(s, d);
    r->action = (int8_t)action;
    if (action >= 0 && action < deg) {
        const int t = t0 + action;
        int q = pkt_alloc(s);
        pkt_t* k = &s->pk[q];
        *k = s->pk[p];
        k->next_free = -2;
        k->last_hop = v;
        k->next_hop = s->c.tun_dst[t];
        k->size = s->c.packet_size + 8 + 20 + 2;
        temp_t* tp = temp_of(s, k->uid);
        tp->dec = d; tp->t_ns = s->now; tp->active = 1;
        rec_at(s, d)->status = ST_ENQUEUED;
        s->cnt.hops++;
        s->cnt.hop_deg_sum += (uint64_t)deg;
        dev_send(s, s->c.tun_link[t], q);   /* RouteOutput device; a drop re-marks the record DROPPED */
    } else {
        rec_at(s, d)->status = ST_DISCARDED;
    }
    receive_counters(s, &orig, v);
    pkt_free(s, p);
    s->pend = 0;
}

/* The engine's decision log is a ring of log_capacity records, and a forwarded packet's uid,
 * destination, start second and reward clock are read back from its previous decision's record
 * (include/prisma.h PRISMA_EBIT_LOGWRAP).  Not part of the reference: the engine's defined
 * failure, restated so that both sides stop at the same event.  A packet whose previous
 * decision is log_capacity or more decisions old ends the episode with error bit 16; the
 * event consumes the packet and does nothing else (no record, no forward, no counters). */
static int log_wrapped(or_sim_t* s, const pkt_t* k) {
    if (s->c.log_capacity == 0u) return 0;
    const temp_t* tp = temp_of(s, k->uid);
    if (!tp->active || s->rec_n - tp->dec < (int64_t)s->c.log_capacity) return 0;
    s->cnt.error |= 16u;                                              /* PRISMA_EBIT_LOGWRAP */
    s->over = 1;
    return 1;
}

/* PointToPointNetDevice::Receive -> PacketRoutingEnv::NotifyPktRcv
 * (point-to-point-net-device.cc:371-467, packet-routing-gym.cc:231-267).
 * Order at the receiving switch v: MacRx trace (the overlay node's managers),
 * then the IP stack (forwarding when v is not the packet's next hop), then
 * the Receive counters.  Returns 1 when a data decision needs an action. */
static int receive(or_sim_t* s, int di, int p) {
    const netdev_t* d = &s->dev[di];
    int v = d->to_node;
    pkt_t* k = &s->pk[p];
    const int overlay = s->c.overlay_index[v] >= 0;
    if (k->type == DATA_PACKET) {
        /* a forwarded packet arriving at its next overlay node or at a switch inside its tunnel */
        if (k->last_hop != 1000 && log_wrapped(s, k)) { pkt_free(s, p); return 0; }
        if (!(k->next_hop == v && k->valable)) {                      /* packet-manager.cc:115 */
            pkt_t orig = *k;
            if (k->next_hop != v) ip_forward(s, v, p);                /* inside a tunnel */
            else pkt_free(s, p);
            receive_counters(s, &orig, v);
            return 0;
        }
        int64_t dn = rec_new(s);
        rec_head_t* r = rec_at(s, dn);
        temp_t* tp = temp_of(s, k->uid);
        r->t_ns = s->now;
        r->uid = k->uid;
        r->node = (uint8_t)v;
        r->dst = (uint8_t)k->dst;
        r->start_s = (uint16_t)k->start_time;
        r->ttl = (uint8_t)k->ttl;
        r->episode = (uint8_t)s->c.episode;
        r->action = -1;
        if (tp->active) {                                             /* handle_transit_packet */
            r->prev = (int32_t)tp->dec;
            r->reward = py_reward(s->now, tp->t_ns);                  /* forwarder.py:360 */
            s->cnt.reward_sum += r->reward;
            tp->active = 0;
        } else {
            r->prev = -1;
            r->reward = 0.0;
        }
        observation(s, v, k->dst, (uint32_t*)((unsigned char*)r + sizeof(rec_head_t)));
        build_info(s, k, v);
        s->cnt.decisions++;
        if (k->dst == v) {                                            /* getGameOver: done */
            r->status = ST_DEST;
            if (s->c.notify_dest) {                                   /* the agent sees it (done=True) */
                s->pend = 1; s->pend_dest = 1; s->pend_pkt = p; s->pend_node = v; s->pend_link = di; s->pend_rec = dn;
                return 1;
            }
            pkt_t orig = *k;
            send_small_signaling(s, &orig, v, di);
            receive_counters(s, &orig, v);                            /* sendPacket does nothing */
            pkt_free(s, p);
            return 0;
        }
        r->status = ST_PENDING;
        s->pend = 1; s->pend_pkt = p; s->pend_node = v; s->pend_link = di; s->pend_rec = dn;
        return 1;
    }
    if (k->type == BIG_SIGN_PACKET) {
        /* BigSignalingPacketManager::receivePacket (big-signaling-packet-manager.cc:93-108):
         * not at the packet's source; valid (nextHop == node, at its final destination) -> Notify */
        if (overlay && k->src != v && k->next_hop == v && k->dst == v) {
            build_big_info(s, k, v);
            if (s->c.notify_dest) {
                s->pend = 1; s->pend_ctrl = 1; s->pend_pkt = p; s->pend_node = v; s->pend_link = di;
                return 1;
            }
        }
    } else if (k->type == SMALL_SIGN_PACKET) {
        /* SmallSignalingPacketManager::receivePacket (small-signaling-packet-manager.cc:86-94):
         * valid (nextHop == node and arrived at its final destination) -> Notify */
        if (k->next_hop == v && k->dst == v) {
            build_ctrl_info(s, k, v);
            if (s->c.notify_dest) {
                s->pend = 1; s->pend_ctrl = 1; s->pend_pkt = p; s->pend_node = v; s->pend_link = di;
                return 1;
            }
        }
    } else if (overlay && k->type == PING_FORWARD_PACKET) {
        ping_forward_receive(s, v, di, p);
    } else if (overlay && k->type == PING_BACK_PACKET) {
        ping_back_receive(s, v, p);
    }
    pkt_t orig = s->pk[p];
    if (k->next_hop != v) ip_forward(s, v, p);                        /* inside a tunnel */
    else pkt_free(s, p);
    receive_counters(s, &orig, v);
    return 0;
}

/* run events until a decision is pending (1) or the episode is over (0) */
static int run_until_decision(or_sim_t* s) {
    while (!s->over) {
        if (s->hn == 0 || s->heap[0].t >= s->t_end) { s->over = 1; break; }
        ev_t e = heap_pop(s);
        s->now = e.t;
        s->cnt.events++;
        if (s->trace_on) {
            if (s->tr_n + 4 > s->tr_cap) { s->tr_cap = s->tr_cap ? 2 * s->tr_cap : 4096; s->tr = xrealloc(s->tr, sizeof(int64_t) * s->tr_cap); }
            s->tr[s->tr_n++] = e.t; s->tr[s->tr_n++] = (int64_t)e.seq; s->tr[s->tr_n++] = e.kind; s->tr[s->tr_n++] = e.id;
        }
        switch (e.kind) {
        case EV_PING: send_ping_packets(s, e.id); break;
        case EV_START: flow_schedule_next(s, e.id); break;             /* StartSending -> ScheduleNextTx */
        case EV_SEND: flow_send_packet(s, e.id); break;
        case EV_BSTART: schedule(s, s->now + s->bs_period, EV_BSEND, e.id, -1); break;   /* StartSending */
        case EV_BSEND: bsig_send_packet(s, e.id); break;
        case EV_COMPLETE: transmit_complete(s, e.id); break;
        case EV_RECEIVE:
            s->dev[e.id].wire--;
            if (receive(s, e.id, e.pkt)) return 1;
            break;
        }
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* public API                                                          */
/* ------------------------------------------------------------------ */
or_sim_t* or_create(const or_config_t* cfg) {
    or_sim_t* s = calloc(1, sizeof(or_sim_t));
    s->c = *cfg;
    s->N = cfg->n_nodes; s->E = cfg->n_links; s->F = cfg->n_flows;
    s->W = (1 + cfg->max_deg + 3) & ~3;                 /* multiple of 4 (16-B rows) */
    s->rec_bytes = (int)sizeof(rec_head_t) + 4 * s->W;
    s->t_end = or_seconds_to_ns(cfg->sim_time_s);
    s->ping_period = or_seconds_to_ns((double)cfg->ping_interval_s);
    s->pk_free = -1;
    s->dev = calloc((size_t)(s->E + s->N), sizeof(netdev_t));
    for (int l = 0; l < s->E; ++l) {                                  /* sim.cc:414-433 */
        netdev_t* d = &s->dev[l];
        d->bps = cfg->link_bps; d->delay = cfg->link_delay_ns; d->max_bytes = cfg->max_buffer_bytes;
        d->to_node = cfg->link_dst[l]; d->is_access = 0;
    }
    for (int u = 0; u < s->N; ++u)
        for (int l = cfg->row_ptr[u]; l < cfg->row_ptr[u + 1]; ++l) s->dev[l].from_node = u;
    for (int u = 0; u < s->N; ++u) {                                  /* sim.cc:398-410 */
        netdev_t* d = &s->dev[s->E + u];
        int deg = cfg->row_ptr[u + 1] - cfg->row_ptr[u];
        d->bps = (uint64_t)1000000 * cfg->link_bps * (uint64_t)deg;
        d->delay = 0; d->max_bytes = 0; d->max_pkts = 1000;
        d->from_node = -1; d->to_node = u; d->is_access = 1;
    }
    s->flow_draws = calloc((size_t)s->F + 1, sizeof(int));
    s->flow_mean = calloc((size_t)s->F + 1, sizeof(double));
    for (int f = 0; f < s->F; ++f)
        s->flow_mean[f] = (double)(cfg->packet_size * 8u) / (double)cfg->flow_rate_bps[f];
    s->ping_index = calloc((size_t)s->N, sizeof(uint32_t));
    s->unacked = calloc((size_t)cfg->n_tunnels + 1, sizeof(sentvec_t));
    s->delays = calloc((size_t)cfg->n_tunnels + 1, sizeof(fvec_t));
    s->lost = calloc((size_t)s->N, sizeof(uvec_t));
    s->cnt.episode = cfg->episode;
    /* signalling (sim.cc:373-392): echo payload by the overlay degree of its sender */
    s->echo_payload = calloc((size_t)s->N, sizeof(uint32_t));
    for (int u = 0; u < s->N; ++u) {
        uint32_t odeg = (uint32_t)(cfg->ov_row_ptr[u + 1] - cfg->ov_row_ptr[u]);
        s->echo_payload[u] = cfg->signaling_type == 1 ? 8u + 8u * (odeg + 1u) : (cfg->signaling_type == 2 ? 24u : 0u);
    }
    /* big signalling (sim.cc:634-647): inside the flow loop, one generator per flow between
     * overlay neighbours; ScheduleNextTx's period in the reference's own arithmetic: the
     * uint32 size * 8 over the float syncStep is a float, 4096 over that a double */
    s->g_src = calloc((size_t)s->F + 1, sizeof(int));
    s->g_dst = calloc((size_t)s->F + 1, sizeof(int));
    s->g_draws = calloc((size_t)s->F + 1, sizeof(int));
    int* g_of_flow = calloc((size_t)s->F + 1, sizeof(int));
    const int bsig = cfg->train && cfg->big_signaling && cfg->signaling_type == 1;
    for (int f = 0; f < s->F; ++f) {
        g_of_flow[f] = -1;
        if (!bsig) continue;
        const int u = cfg->flow_src[f], w = cfg->flow_dst[f];
        for (int t = cfg->ov_row_ptr[u]; t < cfg->ov_row_ptr[u + 1]; ++t)
            if (cfg->tun_dst[t] == w) { g_of_flow[f] = s->G; s->g_src[s->G] = u; s->g_dst[s->G] = w; s->G++; break; }
    }
    {
        const float rate = (float)(cfg->big_signaling_bytes * 8u) / cfg->sync_step_s;
        const double delay = (double)(512u * 8u) / (double)rate;
        s->bs_period = or_seconds_to_ns(delay);
        s->bs_nseg = cfg->big_signaling_bytes / 512u;
    }
    /* setup-time schedule: ping timers (sim.cc:544 -> data-packet-manager.cc:118-121)
       in overlay order, then application starts (Node::Initialize at t=0) in
       flow (src, dst) order (sim.cc:599-631) */
    for (int i = 0; i < cfg->n_overlay; ++i) schedule(s, s->ping_period, EV_PING, cfg->overlay_nodes[i], -1);
    uint32_t key[2] = { (uint32_t)cfg->seed, cfg->replica };
    s->rv_next = cfg->rng_stream_offset;
    for (int f = 0; f < s->F; ++f) {
        double U;
        if (cfg->rng_mode == 1) {
            /* the UniformRandomVariable of flow f's start offset, created in the flow loop */
            const uint32_t sd = ns3_sim_seed(s);
            U = or_mrg_first_u01(sd, s->rv_next++, sd);
        } else {
            uint32_t ctr[4] = { (uint32_t)f, 0u, cfg->episode, 0u };
            uint32_t x[4];
            or_philox4x32_10(ctr, key, x);
            uint64_t u53 = ((uint64_t)(x[0] >> 5) << 26) | (uint64_t)(x[1] >> 6);
            U = (double)u53 * (1.0 / 9007199254740992.0);
        }
        schedule(s, or_seconds_to_ns(0.0001 + U), EV_START, f, -1);
        if (g_of_flow[f] >= 0) schedule(s, or_seconds_to_ns(0.0001), EV_BSTART, g_of_flow[f], -1);   /* AppStartTime */
    }
    free(g_of_flow);
    return s;
}

void or_destroy(or_sim_t* s) {
    if (!s) return;
    for (int i = 0; i < s->E + s->N; ++i) free(s->dev[i].q);
    for (int t = 0; t < s->c.n_tunnels; ++t) { free(s->unacked[t].a); free(s->delays[t].a); }
    for (int u = 0; u < s->N; ++u) free(s->lost[u].a);
    free(s->dev); free(s->flow_draws); free(s->flow_mean); free(s->ping_index);
    free(s->unacked); free(s->delays); free(s->lost); free(s->temp);
    free(s->echo_payload); free(s->g_src); free(s->g_dst); free(s->g_draws);
    free(s->heap); free(s->pk); free(s->rec); free(s->tr);
    free(s);
}

int or_step(or_sim_t* s, int32_t action, int32_t* obs_out) {
    if (s->pend) finish_data_decision(s, action);
    int r = run_until_decision(s);
    if (r && obs_out && s->pend_ctrl) {             /* GetObservation for a control packet: [1000] */
        const pkt_t* k = &s->pk[s->pend_pkt];
        for (int i = 0; i < s->W; ++i) obs_out[i] = 0;
        obs_out[0] = 1000;                          /* + the info fields (engine ABI: include/prisma.h) */
        if (k->type == BIG_SIGN_PACKET) {
            uint32_t nn, seg;
            bsig_index(s, k->ping_idx, &nn, &seg);
            obs_out[1] = (int32_t)nn;
            obs_out[2] = (int32_t)seg;
            obs_out[3] = 0x10000 | s->c.overlay_index[k->src];
        } else {
            obs_out[1] = (int32_t)k->uid;           /* the signalled uid */
            obs_out[2] = (int32_t)k->size;
        }
        return r;
    }
    if (r && obs_out) {
        const uint32_t* o = (const uint32_t*)((unsigned char*)rec_at(s, s->pend_rec) + sizeof(rec_head_t));
        for (int i = 0; i < s->W; ++i) obs_out[i] = (int32_t)o[i];
    }
    return r;
}

int64_t or_run_table(or_sim_t* s, const uint8_t* table, int64_t max_hops) {
    uint64_t h0 = s->cnt.hops;
    while ((int64_t)(s->cnt.hops - h0) < max_hops) {
        if (s->pend) {
            rec_head_t* r = rec_at(s, s->pend_rec);
            finish_data_decision(s, table[(size_t)r->node * s->N + r->dst]);
            continue;
        }
        if (!run_until_decision(s)) break;
    }
    return (int64_t)(s->cnt.hops - h0);
}

/* ------------------------------------------------------------------ */
/* DQN_buffer_model (models.py:258-306) restated in fp32 with a fixed    */
/* operation order: the checker for the in-kernel MLP.    */
/* ------------------------------------------------------------------ */
double or_det_expm1(double x) {                 /* x <= 0; + - * / only */
    if (x < -60.0) return -1.0;
    double t = x * 1.4426950408889634 + 0.5;
    int64_t ki = (int64_t)t;
    if ((double)ki > t) ki -= 1;
    double k = (double)ki;
    double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    static const double inv_fact[14] = { 1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
                                         1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0,
                                         1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 0.0 };
    double p = r * (1.0 / 87178291200.0);
    for (int i = 0; i < 13; ++i) p = (p + inv_fact[i]) * r;
    if (ki == 0) return p;
    uint64_t bits = (uint64_t)(1023 + ki) << 52;
    double scale;
    memcpy(&scale, &bits, 8);
    return scale * (p + 1.0) - 1.0;
}

/* fp32 expm1 for x <= 0, + - * and an int conversion only: the engine's det_expm1f
 * (prisma_amd/csrc/numerics.h), the same operations in the same order. */
float or_det_expm1f(float x) {
    if (!(x == x)) return x;
    if (x < -17.0f) return -1.0f;
    if (x > -5.9604645e-08f) return x;
    const float t = x * 1.44269504f + 0.5f;
    int ki = (int)t;
    if ((float)ki > t) ki -= 1;
    const float k = (float)ki;
    const float r = (x - k * 0.693145751953125f) - k * 1.42860677e-06f;
    static const float c[6] = { 1.38888889e-03f, 8.33333333e-03f, 4.16666667e-02f, 1.66666667e-01f, 0.5f, 1.0f };
    float p = r * 1.98412698e-04f;
    for (int i = 0; i < 6; ++i) p = (p + c[i]) * r;
    if (ki == 0) return p;
    uint32_t bits = (uint32_t)(127 + ki) << 23;
    float scale;
    memcpy(&scale, &bits, 4);
    return scale * (p + 1.0f) - 1.0f;
}

static float elu_f(float x) { return x > 0.0f ? x : or_det_expm1f(x); }

/* Packed weights (float): W1[N][N][32] b1[N][32] Wb[N][D][32] bb[N][32] W2[N][64][64] b2[N][64]
 * W3[N][64][64] b3[N][64] W4[N][64][D] b4[N][D], D = max_deg (prisma_amd.policies.StackedQNet.pack). */
static int mlp_action(const or_sim_t* s, const float* w, int v, const uint32_t* obs, float* q_out) {
    const int N = s->N, D = s->c.max_deg;
    const float* W1 = w;
    const float* b1 = W1 + (size_t)N * N * 32;
    const float* Wb = b1 + (size_t)N * 32;
    const float* bb = Wb + (size_t)N * D * 32;
    const float* W2 = bb + (size_t)N * 32;
    const float* b2 = W2 + (size_t)N * 64 * 64;
    const float* W3 = b2 + (size_t)N * 64;
    const float* b3 = W3 + (size_t)N * 64 * 64;
    const float* W4 = b3 + (size_t)N * 64;
    const float* b4 = W4 + (size_t)N * 64 * D;
    int deg = s->c.ov_row_ptr[v + 1] - s->c.ov_row_ptr[v];
    int dst = (int)obs[0];                                   /* overlay index (one-hot input) */
    float x[128], xn[128], h[64], h2[64];
    float sum = 0.0f, var = 0.0f;
    for (int k = 0; k < deg; ++k) { x[k] = (float)obs[1 + k]; sum = sum + x[k]; }
    float mean = sum / (float)deg;
    for (int k = 0; k < deg; ++k) { float d = x[k] - mean; var = var + d * d; }
    var = var / (float)deg;
    float den = sqrtf(var + 1e-3f);                         /* LayerNormalization, epsilon 1e-3 */
    for (int k = 0; k < deg; ++k) xn[k] = (x[k] - mean) / den;
    for (int j = 0; j < 32; ++j) h[j] = elu_f(W1[((size_t)v * N + dst) * 32 + j] + b1[v * 32 + j]);
    for (int j = 0; j < 32; ++j) {
        float acc = 0.0f;
        for (int k = 0; k < deg; ++k) acc = fmaf(xn[k], Wb[((size_t)v * D + k) * 32 + j], acc);
        h[32 + j] = elu_f(acc + bb[v * 32 + j]);
    }
    for (int j = 0; j < 64; ++j) {
        float acc = 0.0f;
        for (int i = 0; i < 64; ++i) acc = fmaf(h[i], W2[((size_t)v * 64 + i) * 64 + j], acc);
        h2[j] = elu_f(acc + b2[v * 64 + j]);
    }
    for (int j = 0; j < 64; ++j) {
        float acc = 0.0f;
        for (int i = 0; i < 64; ++i) acc = fmaf(h2[i], W3[((size_t)v * 64 + i) * 64 + j], acc);
        h[j] = elu_f(acc + b3[v * 64 + j]);
    }
    int best = 0;
    float bq = 0.0f;
    for (int a = 0; a < deg; ++a) {
        float acc = 0.0f;
        for (int i = 0; i < 64; ++i) acc = fmaf(h[i], W4[((size_t)v * 64 + i) * D + a], acc);
        float q = elu_f(acc + b4[v * D + a]);
        if (q_out) q_out[a] = q;
        if (a == 0 || q < bq) { bq = q; best = a; }          /* tf.argmin: first minimum */
    }
    return best;
}

int64_t or_run_mlp(or_sim_t* s, const float* weights, int64_t max_hops) {
    uint64_t h0 = s->cnt.hops;
    while ((int64_t)(s->cnt.hops - h0) < max_hops) {
        if (s->pend) {
            rec_head_t* r = rec_at(s, s->pend_rec);
            const uint32_t* o = (const uint32_t*)((unsigned char*)r + sizeof(rec_head_t));
            finish_data_decision(s, mlp_action(s, weights, r->node, o, NULL));
            continue;
        }
        if (!run_until_decision(s)) break;
    }
    return (int64_t)(s->cnt.hops - h0);
}

int32_t or_mlp_action(or_sim_t* s, const float* weights, int32_t v, const uint32_t* obs) {
    return mlp_action(s, weights, v, obs, NULL);
}

/* The fixed-order fp32 Q values of the same decision (q_out[0..deg-1]); returns the action. */
int32_t or_mlp_q(or_sim_t* s, const float* weights, int32_t v, const uint32_t* obs, float* q_out) {
    return mlp_action(s, weights, v, obs, q_out);
}

/* n decisions at once: nodes[n], obs[n][obs_stride], q_out[n][q_stride] (unused slots
 * untouched), actions[n]. */
void or_mlp_q_batch(or_sim_t* s, const float* weights, int64_t n, const int32_t* nodes, const uint32_t* obs,
                    int32_t obs_stride, float* q_out, int32_t q_stride, int32_t* actions) {
    for (int64_t i = 0; i < n; ++i)
        actions[i] = mlp_action(s, weights, nodes[i], obs + i * obs_stride, q_out + i * q_stride);
}

int64_t or_record_count(const or_sim_t* s) { return s->rec_n; }
int32_t or_pending_node(const or_sim_t* s) { return s->pend ? s->pend_node : -1; }
int32_t or_obs_width(const or_sim_t* s) { return s->W; }

int64_t or_copy_records(const or_sim_t* s, int64_t first, int64_t count, void* out) {
    if (first < 0 || first > s->rec_n) return 0;
    if (first + count > s->rec_n) count = s->rec_n - first;
    memcpy(out, s->rec + (size_t)first * s->rec_bytes, (size_t)count * s->rec_bytes);
    return count;
}

void or_counters(const or_sim_t* s, void* out) {
    counters_t c = s->cnt;
    c.now_ns = s->now;
    c.seq = (uint32_t)s->seq;
    c.uid = s->next_uid;
    c.dec_count = (uint32_t)s->rec_n;
    c.episode_over = (uint32_t)s->over;
    c.hops_total = c.hops;
    c.events_total = c.events;
    memcpy(out, &c, sizeof(c));
}

void or_diag(const or_sim_t* s, int64_t out[6]) {
    int64_t mx = 0, tot = 0, deep = 0;
    for (int i = 0; i < s->E; ++i) {               /* switch devices: the FIFOs a test probes */
        const int n = s->dev[i].q_len;
        if (n > mx) mx = n;
        tot += n;
        if (n > 4) deep++;
    }
    out[0] = s->relay_drops;
    out[1] = mx;
    out[2] = tot;
    out[3] = deep;
    out[4] = s->max_wire;
    out[5] = s->peak_ring;
}

void or_enable_trace(or_sim_t* s, int on) { s->trace_on = on; }
int64_t or_trace_count(const or_sim_t* s) { return s->tr_n / 4; }
int64_t or_copy_trace(const or_sim_t* s, int64_t first, int64_t count, int64_t* out4) {
    int64_t n = s->tr_n / 4;
    if (first < 0 || first > n) return 0;
    if (first + count > n) count = n - first;
    memcpy(out4, s->tr + first * 4, (size_t)count * 4 * sizeof(int64_t));
    return count;
}

int32_t or_last_info(const or_sim_t* s, char* buf, int32_t cap) {
    int32_t n = (int32_t)strlen(s->info);
    if (cap <= 0) return n;
    int32_t m = n < cap - 1 ? n : cap - 1;
    memcpy(buf, s->info, (size_t)m);
    buf[m] = 0;
    return m;
}
