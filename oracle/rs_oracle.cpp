/*
 * rs_oracle.cpp -- CPU ORACLE (test infrastructure, see rs_oracle.h).
 *
 * A from-scratch restatement of the reference's per-TTI downlink RBG allocation for the
 * backlogged (InfiniteBuffer, one bearer per UE) case, flat arrays instead of the reference's
 * object graph.  Arithmetic order, integer/double promotions and tie rules follow the cited
 * reference lines; libm (pow/exp/log/log10) and libstdc++ std::sort are called directly, as the
 * reference does.  Build: g++ -O2 -ffp-contract=off (no -ffast-math, no -march).
 *
 * `ref:` = /root/reference/src/
 */
#include "rs_oracle.h"

#include <omp.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../radiosaber_amd/csrc/rs_amc_tables.inc" /* numeric data shared with the product */

namespace {

const int kCqiToMcs[15] = {RS_AMC_CQI_TO_MCS};
const double kSinrForCqi[15] = {RS_AMC_SINR_FOR_CQI};
const int kMcsToItbs[29] = {RS_AMC_MCS_TO_ITBS};
const int kTbs[110][27] = {RS_AMC_TBS_TABLE};

}  // namespace

extern "C" {

const int* rso_tbs_table(void) { return &kTbs[0][0]; }
const int* rso_mcs_to_itbs(void) { return kMcsToItbs; }
const int* rso_cqi_to_mcs(void) { return kCqiToMcs; }
const double* rso_sinr_for_cqi(void) { return kSinrForCqi; }

/* ref: protocolStack/mac/AMCModule.cpp:320-327 (+ :271-274, :299-303)
 * eff = (TBS(1 PRB, mcs(cqi)) / 0.001) / 180000. */
double rso_efficiency_from_cqi(int cqi) {
  int mcs = kCqiToMcs[cqi - 1];
  int bits = kTbs[0][kMcsToItbs[mcs]];
  double eff = (bits / 0.001) / 180000.;
  return eff;
}

/* ref: AMCModule.cpp:253-261 -- count thresholds <= sinr, starting at CQI 1 */
int rso_cqi_from_sinr(double sinr) {
  int cqi = 1;
  while (cqi <= 14 && kSinrForCqi[cqi] <= sinr) cqi++;
  return cqi;
}

/* ref: AMCModule.cpp:306-317.  For nbRBs > 110 the reference computes
 * 5*T[nbRBs/5-1][itbs] + T[nbRBs%5-1][itbs]; when nbRBs%5 == 0 that reads T[-1][itbs], an
 * out-of-bounds read.  In the as-shipped -O0 build McsToItbs[29] lies 128 bytes in front of the
 * table, so T[-1][i] == McsToItbs[5+i] for i <= 23 and 0 (padding) for i = 24..26
 * ("reference UB, pinned to the as-shipped build"). */
static int tbs_row_m1(int itbs) { return itbs <= 23 ? kMcsToItbs[5 + itbs] : 0; }

int rso_tbs_bits(int mcs, int nb_rbs) {
  int itbs = kMcsToItbs[mcs];
  if (nb_rbs <= 110) return kTbs[nb_rbs - 1][itbs];
  int sub = nb_rbs / 5, rest = nb_rbs % 5;
  int tail = rest == 0 ? tbs_row_m1(itbs) : kTbs[rest - 1][itbs];
  return 5 * kTbs[sub - 1][itbs] + tail;
}

/* ref: utility/eesm-effective-sinr.h:33-46 (beta = 1) */
double rso_eesm_effective_sinr(const double* sinr, int n) {
  double sum_i = 0;
  double beta = 1;
  for (int i = 0; i < n; i++) {
    double s = pow(10, sinr[i] / 10);
    sum_i += exp(-s / beta);
  }
  double eff = -beta * log(sum_i / (size_t)n);
  eff = 10 * log10(eff);
  return eff;
}

/* ref: eesm-effective-sinr.h:82-103 */
int rso_rbg_size(int nof_prb) {
  if (nof_prb <= 10) return 1;
  if (nof_prb <= 26) return 2;
  if (nof_prb <= 63) return 3;
  if (nof_prb <= 110) return 4;
  if (nof_prb <= 512) return 8;
  return -1; /* reference throws std::runtime_error */
}

/* ref: downlink-transport-scheduler.cpp:638-650: SINR of each allocated PRB's CQI -> EESM -> CQI */
int rso_final_cqi(const uint8_t* cqi_per_prb, int n) {
  std::vector<double> s(n);
  for (int i = 0; i < n; i++) s[i] = kSinrForCqi[cqi_per_prb[i] - 1];
  return rso_cqi_from_sinr(rso_eesm_effective_sinr(s.data(), n));
}

/* ---- glibc TYPE_3 additive feedback generator (glibc 2.35 stdlib/random_r.c: __srandom_r,
 *      __random_r with rand_type 3, degree 31, separation 3).  Not in the reference tree: the
 *      reference calls libc rand()/srand() (downlink-transport-scheduler.cpp:490,511;
 *      single-cell-with-interference.h:84-89).  Pinned by tests against this image's libc. ---- */
void rso_srand(rso_rng* g, unsigned seed) {
  int32_t* r = g->r;
  if (seed == 0) seed = 1;
  r[0] = (int32_t)seed;
  for (int i = 1; i < 31; i++) {
    long hi = r[i - 1] / 127773;
    long lo = r[i - 1] % 127773;
    long word = 16807 * lo - 2836 * hi;
    if (word < 0) word += 2147483647;
    r[i] = (int32_t)word;
  }
  g->f = 3;
  g->b = 0;
  for (int i = 0; i < 310; i++) (void)rso_rand(g);
}

int rso_rand(rso_rng* g) {
  uint32_t* r = (uint32_t*)g->r;
  uint32_t v = r[g->f] += r[g->b];
  int out = (int)(v >> 1);
  if (++g->f >= 31) g->f = 0;
  if (++g->b >= 31) g->b = 0;
  return out;
}

/* ---- inter-slice policies ---- */

/* ref: downlink-transport-scheduler.cpp:249-272 */
void rso_greedy_by_row(const double* eff, const int* quota, int R, int S, int* rbg_to_slice) {
  std::vector<int> got(S, 0);
  for (int i = 0; i < R; i++) {
    double best = -1;
    int pick = -1;
    for (int j = 0; j < S; j++) {
      if (eff[i * S + j] > best && got[j] < quota[j]) {
        best = eff[i * S + j];
        pick = j;
      }
    }
    rbg_to_slice[i] = pick; /* reference asserts pick != -1 */
    if (pick >= 0) got[pick] += 1;
  }
}

typedef std::pair<int, int> coord_t;
typedef std::pair<coord_t, double> coord_eff_t;

static void sorted_cells(const double* eff, int R, int S, std::vector<coord_eff_t>& v) {
  v.clear();
  for (int i = 0; i < R; i++)
    for (int j = 0; j < S; j++) v.emplace_back(coord_t(i, j), eff[i * S + j]);
  /* the very call the reference makes (:361): libstdc++ introsort, comparator by value */
  std::sort(v.begin(), v.end(), [](coord_eff_t a, coord_eff_t b) { return a.second > b.second; });
}

void rso_maximize_cell_order(const double* eff, int R, int S, int* order) {
  std::vector<coord_eff_t> v;
  sorted_cells(eff, R, S, v);
  for (size_t k = 0; k < v.size(); k++) order[k] = v[k].first.first * S + v[k].first.second;
}

/* ref: downlink-transport-scheduler.cpp:351-376 */
void rso_maximize_cell(const double* eff, const int* quota, int R, int S, int* rbg_to_slice) {
  std::vector<coord_eff_t> v;
  sorted_cells(eff, R, S, v);
  std::vector<int> got(S, 0);
  for (int i = 0; i < R; i++) rbg_to_slice[i] = -1;
  for (size_t k = 0; k < v.size(); k++) {
    int rbg = v[k].first.first, sl = v[k].first.second;
    if (got[sl] < quota[sl] && rbg_to_slice[rbg] == -1) {
      rbg_to_slice[rbg] = sl;
      got[sl] += 1;
    }
  }
}

/* ref: downlink-transport-scheduler.cpp:378-451.  max_diff is an int in the reference (the
 * double difference is truncated on assignment, compared as double). */
void rso_vogel(const double* eff, const int* quota, int R, int S, int* rbg_to_slice) {
  std::vector<int> got(S, 0);
  for (int i = 0; i < R; i++) rbg_to_slice[i] = -1;
  for (int it = 0; it < R; it++) {
    int max_diff = -1;
    int pick_rbg = -1, pick_slice = -1;
    for (int j = 0; j < R; j++) { /* horizontal search */
      if (rbg_to_slice[j] != -1) continue;
      double e1 = -1, e2 = -1;
      int s1 = -1;
      for (int k = 0; k < S; k++) {
        if (got[k] >= quota[k]) continue;
        if (e1 == -1 || eff[j * S + k] > e1) { s1 = k; e1 = eff[j * S + k]; continue; }
        if (e2 == -1 || eff[j * S + k] > e2) { e2 = eff[j * S + k]; continue; }
      }
      if (e1 - e2 > max_diff) { max_diff = (int)(e1 - e2); pick_rbg = j; pick_slice = s1; }
    }
    for (int k = 0; k < S; k++) { /* vertical search */
      if (got[k] >= quota[k]) continue;
      double e1 = -1, e2 = -1;
      int r1 = -1;
      for (int j = 0; j < R; j++) {
        if (rbg_to_slice[j] != -1) continue;
        if (e1 == -1 || eff[j * S + k] > e1) { r1 = j; e1 = eff[j * S + k]; continue; }
        if (e2 == -1 || eff[j * S + k] > e2) { e2 = eff[j * S + k]; continue; }
      }
      if (e1 - e2 > max_diff) { max_diff = (int)(e1 - e2); pick_rbg = r1; pick_slice = k; }
    }
    if (pick_rbg < 0 || pick_slice < 0) return; /* reference: uninitialised coordinates (UB) */
    rbg_to_slice[pick_rbg] = pick_slice;
    got[pick_slice] += 1;
  }
}

/* ref: downlink-transport-scheduler.cpp:274-349.  Every RBG first goes to its best slice (first maximum), then single RBGs
 * move from slices above their quota to slices below it, each time the move that loses the least efficiency; ties go to
 * the first candidate in RBG order and, within an RBG, in the order the `slice_fewer` hashtable yields its keys -- the
 * real std::unordered_map is used here so that the order is libstdc++'s, as in the reference.  Negative quotas count as 0
 * (the reference clamps them in place). */
void rso_subopt(const double* eff, const int* quota_in, int R, int S, int* rbg_to_slice) {
  std::vector<int> quota(quota_in, quota_in + S), got(S, 0);
  for (int j = 0; j < S; j++)
    if (quota[j] < 0) quota[j] = 0;
  for (int i = 0; i < R; i++) {
    double best = -1;
    int pick = -1;
    for (int j = 0; j < S; j++)
      if (eff[i * S + j] > best) { best = eff[i * S + j]; pick = j; }
    rbg_to_slice[i] = pick;
    got[pick] += 1;
  }
  std::unordered_map<int, int> more, fewer;
  for (int j = 0; j < S; j++) {
    if (got[j] > quota[j]) more[j] = got[j] - quota[j];
    else if (got[j] < quota[j]) fewer[j] = quota[j] - got[j];
  }
  while (!more.empty() && !fewer.empty()) {
    int from = -1, to = -1, rbg = -1;
    double least = std::numeric_limits<double>::max();
    for (int i = 0; i < R; i++) {
      const int own = rbg_to_slice[i];
      if (more.find(own) == more.end()) continue;
      for (auto it = fewer.begin(); it != fewer.end(); ++it) {
        const double loss = eff[i * S + own] - eff[i * S + it->first];
        if (loss < least) { least = loss; from = own; to = it->first; rbg = i; }
      }
    }
    if (from < 0) break; /* reference asserts */
    got[from] -= 1;
    got[to] += 1;
    rbg_to_slice[rbg] = to;
    more.at(from) -= 1;
    fewer.at(to) -= 1;
    if (more.at(from) <= 0 || got[from] <= 0) more.erase(from);
    if (fewer.at(to) <= 0) fewer.erase(to);
  }
}

}  // extern "C"

/* ===================================================================================== */

struct rso_cell {
  int S, U, R, rbg_size, sched;
  int synthetic = 0; /* the reference's FIRST/SECOND_SYNTHETIC_EXP transport block (rso_cell_set_synthetic_exp) */
  std::vector<double> w;
  std::vector<int> alpha, beta, eps, psi, u2s;
  /* per-bearer PF state (ref: flows/radio-bearer.h:81-85) */
  std::vector<double> avg, last_update;
  std::vector<int> tx_bytes;
  std::vector<int64_t> cum_bytes, cum_rbs;
  /* scheduler state */
  std::vector<double> offset; /* slice_rbs_offset_ (ref: downlink-transport-scheduler.h:38) */
  std::vector<double> ewma;   /* slice_ewma_time_  (ref: downlink-nvs-scheduler.h:41)       */
  std::vector<uint8_t> cqi;   /* [U][R]  CQI of PRB r*rbg_size (what the metric reads) */
  std::vector<uint8_t> cqi_prb; /* [U][R*G] per-PRB CQI when given (EESM/TBS read every PRB), else empty */
  std::vector<double> hol;      /* [U] GetHeadOfLinePacketDelay() of the slice-priority bearer (alpha != 0 slices) */
  std::vector<uint8_t> prio_has_data; /* [U] m_dataToTransmit[slice_priority_[slice]] != 0 */
  std::vector<double> avg2;     /* [U] average rate of the user's second bearer (MAX_BEARERS = 2), < 0: none */
  double eff_of_cqi[16];
  /* ---- finite queues (rso_cell_enable_queues): two bearers per user, index = priority ---- */
  struct Packet { int size; double ts; int frag_off; }; /* MacQueue::QueueElement (flows/MacQueue.h) */
  struct Bearer {
    int kind = 0;            /* 0 none, 1 InfiniteBuffer, 2 finite queue (InternetFlow / TraceBased) */
    std::deque<Packet> q;    /* MacQueue::m_queue */
    int queue_size = 0;      /* MacQueue::m_queueSize  */
    int n_packets = 0;       /* MacQueue::m_nbDataPackets */
    double avg = 100000;     /* RadioBearer::m_averageTransmissionRate */
    int tx_bytes = 0;        /* m_transmittedBytes */
    double last_update = 0.1;
    int64_t cum_bytes = 0, cum_rbs = 0;
    std::vector<double> arr_time; /* arrival bursts: enqueue instants ... */
    std::vector<int> arr_nfull, arr_last; /* ... full packets of RSO_FULL_PACKET bytes, then one of arr_last bytes (0: none) */
    size_t next_arr = 0;
  };
  std::vector<Bearer> bearers; /* [U][2]; empty: backlogged mode */
  std::vector<uint8_t> active; /* [U] user is in UsersToSchedule this TTI */
  std::vector<double> avgsum;  /* [U] 1 + averages of the bearers in the user's record (summed in index order) */
  std::vector<int> data_tx;    /* [U][2] m_dataToTransmit */
  std::vector<long> required_rbs; /* [U] m_requiredRBs (sched 7) */
  /* scratch of allocate_transport, kept between TTIs (no per-TTI heap traffic when many cells run on many threads) */
  std::vector<double> scratch_metrics, scratch_slice_eff, scratch_max_rank;
  std::vector<int> scratch_user_index;
};

extern "C" {

rso_cell* rso_cell_create(const rso_config* cfg) {
  rso_cell* c = new rso_cell();
  c->S = cfg->n_slices; c->U = cfg->n_users; c->R = cfg->n_rbgs; c->rbg_size = cfg->rbg_size;
  c->sched = cfg->sched;
  c->w.assign(cfg->weights, cfg->weights + c->S);
  c->alpha.assign(cfg->alpha, cfg->alpha + c->S);
  c->beta.assign(cfg->beta, cfg->beta + c->S);
  c->eps.assign(cfg->epsilon, cfg->epsilon + c->S);
  c->psi.assign(cfg->psi, cfg->psi + c->S);
  c->u2s.assign(cfg->user_to_slice, cfg->user_to_slice + c->U);
  c->avg.assign(c->U, 100000); /* ref: flows/radio-bearer.cpp:54 */
  c->last_update.assign(c->U, 0.1);
  c->tx_bytes.assign(c->U, 0);
  c->cum_bytes.assign(c->U, 0);
  c->cum_rbs.assign(c->U, 0);
  c->offset.assign(c->S, 0);
  c->ewma.assign(c->S, 0);
  c->cqi.assign((size_t)c->U * c->R, 10); /* ref: device/ENodeB.cpp:212-217 initial CQI 10 */
  c->eff_of_cqi[0] = 0;
  for (int q = 1; q <= 15; q++) c->eff_of_cqi[q] = rso_efficiency_from_cqi(q);
  return c;
}

void rso_cell_destroy(rso_cell* c) { delete c; }

void rso_cell_set_cqi(rso_cell* c, const uint8_t* cqi) {
  memcpy(c->cqi.data(), cqi, (size_t)c->U * c->R);
  c->cqi_prb.clear();
}
/* per-PRB CQI vectors as ENodeB::UserEquipmentRecord::GetCQI() holds them: the metric reads PRB
 * rbg*rbg_size (downlink-transport-scheduler.cpp:536), link adaptation every allocated PRB (:643-646) */
void rso_cell_set_cqi_prb(rso_cell* c, const uint8_t* prb) {
  const int n = c->R * c->rbg_size;
  c->cqi_prb.assign(prb, prb + (size_t)c->U * n);
  for (int u = 0; u < c->U; u++)
    for (int r = 0; r < c->R; r++) c->cqi[(size_t)u * c->R + r] = prb[(size_t)u * n + r * c->rbg_size];
}
void rso_cell_set_user_cqi(rso_cell* c, int user, const uint8_t* row) {
  memcpy(&c->cqi[(size_t)user * c->R], row, c->R);
}
void rso_cell_set_last_update(rso_cell* c, double t) { c->last_update.assign(c->U, t); }
/* slice_rbs_offset_ (downlink-transport-scheduler.h:38) from outside: lets a test follow a context whose calls the oracle did not all take part in */
/* (schedulers 7 and 11: slice_ewma_time_, downlink-nvs-scheduler.h:41 -- the array rso_cell_get_state returns as slice_state) */
void rso_cell_set_slice_offset(rso_cell* c, const double* offset) {
  ((c->sched == RSO_SCHED_NVS || c->sched == RSO_SCHED_NVS_NONGREEDY) ? c->ewma : c->offset).assign(offset, offset + c->S);
}
void rso_cell_set_synthetic_exp(rso_cell* c, int on) { c->synthetic = on ? 1 : 0; }
/* queue state the customised (alpha = 1) slice metrics read: downlink-transport-scheduler.cpp:694-711 */
void rso_cell_set_queue_state(rso_cell* c, const double* hol, const uint8_t* prio_has_data) {
  c->hol.assign(hol, hol + c->U);
  c->prio_has_data.assign(prio_has_data, prio_has_data + c->U);
}
void rso_cell_set_avg_rate(rso_cell* c, const double* a) { c->avg.assign(a, a + c->U); }
void rso_cell_set_second_bearer_avg(rso_cell* c, const double* a2) {
  if (a2) c->avg2.assign(a2, a2 + c->U); else c->avg2.clear();
}

void rso_cell_get_state(const rso_cell* c, double* avg, int64_t* cum_bytes, int64_t* cum_rbs,
                        double* slice_state) {
  if (avg) memcpy(avg, c->avg.data(), sizeof(double) * c->U);
  if (cum_bytes) memcpy(cum_bytes, c->cum_bytes.data(), sizeof(int64_t) * c->U);
  if (cum_rbs) memcpy(cum_rbs, c->cum_rbs.data(), sizeof(int64_t) * c->U);
  if (slice_state)
    memcpy(slice_state, ((c->sched == RSO_SCHED_NVS || c->sched == RSO_SCHED_NVS_NONGREEDY) ? c->ewma : c->offset).data(), sizeof(double) * c->S);
}

}  // extern "C"

namespace {

inline uint8_t prb_cqi(const rso_cell* c, int u, int r, int k) {
  if (c->cqi_prb.empty()) return c->cqi[(size_t)u * c->R + r];
  return c->cqi_prb[(size_t)u * c->R * c->rbg_size + r * c->rbg_size + k];
}

/* ref: flows/radio-bearer.cpp:139-164 */
void update_average_rate(rso_cell* c, double now) {
  for (int u = 0; u < c->U; u++) {
    if (now == c->last_update[u]) continue;
    double rate = (c->tx_bytes[u] * 8) / (now - c->last_update[u]);
    double beta = 0.02;
    c->avg[u] = ((1 - beta) * c->avg[u]) + (beta * rate);
    if (c->avg[u] < 1) c->avg[u] = 1;
    c->tx_bytes[u] = 0;
    c->last_update[u] = now;
  }
}

/* ref: downlink-transport-scheduler.cpp:677-713 and downlink-nvs-scheduler.cpp:360-390 (the NVS variant
 * always multiplies the head-of-line delay when alpha != 0).  `averageRate = 1; for each bearer of the user:
 * averageRate += its average` (:681-686), i.e. (1 + a) + a2 with two bearers. */
double slice_metric(const rso_cell* c, int slice, double se, double avg_rate, int user = -1) {
  double average = 1;
  if (user >= 0 && !c->avgsum.empty()) {
    average = c->avgsum[user]; /* queue mode: 1 + every bearer of the record, summed when the record was built */
  } else {
    average += avg_rate;
    if (user >= 0 && !c->avg2.empty() && c->avg2[user] >= 0) average += c->avg2[user];
  }
  se = se * 180000 / 1000;
  average /= 1000.0;
  if (c->alpha[slice] == 0) return pow(se, c->eps[slice]) / pow(average, c->psi[slice]);
  /* the prioritized flow has no packet: metric 0 */
  if (user >= 0 && !c->prio_has_data.empty() && c->prio_has_data[user] == 0) return 0;
  if (c->sched == RSO_SCHED_NVS || c->beta[slice]) {
    double HoL = (user >= 0 && !c->hol.empty()) ? c->hol[user] : 0;
    return HoL * pow(se, c->eps[slice]) / pow(average, c->psi[slice]);
  }
  return pow(se, c->eps[slice]) / pow(average, c->psi[slice]);
}

/* link adaptation tail shared by all schedulers
 * (ref: downlink-transport-scheduler.cpp:630-674, downlink-nvs-scheduler.cpp:313-357,
 *  downlink-packet-scheduler.cpp:268-322): per user, PRBs in RBG-ascending order. */
/* the reference's FIRST_SYNTHETIC_EXP / SECOND_SYNTHETIC_EXP build (CONFIG/global_config:57-58, off as shipped): the transport
 * block "as if the user can have multiple mcs" -- every allocated PRB with the MCS of its own CQI
 * (ref: downlink-transport-scheduler.cpp:653-659, downlink-nvs-scheduler.cpp:336-342; the per-flow PF scheduler and the NVS sampler
 * have no such branch) */
static bool synthetic_tb(const rso_cell* c) {
  return c->synthetic && (c->sched == RSO_SCHED_NVS || c->sched == RSO_SCHED_SEQUENTIAL || c->sched == RSO_SCHED_MAXCELL ||
                          c->sched == RSO_SCHED_SUBOPT || c->sched == RSO_SCHED_VOGEL || c->sched == RSO_SCHED_UPPERBOUND);
}
static int synthetic_tbs_bits(const uint8_t* prb, int n) {
  int tbs = 0;
  for (int i = 0; i < n; i++) /* GetTBSizeFromMCS(GetMCSFromCQI(GetCQIFromSinr(estimatedSinrValues[i])), 1) */
    tbs += rso_tbs_bits(kCqiToMcs[rso_cqi_from_sinr(kSinrForCqi[prb[i] - 1]) - 1], 1);
  return tbs;
}

void link_adaptation(const rso_cell* c, const int* rbg_to_user, rso_tti_out* out) {
  const int U = c->U, R = c->R, G = c->rbg_size;
  for (int u = 0; u < U; u++) {
    out->user_nprb[u] = 0; out->user_final_cqi[u] = 0; out->user_mcs[u] = 0; out->user_tbs_bits[u] = 0;
  }
  std::vector<uint8_t> prb;
  for (int u = 0; u < U; u++) {
    prb.clear();
    for (int r = 0; r < R; r++)
      if (rbg_to_user[r] == u)
        for (int k = 0; k < G; k++) prb.push_back(prb_cqi(c, u, r, k));
    if (prb.empty()) continue;
    int fc = rso_final_cqi(prb.data(), (int)prb.size());
    int mcs = kCqiToMcs[fc - 1];
    out->user_nprb[u] = (int)prb.size();
    out->user_final_cqi[u] = fc;
    out->user_mcs[u] = mcs;
    out->user_tbs_bits[u] = synthetic_tb(c) ? synthetic_tbs_bits(prb.data(), (int)prb.size()) : rso_tbs_bits(mcs, (int)prb.size());
  }
}

/* the same tail when the PRBs of a user are not in RBG-ascending order (UpperBound pushes every slice's RBGs in that
 * slice's sorted order, :603-616): lists[u] = the user's RBGs in push order */
void link_adaptation_lists(const rso_cell* c, const std::vector<std::vector<int>>& lists, rso_tti_out* out) {
  const int U = c->U, G = c->rbg_size;
  std::vector<uint8_t> prb;
  for (int u = 0; u < U; u++) {
    out->user_nprb[u] = 0; out->user_final_cqi[u] = 0; out->user_mcs[u] = 0; out->user_tbs_bits[u] = 0;
    if (lists[u].empty()) continue;
    prb.clear();
    for (int r : lists[u])
      for (int k = 0; k < G; k++) prb.push_back(prb_cqi(c, u, r, k));
    int fc = rso_final_cqi(prb.data(), (int)prb.size());
    int mcs = kCqiToMcs[fc - 1];
    out->user_nprb[u] = (int)prb.size();
    out->user_final_cqi[u] = fc;
    out->user_mcs[u] = mcs;
    out->user_tbs_bits[u] = synthetic_tb(c) ? synthetic_tbs_bits(prb.data(), (int)prb.size()) : rso_tbs_bits(mcs, (int)prb.size());
  }
}

/* DownlinkTransportScheduler::RBsAllocation, ref: downlink-transport-scheduler.cpp:453-675 */
int allocate_transport(rso_cell* c, const double* avg, int rand0, int rand1, rso_tti_out* out,
                       bool commit) {
  const int S = c->S, U = c->U, R = c->R, G = c->rbg_size;
  int nb_rbs = R * G; /* already a multiple of rbg_size (:460) */
  /* :463-477 targets for slices that have at least one user */
  std::vector<char> with_data(S, 0);
  std::vector<int> target(S, 0);
  int nonempty = 0, extra_rbs = nb_rbs;
  const bool listed = !c->active.empty(); /* queue mode: only the users with queued data are in UsersToSchedule */
  for (int u = 0; u < U; u++) {
    if (listed && !c->active[u]) continue;
    int s = c->u2s[u];
    if (with_data[s]) continue;
    nonempty += 1;
    with_data[s] = 1;
    target[s] = (int)(nb_rbs * c->w[s] + c->offset[s]);
    extra_rbs -= target[s];
  }
  if (nonempty == 0) return -1;
  /* :489-500 spread the spare PRBs, remainder to the first non-empty slice from rand()%S */
  bool first = true;
  for (int i = 0; i < S; i++) {
    int k = (i + rand0) % S;
    if (with_data[k]) {
      target[k] += extra_rbs / nonempty;
      if (first) { target[k] += extra_rbs % nonempty; first = false; }
    }
  }
  /* :501-521 RBG quotas */
  std::vector<int> quota(S, 0), final_rbgs(S, 0);
  int extra_rbgs = R;
  for (int i = 0; i < S; i++) { quota[i] = (int)(target[i] / G); extra_rbgs -= quota[i]; }
  first = true;
  for (int i = 0; i < S; i++) {
    int k = (rand1 + i) % S;
    if (with_data[k]) {
      quota[k] += extra_rbgs / nonempty;
      if (first) { quota[k] += extra_rbgs % nonempty; first = false; }
    }
  }
  for (int s = 0; s < S; s++) { out->target_rbs[s] = target[s]; out->quota_rbgs[s] = quota[s]; }
  /* :530-539 metric matrix */
  std::vector<double>& metrics = c->scratch_metrics;
  metrics.resize((size_t)R * U);
  for (int i = 0; i < R; i++)
    for (int j = 0; j < U; j++)
      if (!listed || c->active[j])
        metrics[(size_t)i * U + j] = slice_metric(c, c->u2s[j], c->eff_of_cqi[c->cqi[(size_t)j * R + i]], avg[j], j);
  /* :545-567 best user of every slice in every RBG, strict '>' from -1: first max wins */
  std::vector<int>& user_index = c->scratch_user_index;
  std::vector<double>& slice_eff = c->scratch_slice_eff;
  std::vector<double>& max_rank = c->scratch_max_rank;
  user_index.assign((size_t)R * S, -1);
  slice_eff.assign((size_t)R * S, 0);
  for (int i = 0; i < R; i++) {
    max_rank.assign(S, -1);
    for (int j = 0; j < U; j++) {
      if (listed && !c->active[j]) continue;
      int s = c->u2s[j];
      if (metrics[(size_t)i * U + j] > max_rank[s]) {
        max_rank[s] = metrics[(size_t)i * U + j];
        user_index[(size_t)i * S + s] = j;
        slice_eff[(size_t)i * S + s] = c->eff_of_cqi[c->cqi[(size_t)j * R + i]];
      }
    }
  }
  if (out->slice_eff)
    for (int i = 0; i < R * S; i++) { out->slice_eff[i] = slice_eff[i]; out->slice_user[i] = user_index[i]; }
  if (c->sched == RSO_SCHED_UPPERBOUND) {
    /* UpperBound, ref: :223-246 and the inter_sched_ >= 4 branch of the apply step :603-616.  Every slice with a positive
     * quota sorts ITS R (rbg, eff) pairs with the same unstable std::sort call and takes its first quota[j] RBGs,
     * whatever the other slices take: several slices may hold one RBG (it is an upper bound, not an allocation).
     * The reference walks an unordered_map of slices; users of different slices are distinct, so the walk order
     * does not reach any result.  quota[j] > R would read past the vector in the reference; clamped here. */
    std::vector<std::vector<int>> lists(U);
    for (int i = 0; i < R; i++) out->rbg_to_user[i] = -1;
    if (out->upper_rbg)
      for (int i = 0; i < S * R; i++) { out->upper_rbg[i] = -1; out->upper_user[i] = -1; }
    for (int j = 0; j < S; j++) {
      if (quota[j] <= 0) continue;
      std::vector<std::pair<int, double>> v;
      for (int i = 0; i < R; i++) v.emplace_back(i, slice_eff[(size_t)i * S + j]);
      std::sort(v.begin(), v.end(), [](std::pair<int, double> a, std::pair<int, double> b) { return a.second > b.second; });
      int take = std::min(quota[j], R);
      for (int k = 0; k < take; k++) {
        int rbg = v[k].first;
        int u = user_index[(size_t)rbg * S + j];
        if (u < 0) return -5; /* reference: assert(uindex != -1) */
        lists[u].push_back(rbg);
        if (out->upper_rbg) { out->upper_rbg[j * R + k] = rbg; out->upper_user[j * R + k] = u; }
        /* reporting convention of this restatement (the reference has no RBG -> UE map here): the user of the
         * lowest-numbered slice that took the RBG */
        if (out->rbg_to_user[rbg] < 0) out->rbg_to_user[rbg] = u;
      }
      final_rbgs[j] += take;
    }
    if (commit)
      for (int s2 = 0; s2 < S; s2++) c->offset[s2] = target[s2] - final_rbgs[s2] * G;
    link_adaptation_lists(c, lists, out);
    out->served_slice = -1;
    return 0;
  }
  /* :570-586 */
  std::vector<int> rbg_to_slice(R, -1);
  switch (c->sched) {
    case RSO_SCHED_SEQUENTIAL: rso_greedy_by_row(slice_eff.data(), quota.data(), R, S, rbg_to_slice.data()); break;
    case RSO_SCHED_MAXCELL: rso_maximize_cell(slice_eff.data(), quota.data(), R, S, rbg_to_slice.data()); break;
    case RSO_SCHED_VOGEL: rso_vogel(slice_eff.data(), quota.data(), R, S, rbg_to_slice.data()); break;
    case RSO_SCHED_SUBOPT: rso_subopt(slice_eff.data(), quota.data(), R, S, rbg_to_slice.data()); break;
    default: return -2;
  }
  /* :589-601 apply; an RBG MaximizeCell could not place stays unassigned (reference would
   * index user_index[i][-1]: UB; cannot happen while sum(quota) == R and every slice has users) */
  for (int i = 0; i < R; i++) {
    int s = rbg_to_slice[i];
    int u = s >= 0 ? user_index[(size_t)i * S + s] : -1;
    out->rbg_to_user[i] = u;
    if (u >= 0) final_rbgs[s] += 1;
  }
  /* :618-620 */
  if (commit)
    for (int s = 0; s < S; s++) c->offset[s] = target[s] - final_rbgs[s] * G;
  link_adaptation(c, out->rbg_to_user, out);
  out->served_slice = -1;
  return 0;
}

/* DownlinkPacketScheduler::RBsAllocation + DL_PF metric,
 * ref: downlink-packet-scheduler.cpp:179-331, dl-pf-packet-scheduler.cpp:128-140 */
int allocate_pf(rso_cell* c, const double* avg, rso_tti_out* out, const std::vector<int>* list = nullptr,
                const int32_t* gate = nullptr) {
  const int U = c->U, R = c->R, G = c->rbg_size;
  /* the flows of the call in container order: every user, or the listed ones (ascending); gate[i] belongs to the i-th of them */
  const int n = list ? (int)list->size() : U;
  for (int s = 0; s < c->S; s++) { out->target_rbs[s] = 0; out->quota_rbgs[s] = 0; }
  std::vector<char> done(n, 0);
  std::vector<std::vector<uint8_t>> prbs(n);
  int n_done = 0;
  for (int r = 0; r < R; r++) {
    out->rbg_to_user[r] = -1;
    if (n_done == n) continue; /* :223-224 break */
    double target = 0;
    int pick = -1;
    for (int i = 0; i < n; i++) {
      const int k = list ? (*list)[i] : i;
      double se = c->eff_of_cqi[c->cqi[(size_t)k * R + r]];
      double metric = (se * 180000.) / avg[k];
      if (metric > target && !done[i]) { target = metric; pick = i; }
    }
    if (pick < 0) continue;
    const int user = list ? (*list)[pick] : pick;
    out->rbg_to_user[r] = user;
    for (int k = 0; k < G; k++) prbs[pick].push_back(prb_cqi(c, user, r, k));
    /* :253-265 incremental TBS test against dataToTransmit*8 (an InfiniteBuffer flow: 800 000 000 bits) */
    int fc = rso_final_cqi(prbs[pick].data(), (int)prbs[pick].size());
    int tbs = rso_tbs_bits(kCqiToMcs[fc - 1], (int)prbs[pick].size());
    const int data = gate ? gate[pick] : 100000000;
    if (tbs >= data * 8) { done[pick] = 1; n_done++; }
  }
  link_adaptation(c, out->rbg_to_user, out);
  out->served_slice = -1;
  return 0;
}

/* DownlinkNVSScheduler: SelectSliceToServe + RBsAllocation,
 * ref: downlink-nvs-scheduler.cpp:94-142, :275-358 */
int nvs_select_slice(rso_cell* c) {
  const int S = c->S;
  std::vector<char> with_queue(S, 0);
  if (c->bearers.empty()) {
    for (int u = 0; u < c->U; u++) with_queue[c->u2s[u]] = 1;
  } else {
    /* :101-121: a slice counts when one of its bearers has packets and dataToTransmit > 0 */
    for (int u = 0; u < c->U; u++)
      for (int b = 0; b < 2; b++) {
        const rso_cell::Bearer& br = c->bearers[(size_t)u * 2 + b];
        if (br.kind == 1 || (br.kind == 2 && !br.q.empty() && br.queue_size + br.n_packets * 8 > 0)) with_queue[c->u2s[u]] = 1;
      }
  }
  int slice_id = 0;
  double max_score = 0;
  for (int i = 0; i < S; i++) {
    if (!with_queue[i]) continue;
    if (c->ewma[i] == 0) { slice_id = i; break; }
    double score = c->w[i] / c->ewma[i];
    if (score >= max_score) { max_score = score; slice_id = i; }
  }
  const double beta = 0.01; /* downlink-nvs-scheduler.h:42 */
  for (int i = 0; i < S; i++) {
    if (!with_queue[i]) continue;
    c->ewma[i] = (1 - beta) * c->ewma[i];
    if (i == slice_id) c->ewma[i] += beta * 1;
  }
  return slice_id;
}

/* required_in [U] by user id: m_requiredRBs from the caller (the gate of :299-300 as an input); NULL: formed here as
 * InsertFlowToUser does */
int allocate_nvs(rso_cell* c, const double* avg, int slice, rso_tti_out* out, const long* required_in = nullptr) {
  const int U = c->U, R = c->R, G = c->rbg_size;
  for (int s = 0; s < c->S; s++) { out->target_rbs[s] = 0; out->quota_rbgs[s] = 0; }
  /* m_requiredRBs (packet-scheduler.cpp:319-334): wideband CQI over ALL PRBs, then
   * dataToTransmit*8 / TBS(1 PRB); >= 800e6/712 > 512, so the gate at :299-300 never binds,
   * but it is restated for fidelity. */
  std::vector<long> required(U, 0);
  std::vector<int> got(U, 0);
  std::vector<uint8_t> all(R * G);
  const bool listed = !c->active.empty(); /* queue mode: only the users of the slice that have queued data */
  for (int u = 0; u < U; u++) {
    if (c->u2s[u] != slice || (listed && !c->active[u])) continue;
    if (required_in) { required[u] = required_in[u]; continue; }
    for (int r = 0; r < R; r++)
      for (int k = 0; k < G; k++) all[r * G + k] = prb_cqi(c, u, r, k);
    int wide = rso_final_cqi(all.data(), R * G);
    /* InsertFlowToUser adds to m_requiredRBs only when it creates the user's record, i.e. for the first bearer seen */
    int first_data = 100000000;
    const bool queues = listed && !c->data_tx.empty(); /* (a listed call on a backlogged cell: InfiniteBuffer flows) */
    if (queues) first_data = c->data_tx[(size_t)u * 2] > 0 ? c->data_tx[(size_t)u * 2] : c->data_tx[(size_t)u * 2 + 1];
    required[u] = (first_data * 8) / kTbs[0][kMcsToItbs[kCqiToMcs[wide - 1]]];
    if (queues) c->required_rbs[u] = required[u];
  }
  for (int r = 0; r < R; r++) {
    double target = std::numeric_limits<double>::lowest();
    int pick = -1;
    for (int u = 0; u < U; u++) {
      if (c->u2s[u] != slice || (listed && !c->active[u])) continue;
      double m = slice_metric(c, slice, c->eff_of_cqi[c->cqi[(size_t)u * R + r]], avg[u], u);
      if (m > target && (long)got[u] < required[u]) { target = m; pick = u; }
    }
    out->rbg_to_user[r] = pick;
    if (pick >= 0) got[pick] += G;
  }
  link_adaptation(c, out->rbg_to_user, out);
  out->served_slice = slice;
  return 0;
}

/* DoStopSchedule accounting, ref: downlink-transport-scheduler.cpp:170-221 (bytes = bits/8,
 * min with dataToTransmit = 1e8), radio-bearer.cpp:100-124 */
void account(rso_cell* c, const rso_tti_out* out) {
  for (int u = 0; u < c->U; u++) {
    int bytes = out->user_tbs_bits[u] / 8;
    if (bytes <= 0) continue;
    int sent = std::min(bytes, 100000000);
    c->tx_bytes[u] += sent;
    c->cum_bytes[u] += sent;
    c->cum_rbs[u] += out->user_nprb[u];
  }
}

/* DownlinkNVSScheduler::RBsAllocationNonGreedyPF + AssignRBsGivenMCS, ref: downlink-nvs-scheduler.cpp:405-528.
 * 300 times: every user of the served slice draws an "MCS" (a CQI index) max(highest_cqi - rand() % 4, 1); with those,
 * every RBG goes to the first user with the largest  eff(mcs) * 180000 / (1 + avg)  among the users whose CQI on the RBG
 * reaches their MCS (0 otherwise; strict '<' from -1: first maximum wins), and the sample's score is the sum of the
 * winners' metrics in RBG order.  The first sample with the strictly largest score (from 0) is applied.  Restated from
 * the cited lines; no reference output exists for this scheduler here. */
int allocate_nvs_nongreedy(rso_cell* c, const double* avg, int slice, const int* draws, int n_draws, rso_tti_out* out) {
  const int U = c->U, R = c->R;
  for (int s = 0; s < c->S; s++) { out->target_rbs[s] = 0; out->quota_rbgs[s] = 0; }
  std::vector<int> users;
  for (int u = 0; u < U; u++)
    if (c->u2s[u] == slice) users.push_back(u);
  const int n = (int)users.size();
  if (n_draws != RSO_NONGREEDY_SAMPLES * n) return -6;
  std::vector<int> highest(n, 0);
  for (int i = 0; i < n; i++)
    for (int r = 0; r < R; r++) highest[i] = std::max(highest[i], (int)prb_cqi(c, users[i], r, 0)); /* :417-424 */
  std::vector<int> best_assign;
  double best = 0;
  std::vector<int> mcs(n), assign(R);
  for (int smp = 0; smp < RSO_NONGREEDY_SAMPLES; smp++) {
    for (int i = 0; i < n; i++) mcs[i] = std::max(highest[i] - draws[(size_t)smp * n + i] % 4, 1); /* :436-440 */
    double pf = 0;
    for (int r = 0; r < R; r++) { /* AssignRBsGivenMCS :508-527 */
      double highest_metric = -1;
      assign[r] = -1;
      for (int i = 0; i < n; i++) {
        int cqi = prb_cqi(c, users[i], r, 0);
        double metric = 0;
        if (mcs[i] <= cqi) {
          double sEff = c->eff_of_cqi[mcs[i]];
          double rate = 1;  /* UserToSchedule::GetAverageTransmissionRate, packet-scheduler.cpp:424-433 */
          rate += avg[users[i]];
          metric = sEff * 180000 / rate;
        }
        if (highest_metric < metric) { highest_metric = metric; assign[r] = users[i]; }
      }
      pf += highest_metric;
    }
    if (best < pf) { best = pf; best_assign = assign; }
  }
  /* :451-459 -- nothing is allocated when no sample scored above 0 (the best assignment stays empty) */
  for (int r = 0; r < R; r++) out->rbg_to_user[r] = best_assign.empty() ? -1 : best_assign[r];
  link_adaptation(c, out->rbg_to_user, out);
  out->served_slice = slice;
  return 0;
}

}  // namespace

extern "C" {

int rso_cell_allocate_nongreedy(rso_cell* c, const double* avg_rate, int slice, const int* draws, int n_draws,
                                rso_tti_out* out) {
  return allocate_nvs_nongreedy(c, avg_rate, slice, draws, n_draws, out);
}

int rso_cell_step_rng(rso_cell* c, double now, rso_rng* g, rso_tti_out* out) {
  if (c->sched != RSO_SCHED_NVS_NONGREEDY) return -7;
  int slice = nvs_select_slice(c); /* same DoSchedule as sched 7 (downlink-nvs-scheduler.cpp:196-218) */
  update_average_rate(c, now);
  int n = 0;
  for (int u = 0; u < c->U; u++) n += c->u2s[u] == slice;
  std::vector<int> draws((size_t)RSO_NONGREEDY_SAMPLES * n);
  for (size_t i = 0; i < draws.size(); i++) draws[i] = rso_rand(g);
  int rc = allocate_nvs_nongreedy(c, c->avg.data(), slice, draws.data(), (int)draws.size(), out);
  if (rc == 0) account(c, out);
  return rc;
}

int rso_cell_allocate(rso_cell* c, const double* avg, int rand0, int rand1, rso_tti_out* out) {
  for (int s = 0; s < c->S; s++)
    if (c->alpha[s] != 0 && c->hol.empty()) return -3; /* customised slices need rso_cell_set_queue_state */
  switch (c->sched) {
    case RSO_SCHED_PF: return allocate_pf(c, avg, out);
    case RSO_SCHED_NVS: return -4; /* needs the slice choice: use rso_cell_step */
    case RSO_SCHED_NVS_NONGREEDY: return -4; /* rso_cell_allocate_nongreedy / rso_cell_step_rng */
    default: return allocate_transport(c, avg, rand0, rand1, out, true);
  }
}

/* RBsAllocation() of one call for a listed set of users, with the per-user gate as an input: what rs_schedule_tti sees when the
 * caller names users through rs_tti_in.user_id and passes required_rbs / data_to_transmit.  PARITY UNPINNED: restated from
 *   sched 7: downlink-nvs-scheduler.cpp:275-312 -- the race of every RBG starts from numeric_limits<double>::lowest() (:294), a user
 *            competes while `GetListOfAllocatedRBs()->size() < m_requiredRBs` (:299-300; gate[i] = m_requiredRBs of the i-th listed
 *            user), the metric is ComputeSchedulingMetric (:360-390: libm pow with the slice's integer exponents, alpha, HoL);
 *   sched 1: downlink-packet-scheduler.cpp:179-331 -- first maximum from 0 over the listed flows, a flow leaves once
 *            `transportBlockSize >= GetDataToTransmit() * 8` (:253-265; gate[i] = GetDataToTransmit() of the i-th listed flow);
 *   sched 8 / 9 / 10 / 101 / 103: downlink-transport-scheduler.cpp:453-675 on GetUsersToSchedule() = the listed users (a slice
 *            without a listed user has no target and no quota, :463-477); slice_rbs_offset_ is carried as by rso_cell_allocate.
 * user_ids ascending, NULL = every user; outputs stay indexed by the cell's user id.  c->active is set for the call and restored.
 * -8: bad list (not ascending, out of range, or for sched 7 a user outside `slice`), -9: a gate for a scheduler that has none. */
int rso_cell_allocate_listed(rso_cell* c, const double* avg, const int32_t* user_ids, int n, int slice, const int32_t* gate,
                             int rand0, int rand1, rso_tti_out* out) {
  const int U = c->U;
  if (c->sched == RSO_SCHED_NVS_NONGREEDY) return -4;
  if (c->sched == RSO_SCHED_NVS && (slice < 0 || slice >= c->S)) return -8;
  for (int s = 0; s < c->S; s++)
    if (c->alpha[s] != 0 && c->hol.empty() && (c->sched != RSO_SCHED_NVS || s == slice)) return -3;
  if (gate && c->sched != RSO_SCHED_NVS && c->sched != RSO_SCHED_PF) return -9;
  std::vector<int> list;
  if (user_ids) {
    for (int i = 0; i < n; i++) {
      if (user_ids[i] < 0 || user_ids[i] >= U || (i > 0 && user_ids[i] <= user_ids[i - 1])) return -8;
      if (c->sched == RSO_SCHED_NVS && c->u2s[user_ids[i]] != slice) return -8;
      list.push_back(user_ids[i]);
    }
  } else {
    for (int u = 0; u < U; u++)
      if (c->sched != RSO_SCHED_NVS || c->u2s[u] == slice) list.push_back(u);
  }
  if (c->sched == RSO_SCHED_PF) return allocate_pf(c, avg, out, &list, gate);
  std::vector<uint8_t> saved(U, 0);
  for (int u : list) saved[u] = 1;
  saved.swap(c->active);
  int rc;
  if (c->sched == RSO_SCHED_NVS) {
    std::vector<long> required(U, 0);
    if (gate)
      for (size_t i = 0; i < list.size(); i++) required[list[i]] = gate[i];
    rc = allocate_nvs(c, avg, slice, out, gate ? required.data() : nullptr);
  } else {
    rc = allocate_transport(c, avg, rand0, rand1, out, true); /* -1: no listed user (DoSchedule :160-165 does not call it) */
  }
  saved.swap(c->active);
  return rc;
}

/* read-only: what the last rso_cell_step_queues left in the users' records -- active [U] (in UsersToSchedule; sched 7: of the served
 * slice), data_tx [U][2] (m_dataToTransmit), required_rbs [U] (m_requiredRBs, sched 7); any pointer may be NULL; -20 without queues */
int rso_cell_get_gates(const rso_cell* c, uint8_t* active, int32_t* data_tx, int64_t* required_rbs) {
  if (c->bearers.empty()) return -20;
  for (int u = 0; u < c->U; u++) {
    if (active) active[u] = c->active[u];
    if (data_tx) { data_tx[u * 2] = c->data_tx[(size_t)u * 2]; data_tx[u * 2 + 1] = c->data_tx[(size_t)u * 2 + 1]; }
    if (required_rbs) required_rbs[u] = c->required_rbs[u];
  }
  return 0;
}

/* DoSchedule(), ref: downlink-transport-scheduler.cpp:152-168, downlink-nvs-scheduler.cpp:196-218,
 * downlink-packet-scheduler.cpp:96-114 */
int rso_cell_step(rso_cell* c, double now, int rand0, int rand1, rso_tti_out* out) {
  for (int s = 0; s < c->S; s++)
    if (c->alpha[s] != 0) return -3;
  int rc;
  if (c->sched == RSO_SCHED_NVS) {
    int slice = nvs_select_slice(c); /* before the EWMA update (:207-208) */
    update_average_rate(c, now);
    rc = allocate_nvs(c, c->avg.data(), slice, out);
  } else {
    update_average_rate(c, now);
    rc = rso_cell_allocate(c, c->avg.data(), rand0, rand1, out);
  }
  if (rc == 0) account(c, out);
  return rc;
}

/* The simulated clock: every subframe is scheduled at Now() + 0.001 in double (ref: core/eventScheduler/simulator.cc:117-126
 * DoSchedule: timeStamp = time + Now(); componentManagers/FrameManager.cpp:186-188), so t_k = fl(t_{k-1} + 0.001) from 0.
 * Pinned against the reference's own Simulator/Calendar compiled in place (oracle/_ref/libref_clock.so). */
static inline double clock_advance(double t) { return t + 0.001; }

void rso_clock_ticks(int first_tti, int n, double* out) {
  double t = 0;
  for (int k = 0; k < first_tti; k++) t = clock_advance(t);
  for (int k = 0; k < n; k++) { out[k] = t; t = clock_advance(t); }
}

static bool uses_rand(int sched) {
  return sched == RSO_SCHED_SEQUENTIAL || sched == RSO_SCHED_MAXCELL || sched == RSO_SCHED_VOGEL || sched == RSO_SCHED_UPPERBOUND ||
         sched == RSO_SCHED_SUBOPT;
}

static thread_local bool g_trace_per_prb = false;
/* rso_run_trace with run->trace = [n_traces][n_rows][R*rbg_size] */
int rso_run_trace_prb(rso_cell* c, const rso_trace_run* run, int* log_map, int* log_fcqi, int* log_quota,
                      int* log_target, int* log_tbs) {
  g_trace_per_prb = true;
  int rc = rso_run_trace(c, run, log_map, log_fcqi, log_quota, log_target, log_tbs);
  g_trace_per_prb = false;
  return rc;
}
int rso_run_trace(rso_cell* c, const rso_trace_run* run, int* log_map, int* log_fcqi, int* log_quota,
                  int* log_target, int* log_tbs) {
  const int S = c->S, U = c->U, R = c->R;
  rso_rng g;
  rso_srand(&g, run->seed);
  for (long i = 0; i < run->rand_skip; i++) (void)rso_rand(&g);
  std::vector<int> target(S), quota(S), map(R), nprb(U), fcqi(U), mcs(U), tbs(U);
  rso_tti_out out = {target.data(), quota.data(), map.data(), nprb.data(), fcqi.data(), mcs.data(), tbs.data(), -1, nullptr, nullptr, nullptr, nullptr};
  /* simulated time: every event is scheduled at Now()+0.001 in double
   * (simulator.cc:117-126, FrameManager.cpp:186-188): t_k = fl(t_{k-1} + 0.001) */
  double t = 0;
  for (int k = 0; k < run->first_tti; k++) t = clock_advance(t);
  rso_cell_set_last_update(c, 0.1); /* bearers are created by the application start event at 0.1 s */
  long last_sent = 0;               /* CqiManager::m_lastSent (uninitialised; behaves as 0) */
  bool reported = false;
  int served_prev = 0;
  for (int n = 0; n < run->n_ttis; n++) {
    /* UE side, runs before the scheduler at equal timestamps (calendar.cpp:58-68):
     * error model draw for every UE that received PRBs in the previous TTI */
    if (run->phy_error_draws)
      for (int i = 0; i < served_prev; i++) (void)rso_rand(&g);
    /* cqi-manager.cpp:105-123 with reporting interval 40; enb-mac-entity.cc:189-191 */
    if (!reported || ((int)(t * 1000) - last_sent) >= 40) {
      reported = true;
      last_sent = (long)(t * 1000);
      int stamp = (int)(t * 1000 / 40);
      int row = stamp % run->row_modulus;
      if (row >= run->n_rows) return -10;
      for (int u = 0; u < U; u++) {
        int tr = run->mapping[u % run->n_map];
        if (g_trace_per_prb) {
          /* the full report of enb-mac-entity.cc:173-186: every PRB; the metric reads PRB rbg*rbg_size */
          const int n = R * c->rbg_size;
          if (c->cqi_prb.empty()) c->cqi_prb.assign((size_t)U * n, 10);
          const uint8_t* rowp = run->trace + ((size_t)tr * run->n_rows + row) * n;
          memcpy(&c->cqi_prb[(size_t)u * n], rowp, n);
          for (int r = 0; r < R; r++) c->cqi[(size_t)u * R + r] = rowp[r * c->rbg_size];
        } else {
          rso_cell_set_user_cqi(c, u, run->trace + ((size_t)tr * run->n_rows + row) * R);
        }
      }
    }
    int r0 = 0, r1 = 0;
    if (uses_rand(c->sched)) { r0 = rso_rand(&g); r1 = rso_rand(&g); }
    int rc = c->sched == RSO_SCHED_NVS_NONGREEDY ? rso_cell_step_rng(c, t, &g, &out) : rso_cell_step(c, t, r0, r1, &out);
    if (rc) return rc;
    served_prev = 0;
    for (int u = 0; u < U; u++) served_prev += nprb[u] > 0;
    if (log_map) memcpy(log_map + (size_t)n * R, map.data(), sizeof(int) * R);
    if (log_fcqi) memcpy(log_fcqi + (size_t)n * U, fcqi.data(), sizeof(int) * U);
    if (log_quota) memcpy(log_quota + (size_t)n * S, quota.data(), sizeof(int) * S);
    if (log_target) memcpy(log_target + (size_t)n * S, target.data(), sizeof(int) * S);
    if (log_tbs) memcpy(log_tbs + (size_t)n * U, tbs.data(), sizeof(int) * U);
    t = clock_advance(t);
  }
  return 0;
}

static int run_synth_impl(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed,
                          int phy_error_draws, int n_ttis, int* log_map, int* log_tbs, bool per_prb);
int rso_run_synth(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed,
                  int phy_error_draws, int n_ttis, int* log_rbg_to_user, int* log_tbs_bits) {
  return run_synth_impl(c, cqi_epochs, n_epochs, refresh, seed, phy_error_draws, n_ttis, log_rbg_to_user, log_tbs_bits, false);
}
/* the same with per-PRB grids [n_epochs][U][R*rbg_size] (reports that differ inside an RBG) */
int rso_run_synth_prb(rso_cell* c, const uint8_t* cqi_prb_epochs, int n_epochs, int refresh, unsigned seed,
                      int phy_error_draws, int n_ttis, int* log_rbg_to_user, int* log_tbs_bits) {
  return run_synth_impl(c, cqi_prb_epochs, n_epochs, refresh, seed, phy_error_draws, n_ttis, log_rbg_to_user, log_tbs_bits, true);
}
static int run_synth_impl(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed,
                          int phy_error_draws, int n_ttis, int* log_map, int* log_tbs, bool per_prb) {
  const int S = c->S, U = c->U, R = c->R;
  rso_rng g;
  rso_srand(&g, seed);
  std::vector<int> target(S), quota(S), map(R), nprb(U), fcqi(U), mcs(U), tbs(U);
  rso_tti_out out = {target.data(), quota.data(), map.data(), nprb.data(), fcqi.data(), mcs.data(), tbs.data(), -1, nullptr, nullptr, nullptr, nullptr};
  double t = 0;
  for (int k = 0; k < 100; k++) t = clock_advance(t);
  rso_cell_set_last_update(c, 0.1);
  int served_prev = 0;
  for (int n = 0; n < n_ttis; n++) {
    if (phy_error_draws)
      for (int i = 0; i < served_prev; i++) (void)rso_rand(&g);
    if (n % refresh == 0) {
      int e = n / refresh;
      if (e >= n_epochs) return -10;
      if (per_prb) rso_cell_set_cqi_prb(c, cqi_epochs + (size_t)e * U * R * c->rbg_size);
      else rso_cell_set_cqi(c, cqi_epochs + (size_t)e * U * R);
    }
    int r0 = 0, r1 = 0;
    if (uses_rand(c->sched)) { r0 = rso_rand(&g); r1 = rso_rand(&g); }
    int rc = c->sched == RSO_SCHED_NVS_NONGREEDY ? rso_cell_step_rng(c, t, &g, &out) : rso_cell_step(c, t, r0, r1, &out);
    if (rc) return rc;
    served_prev = 0;
    for (int u = 0; u < U; u++) served_prev += nprb[u] > 0;
    if (log_map) memcpy(log_map + (size_t)n * R, map.data(), sizeof(int) * R);
    if (log_tbs) memcpy(log_tbs + (size_t)n * U, tbs.data(), sizeof(int) * U);
    t = clock_advance(t);
  }
  return 0;
}

/* bench.py's cpu_baseline leg: n_cells independent cells of one configuration, each with its own rand() stream, all reading the
 * same CQI epochs (read-only), spread over the host cores with OpenMP ("OpenMP over independent cells on all
 * host cores").  threads <= 0: the OpenMP default.  Returns 0 or the first failing cell's code; *threads_used = team size. */
int rso_run_synth_many(const rso_config* cfg, int n_cells, const uint8_t* cqi_epochs, int n_epochs, int refresh,
                       const unsigned* seeds, int phy_error_draws, int n_ttis, int threads, int64_t* total_bytes,
                       int* threads_used) {
  int rc_all = 0, used = 1;
  int64_t bytes = 0;
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bytes)
  for (int i = 0; i < n_cells; i++) {
    if (i == 0) used = omp_get_num_threads();
    rso_cell* c = rso_cell_create(cfg);
    int rc = rso_run_synth(c, cqi_epochs, n_epochs, refresh, seeds[i], phy_error_draws, n_ttis, nullptr, nullptr);
    if (rc) {
#pragma omp critical
      if (!rc_all) rc_all = rc;
    }
    for (int u = 0; u < c->U; u++) bytes += c->cum_bytes[u];
    rso_cell_destroy(c);
  }
  if (total_bytes) *total_bytes = bytes;
  if (threads_used) *threads_used = used;
  return rc_all;
}

/* bench.py's parity sample (round 6): the same, but every cell reads ITS OWN epochs (cqi_epochs [n_cells][n_epochs][U][R]: the grids the
 * GPU batch synthesised for those global cell ids, downloaded) and leaves its final state behind -- avg_rate [n_cells][U],
 * cum_bytes / cum_rbs [n_cells][U], slice_state [n_cells][S] (any may be NULL) -- so that the caller can compare cell by cell. */
int rso_run_synth_cells(const rso_config* cfg, int n_cells, const uint8_t* cqi_epochs, int n_epochs, int refresh, const unsigned* seeds,
                        int phy_error_draws, int n_ttis, int threads, double* avg_rate, int64_t* cum_bytes, int64_t* cum_rbs,
                        double* slice_state, int* threads_used) {
  int rc_all = 0, used = 1;
  if (threads > 0) omp_set_num_threads(threads);
#pragma omp parallel for schedule(dynamic, 1)
  for (int i = 0; i < n_cells; i++) {
    if (i == 0) used = omp_get_num_threads();
    rso_cell* c = rso_cell_create(cfg);
    const size_t U = (size_t)c->U, S = (size_t)c->S, grid = U * c->R;
    int rc = rso_run_synth(c, cqi_epochs + (size_t)i * n_epochs * grid, n_epochs, refresh, seeds[i], phy_error_draws, n_ttis, nullptr, nullptr);
    if (rc) {
#pragma omp critical
      if (!rc_all) rc_all = rc;
    }
    std::vector<double> a(U), sl(S);
    std::vector<int64_t> cb(U), cr(U);
    rso_cell_get_state(c, a.data(), cb.data(), cr.data(), sl.data());
    if (avg_rate) memcpy(avg_rate + i * U, a.data(), 8 * U);
    if (cum_bytes) memcpy(cum_bytes + i * U, cb.data(), 8 * U);
    if (cum_rbs) memcpy(cum_rbs + i * U, cr.data(), 8 * U);
    if (slice_state) memcpy(slice_state + i * S, sl.data(), 8 * S);
    rso_cell_destroy(c);
  }
  if (threads_used) *threads_used = used;
  return rc_all;
}


/* =====================================================================================
 * Finite queues: bearers with MAC queues, arrivals handed in as bursts.
 * Restated from flows/MacQueue.cpp (Enqueue :106-121, GetQueueSizeWithMACHoverhead :86-99, GetPacketToTramsit :123-200),
 * protocolStack/rlc/um-rlc-entity.cpp:126-196 (TransmissionProcedure of a queued bearer), flows/radio-bearer.cpp:281-308
 * (GetHeadOfLinePacketDelay), :344-367 (HasPackets), downlink-transport-scheduler.cpp:105-221 (SelectFlowsToSchedule,
 * DoSchedule, DoStopSchedule), packet-scheduler.cpp:305-335 (InsertFlowToUser), downlink-nvs-scheduler.cpp:94-273.
 * PARITY UNPINNED: no reference output exists for these paths in this image.
 * ===================================================================================== */

void rso_cell_enable_queues(rso_cell* c, const uint8_t* bearer_kind /* [U][2] */) {
  c->bearers.assign((size_t)c->U * 2, rso_cell::Bearer());
  for (size_t i = 0; i < c->bearers.size(); i++) c->bearers[i].kind = bearer_kind[i];
  c->active.assign(c->U, 0);
  c->avgsum.assign(c->U, 1);
  c->data_tx.assign((size_t)c->U * 2, 0);
  c->required_rbs.assign(c->U, 0);
  c->hol.assign(c->U, 0);
  c->prio_has_data.assign(c->U, 0);
}

/* every bearer's average rate from outside, [U][2] (after rso_cell_enable_queues; a test that starts the queue model from chosen averages) */
void rso_cell_set_bearer_avg(rso_cell* c, const double* avg /* [U][2] */) {
  for (size_t i = 0; i < c->bearers.size(); i++) c->bearers[i].avg = avg[i];
}

void rso_cell_set_arrivals(rso_cell* c, int user, int prio, int n, const double* time, const int32_t* n_full, const int32_t* last) {
  rso_cell::Bearer& b = c->bearers[(size_t)user * 2 + prio];
  b.arr_time.assign(time, time + n);
  b.arr_nfull.assign(n_full, n_full + n);
  b.arr_last.assign(last, last + n);
  b.next_arr = 0;
}

void rso_cell_get_bearer_state(const rso_cell* c, double* avg, int64_t* cum_bytes, int64_t* cum_rbs, int32_t* queue_bytes,
                               int32_t* queue_packets) {
  for (size_t i = 0; i < c->bearers.size(); i++) {
    if (avg) avg[i] = c->bearers[i].avg;
    if (cum_bytes) cum_bytes[i] = c->bearers[i].cum_bytes;
    if (cum_rbs) cum_rbs[i] = c->bearers[i].cum_rbs;
    if (queue_bytes) queue_bytes[i] = c->bearers[i].queue_size;
    if (queue_packets) queue_packets[i] = c->bearers[i].n_packets;
  }
}

static void queue_dequeue(rso_cell::Bearer& b, int available) {
  /* UmRlcEntity::TransmissionProcedure, queued bearer (um-rlc-entity.cpp:126-196): packets leave the MAC queue one by one,
   * each costing its data + 8 bytes of RLC/MAC/CRC overhead; the last one may be a fragment */
  while (available > 0 && !b.q.empty()) {
    const int overhead = 8;
    if (overhead >= available) break; /* GetPacketToTramsit returns NULL: availableBytes = 0 */
    rso_cell::Packet& head = b.q.front();
    const int data = head.size - head.frag_off; /* a fragment continues at its offset; a fresh packet has offset 0 */
    if (data + overhead > available) {
      const int frag = available - overhead;
      head.frag_off += frag;
      b.queue_size -= frag;
      available -= frag + overhead;
    } else {
      b.queue_size -= data;
      b.n_packets -= 1;
      b.q.pop_front();
      available -= data + overhead;
    }
  }
}

/* DownlinkPacketScheduler::RBsAllocation on FLOWS (sched 1 with finite queues; downlink-packet-scheduler.cpp:179-331,
 * dl-pf-packet-scheduler.cpp:60-140): a flow = a bearer with packets, in RRC container order (user ascending, bearer index
 * ascending); metric (se * 180000.) / the bearer's own average; a flow leaves the competition once the transport block of
 * its PRBs so far carries its whole queue (:253-265).  DoStopSchedule credits the whole block to the flow and hands it to
 * the RLC.  rbg_to_user reports the flow id 2 * user + bearer. */
static int step_pf_flows(rso_cell* c, rso_tti_out* out) {
  const int U = c->U, R = c->R, G = c->rbg_size;
  std::vector<int> flows;
  for (int u = 0; u < U; u++)
    for (int b = 0; b < 2; b++)
      if (c->data_tx[(size_t)u * 2 + b] > 0) flows.push_back(u * 2 + b);
  const int F = (int)flows.size();
  if (F == 0) return 0;
  std::vector<char> done(F, 0);
  std::vector<std::vector<uint8_t>> prbs(F);
  int n_done = 0;
  for (int r = 0; r < R; r++) {
    if (n_done == F) break;
    double target = 0;
    int pick = -1;
    for (int k = 0; k < F; k++) {
      const int u = flows[k] >> 1;
      double se = c->eff_of_cqi[c->cqi[(size_t)u * R + r]];
      double metric = (se * 180000.) / c->bearers[flows[k]].avg;
      if (metric > target && !done[k]) { target = metric; pick = k; }
    }
    if (pick < 0) continue;
    out->rbg_to_user[r] = flows[pick];
    for (int k = 0; k < G; k++) prbs[pick].push_back(prb_cqi(c, flows[pick] >> 1, r, k));
    int fc = rso_final_cqi(prbs[pick].data(), (int)prbs[pick].size());
    int tbs = rso_tbs_bits(kCqiToMcs[fc - 1], (int)prbs[pick].size());
    if (tbs >= c->data_tx[flows[pick]] * 8) { done[pick] = 1; n_done++; }
  }
  for (int k = 0; k < F; k++) {
    if (prbs[k].empty()) continue;
    const int u = flows[k] >> 1;
    int fc = rso_final_cqi(prbs[k].data(), (int)prbs[k].size());
    int mcs = kCqiToMcs[fc - 1];
    int tbs = rso_tbs_bits(mcs, (int)prbs[k].size());
    out->user_nprb[u] += (int)prbs[k].size();
    out->user_final_cqi[u] = fc;
    out->user_mcs[u] = mcs;
    out->user_tbs_bits[u] += tbs;
    /* DL_PF_PacketScheduler::DoStopSchedule (dl-pf-packet-scheduler.cpp:60-125) */
    int available = tbs / 8;
    if (available > 0) {
      rso_cell::Bearer& br = c->bearers[flows[k]];
      br.tx_bytes += available;
      br.cum_bytes += available;
      br.cum_rbs += (int)prbs[k].size();
      if (br.kind == 2) queue_dequeue(br, available);
    }
  }
  return 0;
}

int rso_cell_step_queues(rso_cell* c, double now, rso_rng* g, rso_tti_out* out) {
  if (c->bearers.empty()) return -20;
  if (c->sched == RSO_SCHED_NVS_NONGREEDY || c->sched == RSO_SCHED_UPPERBOUND) return -21; /* not restated with queues */
  const int U = c->U, S = c->S;
  /* events with a time stamp before this TTI's: the applications' Send() calls (MacQueue::Enqueue per packet) */
  for (rso_cell::Bearer& b : c->bearers)
    while (b.kind == 2 && b.next_arr < b.arr_time.size() && b.arr_time[b.next_arr] <= now) {
      const double ts = b.arr_time[b.next_arr];
      for (int k = 0; k < b.arr_nfull[b.next_arr]; k++) { b.q.push_back({RSO_FULL_PACKET, ts, 0}); b.queue_size += RSO_FULL_PACKET; b.n_packets++; }
      if (b.arr_last[b.next_arr] > 0) { b.q.push_back({b.arr_last[b.next_arr], ts, 0}); b.queue_size += b.arr_last[b.next_arr]; b.n_packets++; }
      b.next_arr++;
    }
  /* UpdateAverageTransmissionRate: every bearer of the RRC container (radio-bearer.cpp:139-164) */
  for (rso_cell::Bearer& b : c->bearers) {
    if (b.kind == 0 || now == b.last_update) continue;
    double rate = (b.tx_bytes * 8) / (now - b.last_update);
    double beta = 0.02;
    b.avg = ((1 - beta) * b.avg) + (beta * rate);
    if (b.avg < 1) b.avg = 1;
    b.tx_bytes = 0;
    b.last_update = now;
  }
  /* SelectFlowsToSchedule + InsertFlowToUser: the users' records */
  std::vector<int> slice_priority(S, 0);
  int n_active = 0;
  for (int u = 0; u < U; u++) {
    c->active[u] = 0;
    double sum = 1;
    for (int b = 0; b < 2; b++) {
      rso_cell::Bearer& br = c->bearers[(size_t)u * 2 + b];
      const bool has = br.kind == 1 || (br.kind == 2 && !br.q.empty());
      int data = 0;
      if (has) {
        data = br.kind == 1 ? 100000000 : br.queue_size + br.n_packets * 8; /* GetQueueSizeWithMACHoverhead */
        c->active[u] = 1;
        sum += br.avg;
        if (b > slice_priority[c->u2s[u]]) slice_priority[c->u2s[u]] = b;
      }
      c->data_tx[(size_t)u * 2 + b] = data;
    }
    c->avgsum[u] = sum;
    n_active += c->active[u];
  }
  for (int u = 0; u < U; u++) {
    const int p = slice_priority[c->u2s[u]];
    const rso_cell::Bearer& br = c->bearers[(size_t)u * 2 + p];
    c->prio_has_data[u] = c->data_tx[(size_t)u * 2 + p] != 0;
    /* GetHeadOfLinePacketDelay (radio-bearer.cpp:281-308): 0 with an empty MAC queue, else now - head time stamp, >= 1e-5 */
    double HOL = 0.;
    if (br.kind != 0 && br.queue_size != 0) {
      HOL = now - br.q.front().ts;
      if (HOL < 0.00001) HOL = 0.00001;
    }
    c->hol[u] = HOL;
  }
  for (int s = 0; s < S; s++) { out->target_rbs[s] = 0; out->quota_rbgs[s] = 0; }
  for (int r = 0; r < c->R; r++) out->rbg_to_user[r] = -1;
  for (int u = 0; u < U; u++) { out->user_nprb[u] = 0; out->user_final_cqi[u] = 0; out->user_mcs[u] = 0; out->user_tbs_bits[u] = 0; }
  out->served_slice = -1;
  int rc = 0;
  if (c->sched == RSO_SCHED_PF) return step_pf_flows(c, out); /* incl. its own DoStopSchedule */
  if (c->sched == RSO_SCHED_NVS) {
    /* downlink-nvs-scheduler.cpp:196-218: the slice is chosen before anything else; users = the slice's bearers with packets */
    const int slice = nvs_select_slice(c);
    int in_slice = 0;
    for (int u = 0; u < U; u++) {
      if (c->u2s[u] != slice) c->active[u] = 0;
      in_slice += c->active[u];
    }
    if (in_slice) rc = allocate_nvs(c, c->avg.data(), slice, out);
    out->served_slice = slice;
  } else if (n_active) {
    /* RBsAllocation runs -- and draws its two rand() values -- only when some user has queued data (:160-165) */
    const int rand0 = rso_rand(g), rand1 = rso_rand(g);
    rc = allocate_transport(c, c->avg.data(), rand0, rand1, out, true);
  }
  if (rc) return rc;
  /* DoStopSchedule (:170-221 / nvs :220-273): the grant goes to the user's bearers from the highest priority down */
  for (int u = 0; u < U; u++) {
    if (!c->active[u]) continue;
    int available = out->user_tbs_bits[u] / 8;
    for (int i = 1; i >= 0; i--) {
      if (available <= 0) break;
      const int data = c->data_tx[(size_t)u * 2 + i];
      if (data > 0) {
        rso_cell::Bearer& br = c->bearers[(size_t)u * 2 + i];
        const int sent = std::min(available, data);
        available -= sent;
        br.tx_bytes += sent;
        br.cum_bytes += sent;
        br.cum_rbs += out->user_nprb[u];
        if (br.kind == 2) queue_dequeue(br, sent);
      }
    }
  }
  return 0;
}

/* queue-mode run on synthetic grids: the clock, the CQI refresh and the rand() coupling of rso_run_synth; per_prb: the grids
 * hold one CQI per PRB ([U][R*G] per epoch; the metric reads each RBG's first PRB, link adaptation, m_requiredRBs and the
 * satisfied-flow break every PRB) */
static int run_synth_queues_impl(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed, int n_ttis,
                                 int* log_rbg_to_user, int* log_tbs_bits, bool per_prb);
int rso_run_synth_queues(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed, int n_ttis,
                         int* log_rbg_to_user, int* log_tbs_bits) {
  return run_synth_queues_impl(c, cqi_epochs, n_epochs, refresh, seed, n_ttis, log_rbg_to_user, log_tbs_bits, false);
}
int rso_run_synth_queues_prb(rso_cell* c, const uint8_t* cqi_prb_epochs, int n_epochs, int refresh, unsigned seed, int n_ttis,
                             int* log_rbg_to_user, int* log_tbs_bits) {
  return run_synth_queues_impl(c, cqi_prb_epochs, n_epochs, refresh, seed, n_ttis, log_rbg_to_user, log_tbs_bits, true);
}
static int run_synth_queues_impl(rso_cell* c, const uint8_t* cqi_epochs, int n_epochs, int refresh, unsigned seed, int n_ttis,
                                 int* log_rbg_to_user, int* log_tbs_bits, bool per_prb) {
  const int S = c->S, U = c->U, R = c->R;
  rso_rng g;
  rso_srand(&g, seed);
  std::vector<int> target(S), quota(S), map(R), nprb(U), fcqi(U), mcs(U), tbs(U);
  rso_tti_out out = {target.data(), quota.data(), map.data(), nprb.data(), fcqi.data(), mcs.data(), tbs.data(), -1, nullptr, nullptr, nullptr, nullptr};
  double t = 0;
  for (int k = 0; k < 100; k++) t = clock_advance(t);
  for (int n = 0; n < n_ttis; n++) {
    if (n % refresh == 0) {
      int e = n / refresh;
      if (e >= n_epochs) return -10;
      if (per_prb) rso_cell_set_cqi_prb(c, cqi_epochs + (size_t)e * U * R * c->rbg_size);
      else rso_cell_set_cqi(c, cqi_epochs + (size_t)e * U * R);
    }
    int rc = rso_cell_step_queues(c, t, &g, &out);
    if (rc) return rc;
    if (log_rbg_to_user) memcpy(log_rbg_to_user + (size_t)n * R, map.data(), sizeof(int) * R);
    if (log_tbs_bits) memcpy(log_tbs_bits + (size_t)n * U, tbs.data(), sizeof(int) * U);
    t = clock_advance(t);
  }
  return 0;
}

}  // extern "C"
