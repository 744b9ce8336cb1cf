/*
 * rs_api.cpp -- host side of the C ABI declared in include/radiosaber_hip.h.
 *
 * Validates configurations, owns the device buffers (cell state, CQI grids, traces), evaluates the
 * link-adaptation tables with the host libm (the only place transcendental functions run), seeds the
 * per-cell libc-compatible rand() streams and launches the gfx950 kernels of rs_kernels.hip.
 * There is no CPU implementation of the scheduling path here: without a HIP device every compute
 * entry point fails with RS_ERR_NO_DEVICE.
 *
 * Build with -ffp-contract=off (the table arithmetic must round like the reference's -O0 SSE2 code).
 */
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <thread>
#include <fstream>
#include <vector>

#include "../../include/radiosaber_hip.h"
#include "rs_amc_tables.inc"
#include "rs_link_pinned.inc"
#include "rs_host.h"
#include "rs_devmem.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess) return fail(RS_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e__));   \
  } while (0)

/* scratch device buffers / events of one call: released on every return path */
struct ScratchBuffers {
  std::vector<void*> ptrs;
  ~ScratchBuffers() { for (void* q : ptrs) (void)hipFree(q); }
  template <typename T> hipError_t alloc(T** out, size_t bytes) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes ? bytes : 1);
    if (e == hipSuccess) { ptrs.push_back(q); *out = (T*)q; }
    return e;
  }
};
struct ScratchEvents {
  std::vector<hipEvent_t> ev;
  ~ScratchEvents() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  hipError_t create(int n) {
    for (int i = 0; i < n; i++) {
      hipEvent_t e = nullptr;
      hipError_t rc = hipEventCreate(&e);
      if (rc != hipSuccess) return rc;
      ev.push_back(e);
    }
    return hipSuccess;
  }
};

const int kCqiToMcs[15] = {RS_AMC_CQI_TO_MCS};
const double kSinrForCqi[15] = {RS_AMC_SINR_FOR_CQI};
const int kMcsToItbs[29] = {RS_AMC_MCS_TO_ITBS};
const int kTbs[110][27] = {RS_AMC_TBS_TABLE};

/* the reference's effective-SINR expression on x = mean(exp(-sinr_lin))
 * (src/utility/eesm-effective-sinr.h:43-44 with beta = 1) */
double eesm_db_of_mean(double x) {
  double beta = 1;
  double eff = -beta * log(x);
  eff = 10 * log10(eff);
  return eff;
}

double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
uint64_t to_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

/* glibc TYPE_3 rand() (glibc 2.35 stdlib/random_r.c), host copy used to seed the device rings */
struct HostRng {
  uint32_t r[31];
  int f, b;
  void seed(unsigned s) {
    if (s == 0) s = 1;
    int32_t w = (int32_t)s;
    r[0] = (uint32_t)w;
    for (int i = 1; i < 31; i++) {
      long hi = w / 127773, lo = w % 127773;
      long word = 16807 * lo - 2836 * hi;
      if (word < 0) word += 2147483647;
      w = (int32_t)word;
      r[i] = (uint32_t)w;
    }
    f = 3;
    b = 0;
    for (int i = 0; i < 310; i++) next();
  }
  int next() {
    uint32_t v = r[f] += r[b];
    if (++f >= 31) f = 0;
    if (++b >= 31) b = 0;
    return (int)(v >> 1);
  }
};

int round_up(int x, int a) { return (x + a - 1) / a * a; }

}  // namespace

extern "C" {

const char* rs_last_error(void) { return g_err; }
int rs_abi_version(void) { return RS_ABI_VERSION; }

int rs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* ref: src/utility/eesm-effective-sinr.h:82-103 (the reference throws above 512 PRBs) */
int rs_get_rbg_size(int nb_rbs) {
  if (nb_rbs < 1) return fail(RS_ERR_INVALID, "nb_rbs %d < 1", nb_rbs);
  if (nb_rbs <= 10) return 1;
  if (nb_rbs <= 26) return 2;
  if (nb_rbs <= 63) return 3;
  if (nb_rbs <= 110) return 4;
  if (nb_rbs <= 512) return 8;
  return fail(RS_ERR_INVALID, "nb_rbs %d > 512: the reference's get_rbg_size throws", nb_rbs);
}

/* ref: src/core/spectrum/bandwidth-manager.cpp:30-38, 52-108: PRBs of a downlink bandwidth; any other value falls back to 5 MHz */
int rs_dl_prbs_for_bandwidth(double bw_mhz) {
  if (bw_mhz == 1.4) return 6;
  if (bw_mhz == 3) return 15;
  if (bw_mhz == 5) return 25;
  if (bw_mhz == 10) return 50;
  if (bw_mhz == 15) return 75;
  if (bw_mhz == 20) return 100;
  if (bw_mhz == 100) return 512;
  return 25;
}

/* the EESM constants as glibc 2.35 (x86-64) evaluates them: E[1..15], X[1..13] (radiosaber_amd/data/link_tables_glibc_2_35.json ->
 * rs_link_pinned.inc by build.py; the same hex values as SURVEY.md Appendix A / tests/golden/appendix_a.json) */
static const double kPinnedE[15] = {RS_LINK_PINNED_E};
static const double kPinnedX[13] = {RS_LINK_PINNED_X};

int rs_link_tables_pinned(double eff[16], double kbps[16], double eesm_e[16], double eesm_x[16]) {
  eff[0] = kbps[0] = eesm_e[0] = eesm_x[0] = 0;
  for (int c = 1; c <= 15; c++) {
    const int bits = kTbs[0][kMcsToItbs[kCqiToMcs[c - 1]]];
    const double e = (bits / 0.001) / 180000.; /* IEEE divisions of table integers: no libm */
    eff[c] = e;
    kbps[c] = e * 180000 / 1000;
    eesm_e[c] = kPinnedE[c - 1];
  }
  eesm_x[14] = eesm_x[15] = 0;
  for (int k = 1; k <= 13; k++) eesm_x[k] = kPinnedX[k - 1];
  return RS_OK;
}

int rs_link_tables_compare(char* msg, size_t msglen) {
  double eff[16], kbps[16], e[16], x[16];
  if (msg && msglen) msg[0] = 0;
  const int rc = rs_link_tables(eff, kbps, e, x);
  if (rc) return rc;
  int diff = 0;
  std::string text;
  char line[160];
  for (int c = 1; c <= 15; c++)
    if (to_bits(e[c]) != to_bits(kPinnedE[c - 1])) {
      diff++;
      snprintf(line, sizeof line, "E[%d] host %a pinned %a; ", c, e[c], kPinnedE[c - 1]);
      text += line;
    }
  for (int k = 1; k <= 13; k++)
    if (to_bits(x[k]) != to_bits(kPinnedX[k - 1])) {
      diff++;
      snprintf(line, sizeof line, "X[%d] host %a pinned %a; ", k, x[k], kPinnedX[k - 1]);
      text += line;
    }
  if (msg && msglen) snprintf(msg, msglen, "%s", text.c_str());
  return diff;
}

int rs_link_tables(double eff[16], double kbps[16], double eesm_e[16], double eesm_x[16]) {
  eff[0] = kbps[0] = eesm_e[0] = eesm_x[0] = 0;
  for (int c = 1; c <= 15; c++) {
    int bits = kTbs[0][kMcsToItbs[kCqiToMcs[c - 1]]];
    double e = (bits / 0.001) / 180000.; /* AMCModule.cpp:320-327 */
    eff[c] = e;
    kbps[c] = e * 180000 / 1000; /* downlink-transport-scheduler.cpp:688 */
    double s = pow(10, kSinrForCqi[c - 1] / 10);
    double beta = 1;
    eesm_e[c] = exp(-s / beta); /* eesm-effective-sinr.h:38-40 */
  }
  eesm_x[14] = eesm_x[15] = 0;
  for (int k = 1; k <= 13; k++) {
    /* largest positive double x with eesm_db_of_mean(x) >= SINR[k] (the function decreases in x) */
    const double thr = kSinrForCqi[k];
    uint64_t lo = 1, hi = to_bits(1.0) - 1; /* smallest subnormal .. largest double below 1 */
    if (!(eesm_db_of_mean(from_bits(lo)) >= thr)) return fail(RS_ERR_INVALID, "EESM threshold %d unreachable", k);
    while (hi - lo > 1) {
      uint64_t mid = lo + (hi - lo) / 2;
      if (eesm_db_of_mean(from_bits(mid)) >= thr) lo = mid; else hi = mid;
    }
    if (eesm_db_of_mean(from_bits(hi)) >= thr) lo = hi;
    /* the comparison on x is only equivalent to the reference's comparison in dB if the host
     * libm composite is monotone around the threshold: check a +-4096 ulp neighbourhood */
    for (int d = 1; d <= 4096; d++) {
      if (!(eesm_db_of_mean(from_bits(lo - d)) >= thr) || (eesm_db_of_mean(from_bits(lo + d)) >= thr))
        return fail(RS_ERR_INVALID, "host libm not monotone around EESM threshold %d (offset %d ulp)", k, d);
    }
    eesm_x[k] = from_bits(lo);
  }
  for (int k = 2; k <= 13; k++)
    if (!(eesm_x[k] < eesm_x[k - 1])) return fail(RS_ERR_INVALID, "EESM thresholds not decreasing at %d", k);
  return RS_OK;
}

}  // extern "C"

/* ===================================================================================== */

struct rs_batch {
  rs_batch_config cfg;
  std::vector<double> weight;
  std::vector<int32_t> eps, psi, u2s, alpha, beta;
  bool any_alpha = false;
  bool synthetic = false;    /* rs_config.synthetic_exp */
  bool gen_exp = false;      /* drop-in context with an exponent outside {0, 1} (ref: packet-scheduler.h:38-49 takes any int) */
  int S, U, R, G, sched, n_cells, threads;
  bool direct = false;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  /* Device memory: every array is a DevBuf (rs_devmem.h), which frees itself with the batch and knows its size -- a size is written
   * once, where the array is made (batch_alloc and the setters), and read from the buffer everywhere else. */
  DevBuf<double> d_gen_num; /* [S][16] pow(kbps[cqi], algo_epsilon[s]), host libm */
  DevBuf<int32_t> d_alpha, d_beta;
  DevBuf<RsTables> d_tab;
  DevBuf<double> d_weight;
  DevBuf<int32_t> d_eps, d_psi;
  DevBuf<uint8_t> d_user_slice;
  DevBuf<int32_t> d_tbs_eff;
  DevBuf<double> d_avg;           /* [cells][U], as d_tx, d_cumb, d_cumr */
  DevBuf<int32_t> d_tx;
  DevBuf<int64_t> d_cumb, d_cumr;
  DevBuf<double> d_sstate;        /* [cells][S] */
  DevBuf<RsCellScalars> d_scal;   /* [cells] */
  /* The CQI source: which kind the batch reads, its arrays and their numbers.  A setter validates on the host, clears the record,
   * allocates and fills, and names the mode last (cqi_replace): the old grids go before the new ones are asked for -- they are the
   * batch's largest allocation --, and a failure on the way leaves no source, never a mode whose arrays are missing. */
  struct CqiSource {
    int32_t mode = RS_CQI_NONE;
    DevBuf<uint8_t> epochs, epochs_prb, trace, trace_prb; /* epoch grids / trace tables; _prb: the per-PRB twins (link adaptation) */
    DevBuf<int32_t> user_trace;
    int64_t grid_stride = 0, grid_stride_prb = 0;
    int32_t n_epochs = 0, n_traces = 0, n_rows = 0, row_mod = 0;
    void clear() { *this = CqiSource(); } /* no source: the arrays released, the numbers zero */
  } cqi;
  DevBuf<unsigned long long> d_cqi_bad; /* rs_pack_cqi_kernel's error word: all ones, or the lowest source byte outside 1..15 << 8 | its value */
  bool cqi_bad_armed = false;           /* the word is all ones, or a pack has written it: nothing to clear ahead of the next pack */
  DevBuf<int32_t> d_err;
  DevBuf<uint64_t> d_slice_bytes;
  DevBuf<unsigned long long> d_stamps;
  /* finite queues (rs_batch_set_bearers / rs_batch_set_arrivals) */
  bool queues = false;
  int qmode = 2;             /* rs_carve's `queue` argument once the queue model is on: 2 = bearers' hot words in LDS when they fit, 3 = in HBM */
  DevBuf<uint8_t> d_bearer_kind;
  DevBuf<int64_t> d_arr_off;
  DevBuf<double> d_arr_time;
  DevBuf<int32_t> d_arr_nfull, d_arr_last;
  DevBuf<int32_t> d_qi;   /* 7 arrays [cells][2][U]: head, tail, pk, frag, bytes, pkts, tx (plane()) */
  DevBuf<double> d_bavg;  /* [cells][2][U] */
  DevBuf<int64_t> d_bcum; /* 2 arrays [cells][2][U]: bytes, rbs */
  DevBuf<uint8_t> d_qflags;
  DevBuf<double> d_qhol;
  /* the flow completion record, one entry per arrival burst (rs_batch_flow_record): output, not state -- not in a checkpoint */
  DevBuf<int32_t> d_flow_tti;
  DevBuf<double> d_flow_time;
  /* bearer records (rs_batch_run_records): [n_cells][cap] records, then n_cells count words; grows, never shrinks.  Output, not state. */
  DevBuf<char> d_recs;
  /* The run-time builds of the batch's kernel (owned by the process-wide cache), one record per build: the general build (batch_new;
   * replaced by the commits of rs_batch_set_cell_configs and rs_batch_set_bearers, reset_builds), its lean build, compiled at the
   * first launch that can use it (lean_kernel), and the records variants of the two (-DRS_JIT_RECORDS=1; rs_batch_run_grant_records),
   * compiled at the first records launch that would pick that build and checked with records on before they serve one
   * (selfcheck_records).  `checked`: the self-check is through with the build -- it passed, came with the mark, or was dropped. */
  enum Slot { kGeneral, kLean, kRecGeneral, kRecLean, kNumBuilds, kBuiltinRecords = kNumBuilds };
  struct Build { RsJitKernel* k = nullptr; bool tried = false, checked = false; };
  struct Builds {
    Build at[kNumBuilds];
    bool rejected = false;     /* the general build disagreed with the built-in kernels: dropped, they serve every launch */
    bool rec_rejected = false; /* the general records variant disagreed: the built-in kernels serve the records launches */
    bool checked = false;      /* the self-check of the plain builds: done (or it does not apply) */
    bool autotuned = false;    /* rs_batch_config.autotune: the candidates were timed (or the tuning does not apply) */
    /* what served the last launch that was no trial: kGeneral or kLean (an empty general slot: the built-in kernels), a records
     * variant, or the built-in kernels with grant records on (kBuiltinRecords) */
    int last = kGeneral;
  } builds;
  RsJitKernel* general() const { return builds.at[kGeneral].k; }
  char selfcheck_msg[160] = "";
  int autotune_n = 0;
  char autotune_msg[768] = "";
  DevBuf<unsigned long long> d_prio_sum; /* TTIs done by all cells of the running launch (the cells' issue-priority feedback) */
  bool jit_wanted = false;
  char jit_msg[512] = ""; /* why the shape-specialised kernel is not in use (empty: it is, or it was not asked for) */
  int64_t ttis_done = 0;
  /* per-cell configurations (rs_batch_set_cell_configs): every cell's own row of the four arrays above, on the host and
   * on the device; the launch block then points at the rows and says so (RsLaunch::cell_cfg).  Configuration, not state. */
  bool cell_cfg = false;
  bool ragged = false;                         /* some row of cc_u2s ends in RS_USER_ABSENT: cells of different user counts */
  std::vector<double> cc_weight;               /* [cells][S] */
  std::vector<int32_t> cc_eps, cc_psi, cc_u2s; /* [cells][S], [cells][S], [cells][U] */
  std::vector<int32_t> cc_users;               /* [cells]: the row's users before the absent suffix (U where there is none) */
  bool ragged_slices = false;                  /* some cell has fewer slices than the batch (rs_batch_set_cell_configs_n) */
  std::vector<int32_t> cc_slices;              /* [cells]: the cell's slice count S_c (S where none was given) */
  DevBuf<double> d_cc_weight;
  DevBuf<int32_t> d_cc_eps, d_cc_psi;
  DevBuf<uint8_t> d_cc_user_slice;
  DevBuf<long long> d_totals;                  /* rs_batch_slice_totals: [2][cells][S] */
  RsLaunch base{};
};

namespace {

int validate(const rs_config* c, bool direct) {
  if (!c) return fail(RS_ERR_INVALID, "null config");
  if (c->n_slices < 1 || c->n_slices > RS_MAX_SLICES) return fail(RS_ERR_INVALID, "n_slices %d outside 1..%d", c->n_slices, RS_MAX_SLICES);
  if (c->n_users < 1 || c->n_users > RS_MAX_USERS) return fail(RS_ERR_INVALID, "n_users %d outside 1..%d", c->n_users, RS_MAX_USERS);
  if (c->n_rbgs < 1 || c->n_rbgs > RS_MAX_RBGS) return fail(RS_ERR_INVALID, "n_rbgs %d outside 1..%d", c->n_rbgs, RS_MAX_RBGS);
  if (c->rbg_size < 1 || c->rbg_size > 8) return fail(RS_ERR_INVALID, "rbg_size %d outside 1..8", c->rbg_size);
  if (c->n_rbgs * c->rbg_size > 512) return fail(RS_ERR_INVALID, "more than 512 PRBs (reference get_rbg_size throws)");
  if ((c->synthetic_exp | 1) != 1) return fail(RS_ERR_INVALID, "synthetic_exp %d is not 0 or 1 (an rs_config of an older ABI? it gained the field in ABI 8)", c->synthetic_exp);
  if (c->link_tables < RS_LINK_DEFAULT || c->link_tables > RS_LINK_PINNED_GLIBC_2_35)
    return fail(RS_ERR_INVALID, "link_tables %d is not an RS_LINK_* value (an rs_config of an older ABI? it gained the field in ABI 11)", c->link_tables);
  if (c->sched != RS_SCHED_PF && c->sched != RS_SCHED_NVS && c->sched != RS_SCHED_SEQUENTIAL && c->sched != RS_SCHED_MAXCELL &&
      c->sched != RS_SCHED_VOGEL && c->sched != RS_SCHED_SUBOPT && c->sched != RS_SCHED_UPPERBOUND && c->sched != RS_SCHED_NVS_NONGREEDY)
    return fail(RS_ERR_INVALID, "sched %d not supported (1, 7, 8, 9, 10, 11, 101, 103)", c->sched);
  if (!c->slice_weight || !c->algo_alpha || !c->algo_epsilon || !c->algo_psi || !c->user_to_slice)
    return fail(RS_ERR_INVALID, "null slice/user array");
  for (int s = 0; s < c->n_slices; s++) {
    if ((c->algo_alpha[s] | 1) != 1 || (c->algo_alpha[s] && (!c->algo_beta || (c->algo_beta[s] | 1) != 1)))
      return fail(RS_ERR_INVALID, "slice %d: algo_alpha/algo_beta must be 0 or 1", s);
    /* batches update the PF averages on the device, which has no pow(): exponents 0 and 1 (exact in libm) only; a drop-in context
     * takes any integers -- the host's libm raises the 16 numerators per slice once and every user's denominator per call */
    if (!direct && ((c->algo_epsilon[s] | 1) != 1 || (c->algo_psi[s] | 1) != 1))
      return fail(RS_ERR_INVALID, "slice %d: algo_epsilon/algo_psi must be 0 or 1 in a batch (any integer in a drop-in context)", s);
    if (c->algo_epsilon[s] < -64 || c->algo_epsilon[s] > 64 || c->algo_psi[s] < -64 || c->algo_psi[s] > 64)
      return fail(RS_ERR_INVALID, "slice %d: algo_epsilon/algo_psi outside -64..64", s);
  }
  for (int u = 0; u < c->n_users; u++) {
    int s = c->user_to_slice[u];
    if (s < 0 || s >= c->n_slices) return fail(RS_ERR_INVALID, "user %d: slice %d out of range", u, s);
    if (u && s < c->user_to_slice[u - 1]) return fail(RS_ERR_INVALID, "user_to_slice must be non-decreasing (user %d)", u);
  }
  return RS_OK;
}

int upad_of(int U) { return rs_upad_of(U); }

/* the longest slice window of the batch in the stage-1 reciprocal array: 8-aligned start of the slice's first user to the
 * 8-aligned end behind its last (a compile-time constant of the shape-specialised kernel, RS_JIT_WIN) */
int map_window(const int32_t* u2s, int U) {
  int win = 0;
  for (int u = 0; u < U && u2s[u] != RS_USER_ABSENT;) { /* (a ragged batch's row: the absent suffix is in no window) */
    int e = u;
    while (e < U && u2s[e] == u2s[u]) e++;
    const int w = ((e + 7) & ~7) - (u & ~7);
    win = w > win ? w : win;
    u = e;
  }
  return win;
}
/* (a batch with per-cell maps: the longest window over all its cells -- one kernel serves them all) */
int slice_window(const rs_batch* b) {
  if (!b->cell_cfg) return map_window(b->u2s.data(), b->U);
  int win = 0;
  for (int c = 0; c < b->n_cells; c++) win = std::max(win, map_window(b->cc_u2s.data() + (size_t)c * b->U, b->U));
  return win;
}
/* the per-cell reads of the load phase are a compile-time switch of a batch's run-time builds (-DRS_JIT_CELL_CONFIGS=<word>), named only
 * by a batch that has per-cell rows -- every other batch's option lists are what they were.  The word is RsLaunch::cell_cfg: 1 rows,
 * 2 rows with absent users, | 4 some cell of fewer slices than the batch */
int cell_cfg_word(bool absent_users, bool fewer_slices) { return (absent_users ? RS_CELL_CFG_RAGGED : 1) | (fewer_slices ? RS_CELL_CFG_SLICES : 0); }

/* The one place a batch asks for a run-time build: `slot` says which (lean bit, records variant), `extra` adds an autotune candidate's
 * options.  The arguments are the cache's key, so every call of a batch spells them the same way: the queue mode, the slice window, the
 * streamed bit (cqi_refresh <= 4), and the variant string -- extra, -DRS_JIT_RECORDS=1, the per-cell switch, in this order; nullptr for
 * the empty list (the key names a variant only where there is one).  A setter that builds BEFORE it commits names what the batch is
 * about to have (BuildAs); -1: what it has. */
struct BuildAs { int qmode = -1, win = -1, cell_cfg = -1; };
RsJitKernel* batch_build(const rs_batch* b, int slot, char* msg, size_t msglen, const char* extra = nullptr, const BuildAs& as = BuildAs()) {
  const bool lean = slot == rs_batch::kLean || slot == rs_batch::kRecLean, records = slot >= rs_batch::kRecGeneral;
  const int cfg_word = as.cell_cfg >= 0 ? as.cell_cfg : (b->cell_cfg ? cell_cfg_word(b->ragged, b->ragged_slices) : 0);
  std::string v = extra ? extra : "";
  if (records) v += std::string(v.empty() ? "" : " ") + "-DRS_JIT_RECORDS=1";
  if (cfg_word) v += std::string(v.empty() ? "" : " ") + "-DRS_JIT_CELL_CONFIGS=" + std::to_string(cfg_word);
  const RsJitSpec spec = {.S = b->S, .U = b->U, .R = b->R, .G = b->G, .NT = b->threads, .sched = b->sched,
                          .qmode = as.qmode >= 0 ? as.qmode : (b->queues ? b->qmode : 0),
                          .win = as.win >= 0 ? as.win : slice_window(b),
                          .flags = (b->cfg.cqi_refresh <= 4 ? 2 : 0) | (lean ? 4 : 0),
                          .variant = v.empty() ? nullptr : v.c_str()};
  return rs_jit_get(b->cfg.cell.device, spec, msg, msglen);
}
/* A new general build and its message (nullptr: the built-in kernels run, rs_batch_jit_status says why); everything that belonged to
 * the old one starts over -- the lean build, the records variants, the self-check and the autotune with their messages. */
void reset_builds(rs_batch* b, RsJitKernel* general, const char* msg) {
  b->builds = rs_batch::Builds();
  b->builds.at[rs_batch::kGeneral].k = general;
  b->builds.at[rs_batch::kGeneral].tried = true;
  b->selfcheck_msg[0] = 0;
  b->autotune_n = 0;
  b->autotune_msg[0] = 0;
  snprintf(b->jit_msg, sizeof b->jit_msg, "%s", msg);
}

void carve_lds(rs_batch* b, RsLaunch* L) {
  /* (drop-in contexts of schedulers 1 and 7 carry the gate scratch too: rs_tti_in.required_rbs / data_to_transmit) */
  const bool gate_scratch = b->direct && (b->sched == RS_SCHED_PF || b->sched == RS_SCHED_NVS);
  /* the same arguments the batch's shape-specialised kernels are compiled with (rs_jit_get: slice_window() for batches, 0 for
   * drop-in contexts); a batch that runs the built-in kernels splits NVS slices earlier (RS_NVS_WHOLE_SLICE_BUILTIN) */
  const RsCarve c = rs_carve(b->S, b->U, b->R, b->sched, b->threads, b->queues ? b->qmode : (gate_scratch ? 1 : 0),
                             b->direct ? 0 : slice_window(b), (b->jit_wanted || b->direct) ? RS_NVS_WHOLE_SLICE : RS_NVS_WHOLE_SLICE_BUILTIN);
  L->Upad = c.Upad;
  L->nvs_seg = c.nvs_seg;
  L->off_avgk = c.off_avgk; L->off_rcp = c.off_rcp; L->off_tab = c.off_tab; L->off_slice = c.off_slice;
  L->off_tx = c.off_tx; L->off_misc = c.off_misc; L->off_tbs = c.off_tbs; L->off_elems = c.off_elems;
  L->off_sorted = c.off_sorted; L->off_items = c.off_items; L->off_sortx = c.off_sortx; L->off_cqi = c.off_cqi;
  L->off_queue = c.off_queue;
  L->off_qstate = c.off_qstate;
  L->q_lds = c.q_lds;
  L->lds_bytes = c.lds_bytes;
  L->n_seg = c.n_seg;
  L->n_items = c.n_items;
}

int init_scalars(rs_batch* b, const uint32_t* seed, const int64_t* skip) {
  std::vector<RsCellScalars> sc(b->n_cells);
  double t = 0;
  for (int k = 0; k < b->cfg.first_tti; k++) t += 0.001; /* simulator.cc:117-126 */
  for (int c = 0; c < b->n_cells; c++) {
    RsCellScalars& s = sc[c];
    memset(&s, 0, sizeof s);
    s.t = t;
    s.last_update = 0.1; /* bearers are created by the application start event at 0.1 s */
    HostRng g;
    g.seed(seed ? seed[c] : 1u);
    if (skip)
      for (int64_t i = 0; i < skip[c]; i++) g.next();
    memcpy(s.rng_r, g.r, sizeof g.r);
    s.rng_f = g.f;
    s.rng_b = g.b;
  }
  HIP_TRY(b->d_scal.upload(sc.data()));
  return RS_OK;
}
/* the cells' scalar records as the device holds them now (the caller has waited for the stream) */
int read_scalars(const rs_batch* b, std::vector<RsCellScalars>* sc) {
  sc->resize(b->d_scal.count());
  HIP_TRY(b->d_scal.download(sc->data()));
  return RS_OK;
}

/* the device's compute units; 256 (an MI355X) where the runtime does not say */
int device_cus(int device) {
  hipDeviceProp_t prop;
  return hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
}

/* the k-th [cells][2][U] array of a queue-model block that holds several (d_qi, d_bcum): each is as long as d_bavg, which holds one */
template <typename T>
T* plane(const rs_batch* b, const DevBuf<T>& block, int k) { return block.get() + (size_t)k * b->d_bavg.count(); }

/* The one sequence of the six CQI setters (rs_batch::CqiSource).  A setter has validated its arguments on the host.  Then: the old
 * source goes, whatever its kind; `fill` allocates the new arrays and writes them and their numbers; the mode is named last.  Any
 * failure of `fill` clears again: the batch has no source and launch() refuses with "no CQI source set". */
template <typename Fill>
int cqi_replace(rs_batch* b, int32_t mode, Fill fill) {
  b->cqi.clear();
  const int rc = fill(b->cqi);
  if (rc) b->cqi.clear();
  else b->cqi.mode = mode;
  return rc;
}

int batch_alloc(rs_batch* b) {
  const size_t cells = b->n_cells, U = b->U, S = b->S;
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  if (b->cfg.cell.stream) {
    b->stream = (hipStream_t)b->cfg.cell.stream;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    b->own_stream = true;
  }
  RsTables t;
  memset(&t, 0, sizeof t);
  double eff[16];
  /* the EESM constants: pinned (glibc 2.35) for batches, this host's libm for a drop-in beside a locally built reference, unless the
   * configuration says otherwise (rs_config.link_tables) */
  const int link = b->cfg.cell.link_tables != RS_LINK_DEFAULT ? b->cfg.cell.link_tables : (b->direct ? RS_LINK_HOST_LIBM : RS_LINK_PINNED_GLIBC_2_35);
  int rc = link == RS_LINK_PINNED_GLIBC_2_35 ? rs_link_tables_pinned(eff, t.kbps, t.eesm_e, t.eesm_x) : rs_link_tables(eff, t.kbps, t.eesm_e, t.eesm_x);
  if (rc) return rc;
  for (int c = 1; c <= 15; c++) {
    t.pfnum[c] = eff[c] * 180000.; /* dl-pf-packet-scheduler.cpp:138 */
    t.eff[c] = eff[c];
    t.mcs_of_cqi[c] = kCqiToMcs[c - 1];
    t.itbs_of_cqi[c] = kMcsToItbs[kCqiToMcs[c - 1]];
    t.tbs1_of_cqi[c] = kTbs[0][kMcsToItbs[kCqiToMcs[c - 1]]];
    /* ref: downlink-transport-scheduler.cpp:643-658 with AMCModule.cpp:253-268: the PRB's SINR is the table value of its CQI, and
     * the CQI read back from it counts the thresholds at or below it */
    int rt = 1;
    while (rt <= 14 && kSinrForCqi[rt] <= kSinrForCqi[c - 1]) rt++;
    t.tbs1_syn[c] = kTbs[0][kMcsToItbs[kCqiToMcs[rt - 1]]];
  }
  /* AMCModule.cpp:313-315 reads TransportBlockSizeTable[-1][itbs] when nbRBs > 110 and nbRBs % 5 == 0.
   * In the as-shipped -O0 build McsToItbs[29] sits 128 bytes in front of the table, so
   * T[-1][i] = McsToItbs[5+i] for i <= 23 and 0 (padding) beyond. */
  for (int i = 0; i < 27; i++) t.tbs_row_m1[i] = i <= 23 ? kMcsToItbs[5 + i] : 0;
  HIP_TRY(b->d_tab.assign(&t, 1));
  HIP_TRY(b->d_weight.assign(b->weight.data(), S));
  HIP_TRY(b->d_eps.assign(b->eps.data(), S));
  HIP_TRY(b->d_psi.assign(b->psi.data(), S));
  HIP_TRY(b->d_alpha.assign(b->alpha.data(), S));
  HIP_TRY(b->d_beta.assign(b->beta.data(), S));
  std::vector<uint8_t> us(U);
  for (size_t u = 0; u < U; u++) us[u] = (uint8_t)b->u2s[u];
  HIP_TRY(b->d_user_slice.assign(us.data(), U));
  {
    /* TBS bits of n RBGs = n*G PRBs per itbs (AMCModule.cpp:306-317); row 0 unused.  The device gets them with the CQI -> MCS -> I_TBS
     * step folded in, [R+1][16] indexed by final CQI: the kernel's LDS table is then a straight copy (round 6: the two dependent loads
     * per entry -- itbs_of_cqi, then the row -- were ~1 us of every one-TTI launch) */
    std::vector<int32_t> te((size_t)(b->R + 1) * 27, 0);
    for (int n = 1; n <= b->R; n++)
      for (int i = 0; i < 27; i++) {
        const int nprb = n * b->G;
        int v;
        if (nprb <= 110) v = kTbs[nprb - 1][i];
        else v = 5 * kTbs[nprb / 5 - 1][i] + (nprb % 5 == 0 ? t.tbs_row_m1[i] : kTbs[nprb % 5 - 1][i]);
        te[(size_t)n * 27 + i] = v;
      }
    for (int32_t v : te)
      if (v / 8 > RS_MAX_BYTES_PER_TTI) return fail(RS_ERR_INVALID, "a transport block of %d bits does not fit the per-launch byte counters", v);
    std::vector<int32_t> te16((size_t)(b->R + 1) * 16, 0);
    for (int n = 0; n <= b->R; n++)
      for (int c = 0; c < 16; c++) te16[(size_t)n * 16 + c] = te[(size_t)n * 27 + t.itbs_of_cqi[c]];
    HIP_TRY(b->d_tbs_eff.assign(te16.data(), te16.size()));
  }
  if (b->gen_exp) {
    /* ref: downlink-transport-scheduler.cpp:688-693  pow(spectralEfficiency * 180000 / 1000, epsilon), with this host's libm --
     * the library the reference itself calls */
    std::vector<double> gn((size_t)S * 16, 0.0);
    for (size_t s = 0; s < S; s++)
      for (int c = 1; c <= 15; c++) gn[s * 16 + c] = pow(t.kbps[c], b->eps[s]);
    HIP_TRY(b->d_gen_num.assign(gn.data(), gn.size()));
  }
  const std::vector<double> avg(cells * U, 100000.0); /* radio-bearer.cpp:54 */
  HIP_TRY(b->d_avg.assign(avg.data(), cells * U));
  HIP_TRY(b->d_tx.alloc_zeroed(cells * U));
  HIP_TRY(b->d_cumb.alloc_zeroed(cells * U));
  HIP_TRY(b->d_cumr.alloc_zeroed(cells * U));
  HIP_TRY(b->d_sstate.alloc_zeroed(cells * S));
  HIP_TRY(b->d_scal.alloc(cells));
  HIP_TRY(b->d_err.alloc_zeroed(1));
  HIP_TRY(b->d_slice_bytes.alloc(64));
#ifdef RS_STAMPS
  HIP_TRY(b->d_stamps.alloc_zeroed(20 * cells));
#endif
  rc = init_scalars(b, nullptr, nullptr);
  if (rc) return rc;

  RsLaunch& L = b->base;
  memset(&L, 0, sizeof L);
  L.S = b->S; L.U = b->U; L.R = b->R; L.G = b->G;
  L.sched = b->sched;
  L.n_cells = b->n_cells;
  L.refresh = b->cfg.cqi_refresh;
  L.epoch_wrap = b->cfg.cqi_epoch_wrap ? 1 : 0;
  L.phy_draws = b->cfg.phy_error_draws;
  L.tab = b->d_tab; L.weight = b->d_weight; L.eps = b->d_eps; L.psi = b->d_psi;
  L.alpha = b->d_alpha; L.beta = b->d_beta;
  L.user_slice = b->d_user_slice;
  L.tbs_eff = b->d_tbs_eff;
  L.synthetic = b->synthetic ? 1 : 0;
  L.avg = b->d_avg; L.tx_bytes = b->d_tx; L.cum_bytes = b->d_cumb; L.cum_rbs = b->d_cumr;
  L.slice_state = b->d_sstate; L.scal = b->d_scal; L.err = b->d_err; L.stamps = b->d_stamps;
  carve_lds(b, &L);
  if (L.lds_bytes > 160 * 1024) return fail(RS_ERR_INVALID, "cell needs %d B of LDS (> 160 KiB)", L.lds_bytes);
  {
    /* co-resident cells take turns at the issue priority (RS_SETPRIO, rs_kernels.hip) when the batch has more cells than the device has
     * compute units -- the second dispatch round shares its CUs with the first, which would win every tie by age.  RS_PRIO_BALANCE=0 / 1
     * overrides. */
    const int cus = device_cus(b->cfg.cell.device);
    int mode = (!b->direct && b->n_cells > cus) ? 2 : 0; /* 2: feedback through a progress sum (rs_kernels.hip), 1: time windows, 0: off */
    if (const char* e = getenv("RS_PRIO_BALANCE")) mode = b->direct ? 0 : atoi(e);
    L.prio_round_cells = mode == 1 ? cus : 0;
    if (mode == 2) {
      HIP_TRY(b->d_prio_sum.alloc_zeroed(1));
      L.prio_sum = b->d_prio_sum;
    }
  }
  HIP_TRY(rs_prepare_kernels(160 * 1024));
  return RS_OK;
}

rs_batch* batch_new(const rs_batch_config* cfg, bool direct) {
  if (!cfg) { fail(RS_ERR_INVALID, "null config"); return nullptr; }
  if (validate(&cfg->cell, direct)) return nullptr;
  if (cfg->n_cells < 1) { fail(RS_ERR_INVALID, "n_cells %d < 1", cfg->n_cells); return nullptr; }
  if (!direct && cfg->cqi_refresh < 1) { fail(RS_ERR_INVALID, "cqi_refresh %d < 1", cfg->cqi_refresh); return nullptr; }
  if (cfg->first_tti < 0) { fail(RS_ERR_INVALID, "first_tti %d < 0", cfg->first_tti); return nullptr; }
  int threads = cfg->threads_per_cell;
  if (threads == 0) {
    /* default: 512 threads per cell while the batch leaves at most ~2 cells per CU (per-level latency
     * matters), 256 (two array positions per lane, fewer instructions per level) once 4+ cells share a CU */
    threads = (!direct && cfg->n_cells >= 4 * device_cus(cfg->cell.device)) ? 256 : 512;
  }
  int want_jit = cfg->jit;
  if (const char* e = getenv("RS_JIT")) want_jit = atoi(e);
  /* the kernels built into the library are bounded at 512 threads; a shape-specialised build takes up to 1 024 (the 64-RBG
   * grid runs 640: two sort positions per lane instead of three on half of the waves) */
  const int max_threads = (want_jit && !direct) ? 1024 : 512;
  if (threads % 64 || threads < 64 || threads > max_threads) {
    fail(RS_ERR_INVALID, "threads_per_cell %d (a multiple of 64 in 64..%d%s)", threads, max_threads,
         max_threads == 512 ? "; up to 1024 with jit = 1" : "");
    return nullptr;
  }
  if ((cfg->cqi_epoch_wrap | 1) != 1) { fail(RS_ERR_INVALID, "cqi_epoch_wrap %d is not 0 or 1", cfg->cqi_epoch_wrap); return nullptr; }
  if ((cfg->autotune | 1) != 1) { fail(RS_ERR_INVALID, "autotune %d is not 0 or 1", cfg->autotune); return nullptr; }
  if (cfg->selfcheck < -1 || cfg->selfcheck > 1) { fail(RS_ERR_INVALID, "selfcheck %d outside -1..1", cfg->selfcheck); return nullptr; }
  if (cfg->queue_state_lds < -1 || cfg->queue_state_lds > 1) { fail(RS_ERR_INVALID, "queue_state_lds %d outside -1..1", cfg->queue_state_lds); return nullptr; }
  if (cfg->cell.sched == RS_SCHED_UPPERBOUND) {
    /* the per-slice sorts use the register form of the sort emulation: at most four array positions per thread */
    const int N = cfg->cell.n_rbgs * cfg->cell.n_slices;
    if (cfg->threads_per_cell == 0)
      while (threads < 512 && N > 4 * threads) threads += 64;
    if (N > 4 * threads) {
      fail(RS_ERR_INVALID, "RS_SCHED_UPPERBOUND: n_rbgs * n_slices = %d exceeds 4 * threads_per_cell = %d", N, 4 * threads);
      return nullptr;
    }
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { fail(RS_ERR_NO_DEVICE, "no HIP device"); return nullptr; }
  if (cfg->cell.device < 0 || cfg->cell.device >= n) { fail(RS_ERR_NO_DEVICE, "device %d of %d", cfg->cell.device, n); return nullptr; }
  rs_batch* b = new (std::nothrow) rs_batch();
  if (!b) { fail(RS_ERR_INVALID, "out of memory"); return nullptr; }
  b->cfg = *cfg;
  const rs_config& c = cfg->cell;
  b->S = c.n_slices; b->U = c.n_users; b->R = c.n_rbgs; b->G = c.rbg_size; b->sched = c.sched;
  b->n_cells = cfg->n_cells;
  b->threads = threads;
  b->direct = direct;
  b->weight.assign(c.slice_weight, c.slice_weight + b->S);
  b->eps.assign(c.algo_epsilon, c.algo_epsilon + b->S);
  b->psi.assign(c.algo_psi, c.algo_psi + b->S);
  b->alpha.assign(c.algo_alpha, c.algo_alpha + b->S);
  b->beta.assign(b->S, 0);
  if (c.algo_beta) b->beta.assign(c.algo_beta, c.algo_beta + b->S);
  b->synthetic = c.synthetic_exp != 0;
  for (int s = 0; s < b->S; s++) b->any_alpha |= b->alpha[s] != 0;
  /* (the per-flow PF scheduler and the NVS sampler do not use the exponents: dl-pf-packet-scheduler.cpp:128-140, nvs :519-520) */
  for (int s = 0; s < b->S; s++)
    b->gen_exp |= direct && c.sched != RS_SCHED_PF && c.sched != RS_SCHED_NVS_NONGREEDY && ((b->eps[s] | 1) != 1 || (b->psi[s] | 1) != 1);
  b->u2s.assign(c.user_to_slice, c.user_to_slice + b->U);
  b->cfg.cell.slice_weight = nullptr; b->cfg.cell.algo_alpha = nullptr; b->cfg.cell.algo_beta = nullptr;
  b->cfg.cell.algo_epsilon = nullptr; b->cfg.cell.algo_psi = nullptr; b->cfg.cell.user_to_slice = nullptr;
  b->jit_wanted = want_jit && !direct; /* (before the LDS carve: its NVS rule depends on which kernels will run) */
  if (batch_alloc(b)) { rs_batch_destroy(b); return nullptr; }
  if (want_jit && !direct) {
    /* failure is not an error of this call: the built-in kernels stay in use and the batch keeps the reason
     * (rs_batch_jit_status); rs_last_error() is left alone */
    char msg[sizeof b->jit_msg] = "";
    RsJitKernel* const k = batch_build(b, rs_batch::kGeneral, msg, sizeof msg);
    if (k) snprintf(msg, sizeof msg, "%s", rs_jit_is_untuned(k) ? "in use, built WITHOUT the -mllvm tuning options (hiprtc refused them): a few per cent slower" : "");
    else if (!msg[0]) snprintf(msg, sizeof msg, "hiprtc build failed");
    reset_builds(b, k, msg);
    if (!k && b->threads > 512) { /* nothing else can launch this workgroup size */
      fail(RS_ERR_INVALID, "threads_per_cell %d needs the shape-specialised kernel, which could not be built: %s", b->threads, b->jit_msg);
      rs_batch_destroy(b);
      return nullptr;
    }
  }
  return b;
}

int check_device_err(rs_batch* b) {
  int e = 0;
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(b->d_err.download(&e));
  if (e) {
    HIP_TRY(b->d_err.zero());
    return fail(RS_ERR_RANGE, e == RS_CQI_EPOCHS ? "ran past the last CQI epoch" : "trace row outside the uploaded rows");
  }
  return RS_OK;
}

/* Long unlogged runs on epoch grids -- what the measurements and any production batch are -- go to the LEAN build of the
 * shape-specialised kernel: the options such a launch does not use (trace rows, per-PRB twins, the decision log, error-model draws,
 * synthetic-experiment blocks) are compile-time constants there.  Compiled once, at the first launch that qualifies
 * (RS_JIT_LEAN_MIN_TTIS, default 256: short test launches are not worth a hiprtc run; RS_JIT_LEAN=0 switches it off) or by
 * rs_batch_prepare_launch; nullptr = the general kernel (or the built-in ones) serves this launch. */
bool lean_qualifies(const rs_batch* b, int n_ttis, bool logged) {
  if (!b->general() || b->direct || logged) return false;
  const char* const e_min = getenv("RS_JIT_LEAN_MIN_TTIS");
  const char* const e_on = getenv("RS_JIT_LEAN");
  const int lean_min = e_min ? atoi(e_min) : 256;
  if (e_on && atoi(e_on) == 0) return false;
  return !(n_ttis < lean_min || b->cqi.mode != RS_CQI_EPOCHS || b->cqi.epochs_prb || b->cfg.phy_error_draws || b->synthetic);
}
RsJitKernel* lean_kernel(rs_batch* b, int n_ttis, bool logged) {
  if (!lean_qualifies(b, n_ttis, logged)) return nullptr;
  rs_batch::Build& lean = b->builds.at[rs_batch::kLean];
  if (!lean.tried) {
    lean.tried = true;
    char msg[512] = "";
    lean.k = batch_build(b, rs_batch::kLean, msg, sizeof msg);
    /* not an error of the launch -- the general build serves it -- but nothing silent either: rs_batch_jit_status carries the reason */
    if (!lean.k) snprintf(b->jit_msg, sizeof b->jit_msg, "lean build unavailable, the general build serves every launch (%.400s)", msg);
  }
  return lean.k;
}

/* One launch of a batch: the TTIs, the device rows of a logged run (all null: unlogged), the record block with one cell's capacity
 * (rs_batch_run_records / rs_batch_run_grant_records), and which kernel runs it.  kUsual: launch() picks -- the records variant, the
 * lean build or the general build as they qualify, after the self-check and the autotune that are due.  kThis / kBuiltin: a TRIAL of the
 * self-checks or the autotune on `kernel` / on the kernels built into the library; it checks nothing, tunes nothing and leaves no mark
 * in `builds.last`. */
struct LaunchReq {
  int n_ttis = 0;
  int16_t *map = nullptr, *quota = nullptr, *target = nullptr;
  int32_t *tbs = nullptr, *uinfo = nullptr;
  uint32_t* keys = nullptr;
  int32_t* bbytes = nullptr; /* the per-bearer rows of a queue-model batch */
  double* bhol = nullptr;
  void* recs = nullptr;
  int64_t rec_cap = 0;
  enum Pick { kUsual, kThis, kBuiltin } pick = kUsual;
  RsJitKernel* kernel = nullptr;
  explicit LaunchReq(int n) : n_ttis(n) {}
  LaunchReq(int n, Pick p, RsJitKernel* k = nullptr) : n_ttis(n), pick(p), kernel(k) {}
  bool logged() const { return map || quota || target || tbs || uinfo || keys || bbytes; }
};
int launch(rs_batch* b, const LaunchReq& rq);
int records_kernel(rs_batch* b, int n_ttis, RsJitKernel** k, int* slot);

/* Everything a batch carries from one launch to the next, as (device pointer, bytes): PF averages, pending grants, cumulative counters,
 * slice state, clock / rand() ring / CQI-report state, and with the queue model the bearers' queues, averages, counters and per-user
 * words.  One list for the checkpoint (rs_batch_checkpoint_*), the autotune's snapshot and the self-check's. */
struct StatePart {
  void* p; size_t n;
  template <typename T> StatePart(const DevBuf<T>& d) : p(d.get()), n(d.bytes()) {} /* a whole array, as the buffer has it */
};
std::vector<StatePart> state_parts(rs_batch* b) { /* (the order is the checkpoint's format) */
  std::vector<StatePart> v = {b->d_avg, b->d_tx, b->d_cumb, b->d_cumr, b->d_sstate, b->d_scal};
  if (b->queues) v.insert(v.end(), {b->d_qi, b->d_bavg, b->d_bcum, b->d_qflags, b->d_qhol});
  return v;
}

/* ---- a device-side snapshot of that state: what rs_batch_config.autotune and the self-check put back after their trial launches ---- */
struct StateParts {
  std::vector<StatePart> parts;
  size_t total = 0;
  /* with_record: the flow completion record too (the self-check's trials write it; it is output, so the checkpoint leaves it out) */
  explicit StateParts(rs_batch* b, bool with_record = false) : parts(state_parts(b)) {
    if (with_record && b->queues && b->d_flow_tti) parts.insert(parts.end(), {b->d_flow_tti, b->d_flow_time});
    for (const StatePart& q : parts) total += (q.n + 255) & ~(size_t)255;
  }
  hipError_t copy(rs_batch* b, void* snapshot, bool save) const {
    size_t off = 0;
    for (const StatePart& q : parts) {
      void* snap = (char*)snapshot + off;
      const hipError_t e = hipMemcpyAsync(save ? snap : q.p, save ? q.p : snap, q.n, hipMemcpyDeviceToDevice, b->stream);
      if (e != hipSuccess) return e;
      off += (q.n + 255) & ~(size_t)255;
    }
    return hipSuccess;
  }
};

/* What a run leaves behind, in the form every kernel of a batch must agree on bit for bit: PF averages, cumulative bytes / RBs, slice
 * state, the bytes of the pending grants (the shape-specialised kernels pack more into that word), clock, rand() ring and CQI-report
 * state.  FNV-1a over the host copy (a few MB, once per trial). */
struct StateDigest {
  unsigned long long part[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; /* PF averages, cumulative bytes, cumulative RBs, slice state, pending grants' bytes, scalars; queue model: the bearers' queues, averages, counters, the flow completion record */
  bool operator==(const StateDigest& o) const { return memcmp(part, o.part, sizeof part) == 0; }
  bool operator!=(const StateDigest& o) const { return !(*this == o); }
  std::string diff(const StateDigest& o) const {
    static const char* const names[14] = {"PF averages", "cumulative bytes", "cumulative RBs", "slice state", "pending grants", "simulated time",
                                          "last EWMA update", "TTIs done", "users served in the last TTI", "rand() ring / CQI-report state",
                                          "bearers' queues", "bearers' PF averages", "bearers' cumulative counters", "flow completion record"};
    std::string d;
    for (int i = 0; i < 14; i++)
      if (part[i] != o.part[i]) d += std::string(d.empty() ? "" : ", ") + names[i];
    return d;
  }
};
int state_digest(rs_batch* b, StateDigest* out) {
  HIP_TRY(hipStreamSynchronize(b->stream));
  auto fnv = [](const void* p, size_t n, unsigned long long d = 1469598103934665603ull) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) { d ^= c[i]; d *= 1099511628211ull; }
    return d;
  };
  std::vector<unsigned char> h;
  const auto whole = [&](const StatePart& q, unsigned long long* d) -> int { /* one array, as it is */
    h.resize(q.n);
    HIP_TRY(hipMemcpy(h.data(), q.p, q.n, hipMemcpyDeviceToHost));
    *d = fnv(h.data(), q.n);
    return RS_OK;
  };
  const StatePart plain[4] = {b->d_avg, b->d_cumb, b->d_cumr, b->d_sstate};
  for (int i = 0; i < 4; i++)
    if (const int rc = whole(plain[i], &out->part[i])) return rc;
  std::vector<int32_t> tx(b->d_tx.count());
  HIP_TRY(b->d_tx.download(tx.data()));
  for (int32_t& v : tx) v &= RS_TX_BYTES_MASK;
  out->part[4] = fnv(tx.data(), 4 * tx.size());
  std::vector<RsCellScalars> sc;
  if (const int rc = read_scalars(b, &sc)) return rc;
  for (int i = 5; i < 10; i++) out->part[i] = 1469598103934665603ull;
  for (const RsCellScalars& c : sc) {
    out->part[5] = fnv(&c.t, 8, out->part[5]);
    out->part[6] = fnv(&c.last_update, 8, out->part[6]);
    out->part[7] = fnv(&c.n_done, 8, out->part[7]);
    /* (read by the error model's draws only: a lean build, which serves batches without them, does not keep it) */
    if (b->cfg.phy_error_draws) out->part[8] = fnv(&c.served_prev, 4, out->part[8]);
    unsigned long long d = out->part[9];
    if (b->cqi.mode == RS_CQI_TRACE) { d = fnv(&c.last_sent, 8, d); d = fnv(&c.reported, 4, d); d = fnv(&c.cqi_row, 4, d); }
    /* the ring in age order: the kernels may leave it rotated differently (f, b) with the same future */
    for (int i = 0; i < 31; i++) { const uint32_t w = c.rng_r[(c.rng_f + i) % 31]; d = fnv(&w, 4, d); }
    out->part[9] = d;
  }
  if (b->queues) {
    /* the queue model: head, tail, pk, frag, bytes, pkts, tx of every bearer; its PF average; its cumulative bytes / RBs.  (The per-user
     * flag and HoL words are rebuilt by every TTI's first phase before anything reads them: scratch, not compared.) */
    const StatePart q[3] = {b->d_qi, b->d_bavg, b->d_bcum};
    for (int i = 0; i < 3; i++)
      if (const int rc = whole(q[i], &out->part[10 + i])) return rc;
    if (b->d_flow_tti) { /* the record: TTI indices and clock values of the completed flows */
      std::vector<unsigned char> hr(b->d_flow_tti.bytes() + b->d_flow_time.bytes());
      HIP_TRY(b->d_flow_tti.download(hr.data()));
      HIP_TRY(b->d_flow_time.download(hr.data() + b->d_flow_tti.bytes()));
      out->part[13] = fnv(hr.data(), hr.size());
    }
  }
  return RS_OK;
}

/* The pending-grant words between their two formats.  A shape-specialised kernel keeps bytes | PRBs << 20 | "counted" << 30 there (RS_TX_*:
 * the grant is in the cumulative totals already), the built-in kernels plain bytes (they count at grant time).  to_packed = false: the
 * run-time builds' word to plain bytes; true: plain bytes to a word whose grant is in the totals.  Wherever the built-in kernels run a
 * launch, or take over, beside run-time builds.  The queue model's kernels, built-in and run-time, share one format (and consume every
 * grant before the launch ends): nothing to convert there. */
int convert_tx(rs_batch* b, bool to_packed) {
  if (b->queues) return RS_OK;
  std::vector<int32_t> tx(b->d_tx.count());
  if (hipStreamSynchronize(b->stream) != hipSuccess || b->d_tx.download(tx.data()) != hipSuccess)
    return fail(RS_ERR_HIP, "copy of the pending grants failed");
  for (int32_t& w : tx) w = to_packed ? (w ? ((w & RS_TX_BYTES_MASK) | RS_TX_COUNTED) : 0) : (w & RS_TX_BYTES_MASK);
  if (b->d_tx.upload(tx.data()) != hipSuccess) return fail(RS_ERR_HIP, "copy of the pending grants failed");
  return RS_OK;
}

/* The trials of the self-checks and the autotune: launches of the batch's next TTIs on a kernel the caller names, every one from the
 * same snapshot, and the snapshot put back afterwards so that they leave no trace in the run.  Owns the snapshot, the saved TTI count
 * and the scratch allocations (the callers' record blocks too); `who` opens its error messages. */
struct Trials {
  rs_batch* const b;
  const char* const who;
  const StateParts sp;
  const int64_t done0;
  ScratchBuffers scratch;
  void* snap = nullptr;
  bool open = false; /* the snapshot is taken and not yet put back for good */
  Trials(rs_batch* b, const char* who, bool with_record) : b(b), who(who), sp(b, with_record), done0(b->ttis_done) {}
  ~Trials() { if (open) (void)put_back(); } /* an early return of the caller: the run still continues from where it was */
  int begin() {
    if (scratch.alloc(&snap, sp.total) != hipSuccess || sp.copy(b, snap, true) != hipSuccess) return fail(RS_ERR_HIP, "%s: snapshot failed", who);
    open = true;
    return RS_OK;
  }
  /* one trial: the state of the snapshot -- the pending-grant words as plain bytes where the built-in kernels run (convert_tx) --, the
   * launch, between the two events if the caller times it, and what it left (`out`; nullptr: not looked at) */
  int run(const LaunchReq& rq, StateDigest* out, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    if (sp.copy(b, snap, false) != hipSuccess) return fail(RS_ERR_HIP, "%s: state restore failed", who);
    int rc = rq.pick == LaunchReq::kBuiltin ? convert_tx(b, false) : RS_OK;
    if (!rc && e0 && hipEventRecord(e0, b->stream) != hipSuccess) rc = fail(RS_ERR_HIP, "%s: timing failed", who);
    if (!rc) rc = launch(b, rq);
    if (!rc && e1 && hipEventRecord(e1, b->stream) != hipSuccess) rc = fail(RS_ERR_HIP, "%s: timing failed", who);
    if (!rc && out) rc = state_digest(b, out);
    return rc;
  }
  int put_back() {
    open = false;
    const hipError_t back = sp.copy(b, snap, false);
    const hipError_t sync = hipStreamSynchronize(b->stream);
    b->ttis_done = done0;
    return back != hipSuccess || sync != hipSuccess ? fail(RS_ERR_HIP, "%s: the cell state could not be put back", who) : RS_OK;
  }
  /* the end of the trials: the state back, then `rc` of the trials if one failed, then the device's error word */
  int finish(int rc) {
    const int back = put_back();
    return back ? back : rc ? rc : check_device_err(b);
  }
};

/* rs_batch_config.autotune: time the lean kernel in the variants the rule table of rs_jit.cpp chooses between, on this batch's own
 * next TTIs, and keep the fastest.  Every trial starts from the same snapshot and the snapshot is put back at the end, so the tuning
 * leaves no trace in the run.  All variants compute the same results (the parity tests run them against the oracle) -- and every
 * trial's final state is compared with the rule table's: a variant that disagrees is never kept (and says so in the report). */
int autotune(rs_batch* b, int n_ttis) {
  if (b->builds.autotuned || !b->cfg.autotune) return RS_OK;
  RsJitKernel* const k_default = lean_kernel(b, n_ttis, false);
  if (!k_default) return RS_OK; /* this launch does not qualify for the lean build: try again at a later one */
  b->builds.autotuned = true;
  const int sched = b->sched;
  if (b->queues || b->direct || !(sched == 8 || sched == 9 || sched == 101 || sched == 103)) return RS_OK;
  const int win = slice_window(b);
  std::vector<std::string> cand = {""};
  const bool ilp_by_rule = sched == 9 || (sched == 8 && (b->R > 32 || win > 0));
  cand.push_back(ilp_by_rule ? "ss=default" : "ss=iterative-ilp");
  cand.push_back(b->R > 32 ? "-DRS_NO_SPEC" : "-DRS_NO_HOLD");
  if (sched == 9) cand.push_back("-DRS_P3_BLOCK=8");
  /* the snapshot and the two events live exactly as long as this call, whichever way it returns; the lean slot keeps the rule table's
   * build until a better one has been chosen (every trial names its kernel) */
  Trials trials(b, "autotune", false);
  ScratchEvents events;
  HIP_TRY(events.create(2));
  const hipEvent_t e0 = events.ev[0], e1 = events.ev[1];
  const int trial = n_ttis < 512 ? n_ttis : 512;
  RsJitKernel* best = k_default;
  float best_ms = 0, default_ms = 0;
  StateDigest default_digest;
  int rc = trials.begin();
  if (rc) return rc;
  std::string report;
  for (size_t i = 0; i < cand.size() && rc == RS_OK; i++) {
    char msg[512] = "";
    RsJitKernel* k = i == 0 ? k_default : batch_build(b, rs_batch::kLean, msg, sizeof msg, cand[i].c_str());
    if (!k) { report += cand[i] + ": not built; "; continue; }
    float ms = 0;
    StateDigest digest;
    for (int rep = 0; rep < 3 && rc == RS_OK; rep++) { /* one warm launch, then the faster of two; the state the last one left */
      rc = trials.run(LaunchReq(trial, LaunchReq::kThis, k), rep == 2 ? &digest : nullptr, e0, e1);
      if (rc) break;
      float t = 0;
      if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) {
        rc = fail(RS_ERR_HIP, "autotune: timing failed");
        break;
      }
      if (rep == 1 || (rep == 2 && t < ms)) ms = t;
    }
    if (rc) break;
    if (i == 0) default_digest = digest;
    char line[320];
    if (digest != default_digest) {
      /* never seen; if it ever is, the variant is a miscompiled kernel (profiles/r05_onelane.md) and must not serve the batch */
      snprintf(line, sizeof line, "%s: %.3f ms, REJECTED: its state after the trial differs from the rule table's build (%s); ", cand[i].c_str(), ms,
               digest.diff(default_digest).c_str());
      report += line;
      rs_jit_reject(k);
      continue;
    }
    /* a variant that agrees with a build that carries the self-check mark has passed the same check by transitivity */
    if (i > 0 && rs_jit_is_verified(k_default)) rs_jit_mark_verified(k);
    snprintf(line, sizeof line, "%s: %.3f ms; ", i == 0 ? "rule table" : cand[i].c_str(), ms);
    report += line;
    b->autotune_n++;
    /* (another build has to win by more than 1 %: below that the launches' own jitter decides) */
    if (i == 0) { best = k; best_ms = default_ms = ms; }
    else if (ms < best_ms && ms < 0.99f * default_ms) { best = k; best_ms = ms; }
  }
  /* the run continues from where it was, whatever happened above */
  rc = trials.finish(rc);
  if (rc) return rc;
  b->builds.at[rs_batch::kLean].k = best;
  snprintf(b->autotune_msg, sizeof b->autotune_msg, "autotune over %d TTIs: %skept %s", trial, report.c_str(),
           best == k_default ? "the rule table's build" : "the fastest");
  return RS_OK;
}

/* Which run-time builds a batch checks against the built-in kernels before it trusts them (round 6: on by default).
 *   rs_batch_config.selfcheck  1: every build, marked or not;  -1: none;  0 (default): every build WITHOUT the self-check mark -- one
 *   that this process compiled, or that came from the disk cache of a process that never checked it.  A build that passed leaves the mark
 *   in its cache file (rs_jit_mark_verified), so the second process of a campaign skips the check.
 *   RS_JIT_SELFCHECK=0 switches the default off (cfg.selfcheck = 1 still checks), RS_JIT_SELFCHECK=2 makes it "every build". */
enum { kCheckNever = 0, kCheckUnmarked = 1, kCheckAll = 2 };
int selfcheck_policy(const rs_batch* b) {
  if (b->cfg.selfcheck > 0) return kCheckAll;
  if (b->cfg.selfcheck < 0) return kCheckNever;
  const char* e = getenv("RS_JIT_SELFCHECK");
  if (e && e[0] == '0') return kCheckNever;
  if (e && e[0] == '2') return kCheckAll;
  return kCheckUnmarked;
}

/* The self-check: the batch's next min(n, 256) TTIs on the kernels built into the library and on its run-time compiled ones (general
 * build, lean build), each from the same snapshot; the final states must agree bit for bit (state_digest).  The built-in kernels are
 * ONE binary, the one the GPU parity suite runs against the oracle; a run-time build is a fresh compilation for this shape, and round 4
 * met one that the compiler got wrong (profiles/r05_onelane.md).  A general build that disagrees is dropped: the batch runs on the
 * built-in kernels and rs_batch_jit_status returns -2 with the reason; a lean build that disagrees while the general one agreed is
 * dropped alone (status stays 1, the message says so).  The snapshot is put back: no trace.  With the queue model the snapshot and the
 * comparison include the bearers' queues, averages and counters (they were left out and the check refused nothing but
 * silently advanced them). */
int selfcheck(rs_batch* b, int n_ttis, bool logged) {
  const int policy = selfcheck_policy(b);
  rs_batch::Builds& B = b->builds;
  rs_batch::Build &gen = B.at[rs_batch::kGeneral], &lean = B.at[rs_batch::kLean];
  if (policy == kCheckNever || B.checked) return RS_OK;
  if (!gen.k || b->direct) { B.checked = true; return RS_OK; } /* nothing run-time compiled */
  if (b->threads > 512) { /* no built-in kernel of this workgroup size to compare with */
    B.checked = true;
    snprintf(b->selfcheck_msg, sizeof b->selfcheck_msg, "not self-checked: the kernels built into the library stop at 512 threads per cell");
    return RS_OK;
  }
  /* the general build at the first launch; the lean build at the first launch that qualifies for it (RS_JIT_LEAN_MIN_TTIS, unlogged) */
  RsJitKernel* const k_lean = lean_kernel(b, n_ttis, logged);
  const bool need_gen = !gen.checked && (policy == kCheckAll || !rs_jit_is_verified(gen.k));
  const bool need_lean = k_lean && !lean.checked && (policy == kCheckAll || !rs_jit_is_verified(k_lean));
  const char* const e_on = getenv("RS_JIT_LEAN");
  const bool lean_off = e_on && atoi(e_on) == 0;
  if (!need_gen && !need_lean) {
    /* builds that came with the mark of an earlier process's check */
    if (!gen.checked) {
      gen.checked = true;
      snprintf(b->selfcheck_msg, sizeof b->selfcheck_msg, "the run-time build carries the self-check mark of the process that compiled it (cache file)");
    }
    if (k_lean) lean.checked = true;
    B.checked = lean.checked || lean_off;
    return RS_OK;
  }
  /* The trials name their kernel: the lean trial runs the lean build however short it is (a launch of `trial` TTIs picking for itself
   * would compare them with RS_JIT_LEAN_MIN_TTIS).  The built-in kernels keep plain bytes in the pending-grant words where a
   * shape-specialised kernel keeps bytes | PRBs << 20 | "counted" << 30 (RS_TX_*): Trials::run converts (convert_tx). */
  Trials trials(b, "selfcheck", true); /* (the trials write the flow completion record: it is put back with the state and compared) */
  const int trial = n_ttis < 256 ? n_ttis : 256;
  StateDigest want, got;
  const char* bad = nullptr;
  int rc = trials.begin();
  if (rc) return rc;
  rc = trials.run(LaunchReq(trial, LaunchReq::kBuiltin), &want);
  if (!rc && need_gen) {
    rc = trials.run(LaunchReq(trial, LaunchReq::kThis, gen.k), &got);
    if (!rc && got != want) bad = "general";
  }
  if (!rc && !bad && need_lean) {
    rc = trials.run(LaunchReq(trial, LaunchReq::kThis, k_lean), &got);
    if (!rc && got != want) bad = "lean";
  }
  rc = trials.finish(rc);
  if (rc) return rc;
  if (bad && bad[0] == 'l') {
    /* the lean build alone is wrong (the general one agreed just now or earlier, or carries the mark): the general build keeps serving every launch */
    rs_jit_reject(k_lean);
    if (need_gen) { gen.checked = true; rs_jit_mark_verified(gen.k); }
    lean = {nullptr, true, true};
    B.checked = true;
    snprintf(b->jit_msg, sizeof b->jit_msg, "selfcheck: after %d TTIs the lean build of the shape-specialised kernel left a state that differs from the "
             "built-in kernels' in: %s; it is dropped and the general build, which agreed, serves every launch", trial, got.diff(want).c_str());
    return RS_OK;
  }
  if (bad) {
    rs_jit_reject(gen.k);
    gen.k = nullptr;
    lean.k = nullptr;
    lean.tried = true;
    B.rejected = true;
    B.checked = true;
    /* the state just put back may have been left by the shape-specialised kernel: the built-in kernels that take over read plain bytes
     * (the first EWMA after a rejection used the packed word as a byte count) */
    rc = convert_tx(b, false);
    if (rc) return rc;
    snprintf(b->jit_msg, sizeof b->jit_msg, "selfcheck: after %d TTIs the %s build of the shape-specialised kernel left a state that differs from the "
             "built-in kernels' in: %s; the batch runs on the built-in kernels (lint the code object: tools/lint_exec_restore.py)", trial, bad,
             got.diff(want).c_str());
    return RS_OK;
  }
  if (need_gen) { gen.checked = true; rs_jit_mark_verified(gen.k); }
  if (need_lean) rs_jit_mark_verified(k_lean);
  if (k_lean) lean.checked = true; /* (checked just now, or came with the mark) */
  snprintf(b->selfcheck_msg, sizeof b->selfcheck_msg, "selfcheck over %d TTIs: the built-in kernels and the %s build%s agree", trial,
           lean.checked ? "general and lean" : "general", lean.checked ? "s" : "");
  B.checked = lean.checked || lean_off; /* the lean build is still to come: look again at the next launch */
  return RS_OK;
}

/* ---- grant records of a backlogged batch (rs_batch_run_grant_records) ---- */

/* most grants of one cell in one TTI: a grant needs an RBG and goes to one user -- min(U, R); UpperBound's slices take their RBGs
 * whatever the other slices take: the sum over the slices of min(the slice's users, R), as rs_group_grant_bound has it */
int grant_bound(const rs_batch* b) {
  if (b->sched != RS_SCHED_UPPERBOUND) { /* (a ragged batch: the largest cell's users) */
    int users = b->U;
    if (b->ragged) users = *std::max_element(b->cc_users.begin(), b->cc_users.end());
    return std::min(users, b->R);
  }
  int most = 0;
  /* (per-cell maps: one capacity serves every cell's list -- the maximum over the cells of the per-slice sum) */
  for (int c = 0; c < (b->cell_cfg ? b->n_cells : 1); c++) {
    const int32_t* const u2s = b->cell_cfg ? b->cc_u2s.data() + (size_t)c * b->U : b->u2s.data();
    int sum = 0;
    for (int u = 0; u < b->U && u2s[u] != RS_USER_ABSENT;) { /* (absent users are in no slice) */
      int e = u;
      while (e < b->U && u2s[e] == u2s[u]) e++;
      sum += std::min(e - u, b->R);
      u = e;
    }
    most = std::max(most, sum);
  }
  return most;
}

/* DoStopSchedule's walk: TTI, then user.  The device hands out all places of TTI k before any of TTI k + 1 and a (TTI, user) occurs once,
 * so every TTI's stretch is sorted by itself, as rs_batch_run_records does it -- but a stretch comes in lane (RBG) order, which says
 * nothing about the users' order, and an insertion sort moves a 32-byte record n / 4 times on average: a record's place is the number
 * of records of the stretch with a smaller user (integer compares, no moves), then one pass through a small buffer.  A stretch longer
 * than the buffer (UpperBound with many slices) and a list whose TTIs do not ascend go to std::sort. */
void sort_grant_records(rs_batch_grant_record* r, size_t n) {
  bool ascending = true;
  constexpr size_t kBuf = 128;
  rs_batch_grant_record tmp[kBuf];
  const auto by_user = [](const rs_batch_grant_record& x, const rs_batch_grant_record& y) { return x.user < y.user; };
  for (size_t i = 0, j; i < n; i = j) {
    if (i && r[i].tti < r[i - 1].tti) ascending = false;
    bool sorted = true;
    for (j = i + 1; j < n && r[j].tti == r[i].tti; j++) sorted &= r[j - 1].user <= r[j].user;
    if (sorted) continue;
    const size_t m = j - i;
    if (m > kBuf) { std::sort(r + i, r + j, by_user); continue; }
    memcpy(tmp, r + i, m * sizeof tmp[0]);
    for (size_t a = 0; a < m; a++) {
      size_t rank = 0;
      for (size_t q = 0; q < m; q++) rank += (tmp[q].user < tmp[a].user || (tmp[q].user == tmp[a].user && q < a)) ? 1 : 0;
      r[i + rank] = tmp[a];
    }
  }
  if (!ascending)
    std::sort(r, r + n, [](const rs_batch_grant_record& x, const rs_batch_grant_record& y) { return x.tti != y.tti ? x.tti < y.tti : x.user < y.user; });
}

/* The self-check of a records variant (v: 0 general, 1 lean): a fresh compilation whose new code is the record writing, so it is checked
 * with records on -- the batch's next min(n, 256) TTIs from one snapshot on the built-in kernels and on the variant, each into a scratch
 * record block; the final states must agree bit for bit and the sorted lists record for record.  A variant that disagrees is dropped
 * alone (the caller goes on to the next fallback), rs_batch_jit_status names cell, record index and field.  The snapshot is put back. */
int selfcheck_records(rs_batch* b, int n_ttis, int v) {
  rs_batch::Build& var = b->builds.at[rs_batch::kRecGeneral + v];
  RsJitKernel* const k = var.k;
  var.checked = true;
  const int policy = selfcheck_policy(b);
  if (policy == kCheckNever) return RS_OK;
  if (policy == kCheckUnmarked && rs_jit_is_verified(k)) {
    snprintf(b->selfcheck_msg, sizeof b->selfcheck_msg, "the records variant of the %s build carries the self-check mark of the process that checked it (cache file)", v ? "lean" : "general");
    return RS_OK;
  }
  if (b->threads > 512) return RS_OK; /* no built-in kernel of this workgroup size to compare with (selfcheck() says so for the plain builds) */
  Trials trials(b, "selfcheck", false);
  const size_t cells = (size_t)b->n_cells;
  const int trial = n_ttis < 256 ? n_ttis : 256;
  const int64_t cap = (int64_t)trial * grant_bound(b);
  const size_t list_bytes = cells * (size_t)cap * sizeof(RsBatchGrantRecord), block_bytes = list_bytes + 4 * cells;
  char* block[2] = {nullptr, nullptr};
  HIP_TRY(trials.scratch.alloc(&block[0], block_bytes));
  HIP_TRY(trials.scratch.alloc(&block[1], block_bytes));
  StateDigest want, got;
  int rc = trials.begin();
  if (rc) return rc;
  for (int t = 0; t < 2 && rc == RS_OK; t++) { /* t = 0: the built-in kernels, 1: the variant */
    if (hipMemsetAsync(block[t] + list_bytes, 0, 4 * cells, b->stream) != hipSuccess) rc = fail(RS_ERR_HIP, "selfcheck: record block");
    LaunchReq rq(trial, t == 0 ? LaunchReq::kBuiltin : LaunchReq::kThis, t == 0 ? nullptr : k);
    rq.recs = block[t];
    rq.rec_cap = cap;
    if (!rc) rc = trials.run(rq, t == 0 ? &want : &got);
  }
  /* the two blocks, sorted as the caller's lists are */
  std::vector<rs_batch_grant_record> list[2];
  std::vector<uint32_t> count[2];
  for (int t = 0; t < 2 && rc == RS_OK; t++) {
    list[t].resize(cells * (size_t)cap);
    count[t].resize(cells);
    if (hipMemcpy(count[t].data(), block[t] + list_bytes, 4 * cells, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(RS_ERR_HIP, "selfcheck: copy of the records failed"); break; }
    for (size_t c = 0; c < cells && rc == RS_OK; c++) {
      const size_t used = (size_t)std::min((int64_t)count[t][c], cap);
      if (used && hipMemcpy(list[t].data() + c * (size_t)cap, block[t] + c * (size_t)cap * sizeof(RsBatchGrantRecord), used * sizeof(RsBatchGrantRecord), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(RS_ERR_HIP, "selfcheck: copy of the records failed");
      if (!rc) sort_grant_records(list[t].data() + c * (size_t)cap, used);
    }
  }
  rc = trials.finish(rc);
  if (rc) return rc;
  char why[256] = "";
  if (got != want) snprintf(why, sizeof why, "left a state that differs from the built-in kernels' in: %s", got.diff(want).c_str());
  for (size_t c = 0; c < cells && !why[0]; c++) {
    if (count[0][c] != count[1][c]) { snprintf(why, sizeof why, "wrote %u grant records for cell %zu, the built-in kernels %u", count[1][c], c, count[0][c]); break; }
    const rs_batch_grant_record *x = list[0].data() + c * (size_t)cap, *y = list[1].data() + c * (size_t)cap;
    const size_t used = (size_t)std::min((int64_t)count[0][c], cap);
    for (size_t i = 0; i < used && !why[0]; i++) {
      const long long fx[9] = {x[i].tti, x[i].user, x[i].tbs_bits, x[i].bytes, (long long)x[i].rbg_mask, x[i].nprb, x[i].final_cqi, x[i].mcs, x[i].reserved};
      const long long fy[9] = {y[i].tti, y[i].user, y[i].tbs_bits, y[i].bytes, (long long)y[i].rbg_mask, y[i].nprb, y[i].final_cqi, y[i].mcs, y[i].reserved};
      static const char* const names[9] = {"tti", "user", "tbs_bits", "bytes", "rbg_mask", "nprb", "final_cqi", "mcs", "reserved"};
      for (int f = 0; f < 9; f++)
        if (fx[f] != fy[f]) {
          snprintf(why, sizeof why, "wrote a grant record that differs from the built-in kernels': cell %zu, record %zu, field %s: %lld against %lld", c, i, names[f], fy[f], fx[f]);
          break;
        }
    }
  }
  if (why[0]) {
    rs_jit_reject(k);
    var.k = nullptr;
    if (v == 0) b->builds.rec_rejected = true;
    snprintf(b->jit_msg, sizeof b->jit_msg, "selfcheck: after %d TTIs the records variant of the %s build %s; it is dropped and %s the records launches", trial,
             v ? "lean" : "general", why, v ? "the general build's records variant serves" : "the built-in kernels serve");
    return RS_OK;
  }
  rs_jit_mark_verified(k);
  snprintf(b->selfcheck_msg, sizeof b->selfcheck_msg, "selfcheck over %d TTIs: the built-in kernels and the records variant of the %s build agree, state and records", trial,
           v ? "lean" : "general");
  return RS_OK;
}

/* The kernel of a records launch: the records variant (-DRS_JIT_RECORDS=1) of the build launch() would pick for an unlogged launch of
 * these TTIs -- lean where it qualifies, streamed where the batch is --, compiled at the first records launch that needs it and checked
 * with records on; it falls back as the lean build does, to the general build's variant and then (*k = nullptr) to the built-in kernels. */
int records_kernel(rs_batch* b, int n_ttis, RsJitKernel** k, int* slot) {
  *k = nullptr;
  *slot = rs_batch::kBuiltinRecords;
  if (!b->general() || b->builds.rec_rejected) return RS_OK;
  for (int v = lean_qualifies(b, n_ttis, false) ? 1 : 0; v >= 0; --v) {
    rs_batch::Build& var = b->builds.at[rs_batch::kRecGeneral + v];
    if (!var.tried) {
      var.tried = true;
      char msg[512] = "";
      var.k = batch_build(b, rs_batch::kRecGeneral + v, msg, sizeof msg);
      if (!var.k)
        snprintf(b->jit_msg, sizeof b->jit_msg, "records variant of the %s build unavailable, %s the records launches (%.380s)", v ? "lean" : "general",
                 v ? "the general build's serves" : "the built-in kernels serve", msg);
    }
    if (var.k && !var.checked) {
      const int rc = selfcheck_records(b, n_ttis, v); /* (a variant that disagrees is gone afterwards) */
      if (rc) return rc;
    }
    if (var.k) { *k = var.k; *slot = rs_batch::kRecGeneral + v; return RS_OK; }
  }
  return RS_OK;
}

int launch(rs_batch* b, const LaunchReq& rq) {
  const int n_ttis = rq.n_ttis;
  if (n_ttis < 1) return fail(RS_ERR_INVALID, "n_ttis %d < 1", n_ttis);
  if (b->cqi.mode == RS_CQI_NONE) return fail(RS_ERR_STATE, "no CQI source set");
  if (b->any_alpha && !b->direct && !b->queues)
    return fail(RS_ERR_STATE, "customised slices (algo_alpha = 1) read queue state: call rs_batch_set_bearers / rs_batch_set_arrivals first");
  if (b->queues && !b->d_arr_off) return fail(RS_ERR_STATE, "rs_batch_set_arrivals has not been called");
  if (n_ttis > RS_MAX_TTIS_PER_LAUNCH) {
    /* longer runs go out as several launches (state carries over; the per-launch counters of the kernel are 32-bit) */
    if (rq.logged()) return fail(RS_ERR_INVALID, "logged runs are limited to %d TTIs per call", RS_MAX_TTIS_PER_LAUNCH);
    for (int done = 0; done < n_ttis;) {
      const int chunk = n_ttis - done < RS_MAX_TTIS_PER_LAUNCH ? n_ttis - done : RS_MAX_TTIS_PER_LAUNCH;
      const int rc = launch(b, LaunchReq(chunk));
      if (rc) return rc;
      done += chunk;
    }
    return RS_OK;
  }
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  RsLaunch L = b->base;
  L.n_ttis = n_ttis;
  const rs_batch::CqiSource& q = b->cqi; /* (a batch holds the arrays of the kind it reads and no others: the rest are null) */
  L.cqi_mode = q.mode;
  L.epochs = q.epochs; L.grid_stride = q.grid_stride; L.n_epochs = q.n_epochs;
  L.trace = q.trace; L.n_traces = q.n_traces; L.n_rows = q.n_rows; L.row_mod = q.row_mod;
  L.user_trace = q.user_trace;
  L.epochs_prb = q.epochs_prb; L.grid_stride_prb = q.grid_stride_prb;
  L.trace_prb = q.trace_prb;
  L.log_map = rq.map; L.log_quota = rq.quota; L.log_target = rq.target; L.log_tbs = rq.tbs; L.log_uinfo = rq.uinfo;
  L.log_keys = rq.keys;
  if (b->queues) {
    L.bearer_kind = b->d_bearer_kind; L.arr_off = b->d_arr_off; L.arr_time = b->d_arr_time;
    L.arr_nfull = b->d_arr_nfull; L.arr_last = b->d_arr_last;
    L.q_head = plane(b, b->d_qi, 0); L.q_tail = plane(b, b->d_qi, 1); L.q_pk = plane(b, b->d_qi, 2); L.q_frag = plane(b, b->d_qi, 3);
    L.q_bytes = plane(b, b->d_qi, 4); L.q_pkts = plane(b, b->d_qi, 5); L.b_tx = plane(b, b->d_qi, 6);
    L.b_avg = b->d_bavg; L.b_cumb = plane(b, b->d_bcum, 0); L.b_cumr = plane(b, b->d_bcum, 1);
    L.q_flags = b->d_qflags; L.q_hol = b->d_qhol;
    L.flow_tti = b->d_flow_tti; L.flow_time = b->d_flow_time;
    L.log_bbytes = rq.bbytes; L.log_bhol = rq.bhol;
    /* bearer records (rs_batch_run_records; RsBearerRecord, rs_device.h): a batch launch sends no group's sent rows, the two words carry
     * the record block and one cell's capacity.  Null in every other launch -- the self-check's and the autotune's trials included. */
    L.grp_sent = (int32_t*)rq.recs; L.grp_sent_stride = rq.recs ? rq.rec_cap : 0;
  }
  /* grant records of a backlogged batch (rs_batch_run_grant_records; RsBatchGrantRecord, rs_device.h): the same two words.  Null in every
   * other launch -- the self-check's and the autotune's trials included; selfcheck_records' trials bring scratch blocks of their own. */
  const bool records = !b->queues && !b->direct && rq.recs != nullptr;
  if (records) { L.grp_sent = (int32_t*)rq.recs; L.grp_sent_stride = rq.rec_cap; }
  const bool logged = rq.logged(), trial = rq.pick != LaunchReq::kUsual;
  /* (a records launch runs none of the plain builds: they are checked at the first launch they serve) */
  if (!trial && !records && !b->builds.checked && b->general() && !b->direct) {
    const int rc = selfcheck(b, n_ttis, logged); /* (its trials come back through here, as trials) */
    if (rc) return rc;
  }
  if (!trial && b->cfg.autotune && !b->builds.autotuned && !logged && !records) {
    const int rc = autotune(b, n_ttis);
    if (rc) return rc;
  }
  RsJitKernel* k = nullptr;
  bool builtin_beside_jit = false; /* the built-in kernels serve this launch of a batch whose state the run-time builds keep */
  if (trial) {
    k = rq.pick == LaunchReq::kThis ? rq.kernel : nullptr; /* (the built-in kernels' trial: Trials::run has converted the pending-grant words) */
  } else if (records) {
    int slot = rs_batch::kBuiltinRecords;
    const int rc = records_kernel(b, n_ttis, &k, &slot); /* (compiles and checks the variant at its first launch) */
    if (rc) return rc;
    if (!k && b->threads > 512) return fail(RS_ERR_STATE, "grant records: no records variant of the run-time build is available and the built-in kernels stop at 512 threads per cell (%s)", b->jit_msg);
    b->builds.last = slot;
    builtin_beside_jit = !k && b->general();
  } else {
    k = lean_kernel(b, n_ttis, logged);
    b->builds.last = k ? rs_batch::kLean : rs_batch::kGeneral;
    if (!k) k = b->general();
  }
  if (builtin_beside_jit) { const int rc = convert_tx(b, false); if (rc) return rc; }
  if (L.prio_sum) HIP_TRY(hipMemsetAsync(L.prio_sum, 0, 8, b->stream)); /* (every launch counts from zero) */
  if (k) HIP_TRY(rs_jit_launch(k, &L, b->stream));
  else HIP_TRY(rs_launch_cells(&L, b->threads, b->stream));
  if (builtin_beside_jit) { const int rc = convert_tx(b, true); if (rc) return rc; }
  b->ttis_done += n_ttis;
  return RS_OK;
}

/* the layout check of the three *_create_checked functions (rs_batch_create_checked says why); `name`: the caller's config struct */
bool abi_matches(int abi_version, size_t cfg_size, size_t lib_size, const char* name) {
  if (abi_version == RS_ABI_VERSION && cfg_size == lib_size) return true;
  fail(RS_ERR_INVALID, "ABI mismatch: caller was built against ABI %d with an %s of %zu bytes, this library is ABI %d with %zu bytes", abi_version,
       name, cfg_size, RS_ABI_VERSION, lib_size);
  return false;
}

}  // namespace

extern "C" {

rs_batch* rs_batch_create(const rs_batch_config* cfg) { return batch_new(cfg, false); }

/* the same behind a deterministic layout check: the caller passes the ABI version and the struct size IT was compiled with
 * (RS_BATCH_CREATE in the header does); a caller built against another layout is refused instead of being read field-shifted */
rs_batch* rs_batch_create_checked(const rs_batch_config* cfg, int abi_version, size_t cfg_size) {
  return abi_matches(abi_version, cfg_size, sizeof(rs_batch_config), "rs_batch_config") ? rs_batch_create(cfg) : nullptr;
}

void rs_batch_destroy(rs_batch* b) {
  if (!b) return;
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  const hipStream_t own = b->own_stream ? b->stream : nullptr;
  delete b; /* every device array frees itself here (DevBuf), ahead of the stream as before */
  if (own) (void)hipStreamDestroy(own);
}

int rs_batch_seed(rs_batch* b, const uint32_t* seed, const int64_t* rand_skip) {
  if (!b || !seed) return fail(RS_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  if (b->ttis_done) return fail(RS_ERR_STATE, "rs_batch_seed after TTIs were run");
  return init_scalars(b, seed, rand_skip);
}

/* ---- per-cell configurations ---- */
static int check_slice_state(const rs_batch* b, const double* v, size_t cell, const double* weight = nullptr, int n_slices = -1); /* (the domain rule, stated at its definition below) */
int rs_batch_set_cell_configs(rs_batch* b, const double* slice_weight, const int32_t* algo_epsilon, const int32_t* algo_psi, const int32_t* user_to_slice) {
  return rs_batch_set_cell_configs_n(b, nullptr, slice_weight, algo_epsilon, algo_psi, user_to_slice);
}
int rs_batch_set_cell_configs_n(rs_batch* b, const int32_t* cell_slices, const double* slice_weight, const int32_t* algo_epsilon, const int32_t* algo_psi,
                                const int32_t* user_to_slice) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (b->direct) return fail(RS_ERR_INVALID, "per-cell configurations: not a batch");
  if (b->sched == RS_SCHED_NVS_NONGREEDY) return fail(RS_ERR_INVALID, "per-cell configurations: scheduler %d runs on another kernel, which reads one configuration", b->sched);
  if (b->queues) return fail(RS_ERR_STATE, "per-cell configurations: the batch has the queue model, which keeps one configuration for every cell");
  if (b->ttis_done) return fail(RS_ERR_STATE, "rs_batch_set_cell_configs after TTIs were run");
  const size_t cells = (size_t)b->n_cells, S = (size_t)b->S, U = (size_t)b->U;
  /* a NULL array: every cell keeps the shared configuration's values for that field */
  std::vector<double> w(cells * S);
  std::vector<int32_t> e(cells * S), ps(cells * S), us(cells * U), nu(cells), ns(cells, (int32_t)S);
  bool any_absent = false, any_fewer = false;
  /* a cell's slice count S_c: its rows' first S_c entries are its slices, the entries behind them belong to absent slices -- stored,
   * returned as given, not validated, ignored */
  for (size_t c = 0; c < cells && cell_slices; c++) {
    if (cell_slices[c] < 1 || cell_slices[c] > b->S)
      return fail(RS_ERR_INVALID, "cell %zu: cell_slices[%zu] = %d outside 1..%d (the batch's n_slices)", c, c, cell_slices[c], b->S);
    ns[c] = cell_slices[c];
    any_fewer |= ns[c] != b->S;
  }
  for (size_t c = 0; c < cells; c++) {
    for (size_t k = 0; k < S; k++) {
      w[c * S + k] = slice_weight ? slice_weight[c * S + k] : b->weight[k];
      e[c * S + k] = algo_epsilon ? algo_epsilon[c * S + k] : b->eps[k];
      ps[c * S + k] = algo_psi ? algo_psi[c * S + k] : b->psi[k];
    }
    for (size_t u = 0; u < U; u++) us[c * U + u] = user_to_slice ? user_to_slice[c * U + u] : b->u2s[u];
  }
  /* every row as validate() takes a configuration */
  for (size_t c = 0; c < cells; c++) {
    for (size_t k = 0; k < (size_t)ns[c]; k++) {
      if (!std::isfinite(w[c * S + k])) return fail(RS_ERR_INVALID, "cell %zu: slice_weight[%zu] = %g is not finite", c, k, w[c * S + k]);
      if ((e[c * S + k] | 1) != 1 || (ps[c * S + k] | 1) != 1)
        return fail(RS_ERR_INVALID, "cell %zu, slice %zu: algo_epsilon %d / algo_psi %d must be 0 or 1 in a batch", c, k, e[c * S + k], ps[c * S + k]);
    }
    /* a row's users, then -- a cell of fewer users than the batch's -- RS_USER_ABSENT to the end (the shared map has none) */
    size_t n = 0;
    for (size_t u = 0; u < U; u++) {
      const int32_t sl = us[c * U + u];
      if (sl == RS_USER_ABSENT && user_to_slice) {
        if (u == 0) return fail(RS_ERR_INVALID, "cell %zu, user 0: RS_USER_ABSENT -- a cell has at least one user (the absent users are a suffix of the row)", c);
        continue;
      }
      if (sl < 0 || sl >= b->S) return fail(RS_ERR_INVALID, "cell %zu, user %zu: slice %d out of range", c, u, sl);
      if (sl >= ns[c]) return fail(RS_ERR_INVALID, "cell %zu, user %zu: slice %d is absent -- the cell has %d slices (cell_slices[%zu])", c, u, sl, ns[c], c);
      if (n != u) return fail(RS_ERR_INVALID, "cell %zu, user %zu: slice %d behind RS_USER_ABSENT (user %zu) -- the absent users are a suffix of the row", c, u, sl, n);
      if (u && sl < us[c * U + u - 1]) return fail(RS_ERR_INVALID, "cell %zu: user_to_slice must be non-decreasing (user %zu)", c, u);
      n = u + 1;
    }
    nu[c] = (int32_t)n;
    any_absent |= n != U;
  }
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  { /* the slice state the cells hold now (zeros, or what rs_batch_write_state put there) against each cell's new weights */
    std::vector<double> st(b->d_sstate.count());
    HIP_TRY(b->d_sstate.download(st.data()));
    for (size_t c = 0; c < cells; c++)
      if (const int rc = check_slice_state(b, st.data() + c * S, c, w.data() + c * S, ns[c])) return rc;
  }
  /* one kernel serves all cells: LDS carve and run-time builds for the longest slice window of any cell -- validated and built BEFORE
   * the batch changes, so that a refusal leaves it as it was */
  int win = 0;
  for (size_t c = 0; c < cells; c++) win = std::max(win, map_window(us.data() + c * U, b->U));
  const RsCarve cv = rs_carve(b->S, b->U, b->R, b->sched, b->threads, 0, win, b->jit_wanted ? RS_NVS_WHOLE_SLICE : RS_NVS_WHOLE_SLICE_BUILTIN);
  if (cv.lds_bytes > 160 * 1024) return fail(RS_ERR_INVALID, "cell needs %d B of LDS with a slice window of %d users (> 160 KiB)", cv.lds_bytes, win);
  RsJitKernel* cjit = nullptr;
  char cmsg[sizeof b->jit_msg] = {0};
  if (b->jit_wanted) {
    BuildAs as;
    as.win = win;
    as.cell_cfg = cell_cfg_word(any_absent, any_fewer);
    cjit = batch_build(b, rs_batch::kGeneral, cmsg, sizeof cmsg, nullptr, as);
    if (cjit) snprintf(cmsg, sizeof cmsg, "%s", rs_jit_is_untuned(cjit) ? "in use, built WITHOUT the -mllvm tuning options (hiprtc refused them): a few per cent slower" : "");
    else if (!cmsg[0]) snprintf(cmsg, sizeof cmsg, "hiprtc build of the kernel with per-cell configurations failed");
    if (!cjit && b->threads > 512) return fail(RS_ERR_INVALID, "threads_per_cell %d needs the shape-specialised kernel with per-cell configurations: %s", b->threads, cmsg);
  }
  /* the four rows, all or none; a later call writes into them */
  if (!b->d_cc_weight) HIP_TRY(dev_alloc_all(b->d_cc_weight, cells * S, b->d_cc_eps, cells * S, b->d_cc_psi, cells * S, b->d_cc_user_slice, cells * U));
  std::vector<uint8_t> us8(cells * U);
  for (size_t i = 0; i < cells * U; i++) us8[i] = us[i] == RS_USER_ABSENT ? (uint8_t)RS_SLICE_ABSENT : (uint8_t)us[i];
  HIP_TRY(b->d_cc_weight.upload(w.data()));
  { /* the device row of eps carries the cell's slice count: RS_EPS_ABSENT from slice S_c on (the host row keeps what was given) */
    std::vector<int32_t> ed(e);
    for (size_t c = 0; c < cells; c++)
      for (size_t k = (size_t)ns[c]; k < S; k++) ed[c * S + k] = RS_EPS_ABSENT;
    HIP_TRY(b->d_cc_eps.upload(ed.data()));
  }
  HIP_TRY(b->d_cc_psi.upload(ps.data()));
  HIP_TRY(b->d_cc_user_slice.upload(us8.data()));
  /* commit: rows, launch block, carve and kernels together */
  b->cc_weight.swap(w); b->cc_eps.swap(e); b->cc_psi.swap(ps); b->cc_u2s.swap(us); b->cc_users.swap(nu); b->cc_slices.swap(ns);
  b->cell_cfg = true;
  b->ragged = any_absent;
  b->ragged_slices = any_fewer;
  b->base.weight = b->d_cc_weight; b->base.eps = b->d_cc_eps; b->base.psi = b->d_cc_psi; b->base.user_slice = b->d_cc_user_slice;
  b->base.cell_cfg = cell_cfg_word(any_absent, any_fewer);
  carve_lds(b, &b->base);
  /* the builds belong to the rows' window and to the switch: everything starts over with the new general build */
  if (b->jit_wanted) reset_builds(b, cjit, cmsg);
  return RS_OK;
}

int rs_batch_get_cell_config(rs_batch* b, int32_t cell, double* slice_weight, int32_t* algo_epsilon, int32_t* algo_psi, int32_t* user_to_slice) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (cell < 0 || cell >= b->n_cells) return fail(RS_ERR_INVALID, "cell %d outside 0..%d", cell, b->n_cells - 1);
  const size_t S = (size_t)b->S, U = (size_t)b->U, c = (size_t)cell;
  /* (a batch that was given no rows: every cell has the shared configuration's) */
  if (slice_weight) memcpy(slice_weight, b->cell_cfg ? b->cc_weight.data() + c * S : b->weight.data(), 8 * S);
  if (algo_epsilon) memcpy(algo_epsilon, b->cell_cfg ? b->cc_eps.data() + c * S : b->eps.data(), 4 * S);
  if (algo_psi) memcpy(algo_psi, b->cell_cfg ? b->cc_psi.data() + c * S : b->psi.data(), 4 * S);
  if (user_to_slice) memcpy(user_to_slice, b->cell_cfg ? b->cc_u2s.data() + c * U : b->u2s.data(), 4 * U);
  return RS_OK;
}

int rs_batch_cell_users(rs_batch* b, int32_t* n_users) {
  if (!b || !n_users) return fail(RS_ERR_INVALID, "null argument");
  if (b->direct) return fail(RS_ERR_INVALID, "cell users: not a batch");
  for (int c = 0; c < b->n_cells; c++) n_users[c] = b->cell_cfg ? b->cc_users[c] : b->U;
  return RS_OK;
}

int rs_batch_cell_slices(rs_batch* b, int32_t* n_slices) {
  if (!b || !n_slices) return fail(RS_ERR_INVALID, "null argument");
  if (b->direct) return fail(RS_ERR_INVALID, "cell slices: not a batch");
  for (int c = 0; c < b->n_cells; c++) n_slices[c] = b->cell_cfg ? b->cc_slices[c] : b->S;
  return RS_OK;
}

int rs_batch_slice_totals(rs_batch* b, int64_t* cum_bytes, int64_t* cum_rbs) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (b->direct) return fail(RS_ERR_INVALID, "slice totals: not a batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  if (!b->d_totals) HIP_TRY(b->d_totals.alloc(2 * b->d_sstate.count())); /* bytes and RBs, each [cells][S] */
  const size_t n = b->d_totals.count() / 2;
  HIP_TRY(rs_launch_slice_totals(b->d_cumb, b->d_cumr, b->cell_cfg ? b->d_cc_user_slice : b->d_user_slice, b->cell_cfg ? b->U : 0, b->n_cells, b->U, b->S,
                                 b->d_totals, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (cum_bytes) HIP_TRY(hipMemcpy(cum_bytes, b->d_totals, 8 * n, hipMemcpyDeviceToHost));
  if (cum_rbs) HIP_TRY(hipMemcpy(cum_rbs, b->d_totals + n, 8 * n, hipMemcpyDeviceToHost));
  return RS_OK;
}

/* ---- the CQI source: six setters, one sequence (cqi_replace) ---- */

/* the stride of one stored grid, the cell kernel's LDS image: RBG-major [R][Upad] with zero padding (a refresh is a straight copy) */
static size_t grid_stride_of(const rs_batch* b) { return (size_t)round_up(rs_upad_of(b->U) * b->R, 16); }

/* epoch grids from host memory [cells][n_epochs][U][R], and -- h_cqi_prb -- their per-PRB twin [cells][n_epochs][U][R * G] */
static int upload_epochs(rs_batch* b, const uint8_t* h_cqi, int32_t n_epochs, const uint8_t* h_cqi_prb) {
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  const size_t grid = (size_t)b->U * b->R, Upad = (size_t)rs_upad_of(b->U), stride = grid_stride_of(b);
  const size_t total = (size_t)b->n_cells * n_epochs;
  for (size_t i = 0; i < total * grid; i++)
    if (h_cqi[i] < 1 || h_cqi[i] > 15) return fail(RS_ERR_INVALID, "CQI %d at byte %zu outside 1..15", h_cqi[i], i);
  std::vector<uint8_t> packed(total * stride, 0), packed_prb;
  for (size_t g = 0; g < total; g++)
    for (size_t u = 0; u < (size_t)b->U; u++)
      for (size_t r = 0; r < (size_t)b->R; r++) packed[g * stride + r * Upad + u] = h_cqi[g * grid + u * b->R + r];
  const size_t grid_prb = grid * b->G, stride_prb = round_up((int)grid_prb, 16);
  if (h_cqi_prb) {
    packed_prb.assign(total * stride_prb, 0);
    for (size_t g = 0; g < total; g++) memcpy(&packed_prb[g * stride_prb], h_cqi_prb + g * grid_prb, grid_prb);
  }
  return cqi_replace(b, RS_CQI_EPOCHS, [&](rs_batch::CqiSource& q) -> int {
    HIP_TRY(q.epochs.assign(packed.data(), packed.size()));
    q.grid_stride = (int64_t)stride;
    q.n_epochs = n_epochs;
    if (!h_cqi_prb) return RS_OK;
    HIP_TRY(q.epochs_prb.assign(packed_prb.data(), packed_prb.size()));
    q.grid_stride_prb = (int64_t)stride_prb;
    return RS_OK;
  });
}

int rs_batch_upload_cqi_epochs(rs_batch* b, const uint8_t* h_cqi, int32_t n_epochs) {
  if (!b || !h_cqi || n_epochs < 1) return fail(RS_ERR_INVALID, "bad argument");
  return upload_epochs(b, h_cqi, n_epochs, nullptr);
}

int rs_batch_upload_cqi_epochs_prb(rs_batch* b, const uint8_t* h_cqi_prb, int32_t n_epochs) {
  if (!b || !h_cqi_prb || n_epochs < 1) return fail(RS_ERR_INVALID, "bad argument");
  const size_t per_user = (size_t)b->R * b->G, grid = (size_t)b->U * per_user, total = (size_t)b->n_cells * n_epochs;
  /* the metric reads the first PRB of every RBG (ref: downlink-transport-scheduler.cpp:536): the per-RBG grids the kernels keep in LDS */
  std::vector<uint8_t> rbg(total * b->U * b->R);
  for (size_t g = 0; g < total; g++)
    for (size_t u = 0; u < (size_t)b->U; u++)
      for (size_t r = 0; r < (size_t)b->R; r++) rbg[(g * b->U + u) * b->R + r] = h_cqi_prb[g * grid + u * per_user + r * b->G];
  for (size_t i = 0; i < total * grid; i++)
    if (h_cqi_prb[i] < 1 || h_cqi_prb[i] > 15) return fail(RS_ERR_INVALID, "CQI %d at byte %zu outside 1..15", h_cqi_prb[i], i);
  return upload_epochs(b, rbg.data(), n_epochs, h_cqi_prb);
}

int rs_batch_synthesize_cqi(rs_batch* b, uint64_t seed, const double* w, int32_t n_epochs) {
  return rs_batch_synthesize_cqi_at(b, seed, w, n_epochs, 0);
}

int rs_batch_synthesize_cqi_at(rs_batch* b, uint64_t seed, const double* w, int32_t n_epochs, int64_t first_cell) {
  if (!b || !w || n_epochs < 1 || first_cell < 0) return fail(RS_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  double tot = 0;
  for (int i = 0; i < 15; i++) {
    if (!(w[i] >= 0)) return fail(RS_ERR_INVALID, "negative CQI weight");
    tot += w[i];
  }
  if (!(tot > 0)) return fail(RS_ERR_INVALID, "all CQI weights are zero");
  uint32_t cdf[16];
  double acc = 0;
  for (int i = 0; i < 15; i++) {
    acc += w[i];
    double v = floor(acc / tot * 4294967296.0);
    cdf[i] = v >= 4294967295.0 ? 4294967295u : (uint32_t)v;
  }
  cdf[14] = 4294967295u;
  cdf[15] = 4294967295u;
  const size_t stride = grid_stride_of(b);
  return cqi_replace(b, RS_CQI_EPOCHS, [&](rs_batch::CqiSource& q) -> int {
    HIP_TRY(q.epochs.alloc((size_t)b->n_cells * n_epochs * stride));
    HIP_TRY(rs_launch_synth(q.epochs, (int64_t)stride, b->n_cells, n_epochs, b->U, b->R, rs_upad_of(b->U), seed, first_cell, cdf, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    q.grid_stride = (int64_t)stride;
    q.n_epochs = n_epochs;
    return RS_OK;
  });
}

int rs_batch_download_cqi_epochs(rs_batch* b, int32_t cell, uint8_t* h_cqi) {
  if (!b || !h_cqi || cell < 0 || cell >= b->n_cells) return fail(RS_ERR_INVALID, "bad argument");
  const rs_batch::CqiSource& q = b->cqi;
  if (q.mode != RS_CQI_EPOCHS) return fail(RS_ERR_STATE, "no epoch grids on the device");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  const size_t grid = (size_t)b->U * b->R, stride = (size_t)q.grid_stride;
  std::vector<uint8_t> tmp((size_t)q.n_epochs * stride);
  HIP_TRY(hipMemcpy(tmp.data(), q.epochs + (size_t)cell * q.n_epochs * stride, tmp.size(), hipMemcpyDeviceToHost));
  const size_t Upad = (size_t)rs_upad_of(b->U);
  for (int e = 0; e < q.n_epochs; e++) /* back to the caller's [U][R] order */
    for (size_t u = 0; u < (size_t)b->U; u++)
      for (size_t r = 0; r < (size_t)b->R; r++) h_cqi[e * grid + u * b->R + r] = tmp[e * stride + r * Upad + u];
  return RS_OK;
}

/* ---- CQI source A from device memory: rs_pack_cqi_kernel packs, checks and clamps on the batch's stream ---- */

/* d_cqi must be `want` bytes of device memory on the batch's device: asked of the runtime, nothing is read */
static int cqi_device_source(rs_batch* b, const uint8_t* d_cqi, size_t d_bytes, size_t want) {
  if (d_bytes != want) return fail(RS_ERR_INVALID, "d_bytes is %zu, the shape implies %zu", d_bytes, want);
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  hipError_t e = hipPointerGetAttributes(&at, d_cqi);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(RS_ERR_INVALID, "d_cqi is not device memory (hipPointerGetAttributes: %s): a host pointer?", hipGetErrorString(e));
  }
  if (at.type != hipMemoryTypeDevice || at.isManaged)
    return fail(RS_ERR_INVALID, "d_cqi is %s memory, not device memory", at.isManaged ? "managed" : "host");
  if (at.device != b->cfg.cell.device)
    return fail(RS_ERR_INVALID, "d_cqi is on device %d, the batch on device %d", at.device, b->cfg.cell.device);
  void* base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_cqi) != hipSuccess) (void)hipGetLastError();
  else if (d_cqi + d_bytes > (const uint8_t*)base + size)
    return fail(RS_ERR_INVALID, "d_cqi + d_bytes ends %zu bytes behind its allocation", (size_t)(d_cqi + d_bytes - ((const uint8_t*)base + size)));
  return RS_OK;
}

/* the pack of n source epochs into epochs (first + j) mod n_epochs of the grids `q`, enqueued; the error word is cleared ahead of the
 * first pack and after every report, and sticky in between */
static int cqi_pack(rs_batch* b, const rs_batch::CqiSource& q, const uint8_t* d_cqi, int32_t first, int32_t n) {
  if (!b->d_cqi_bad) HIP_TRY(b->d_cqi_bad.alloc(1));
  if (!b->cqi_bad_armed) {
    HIP_TRY(hipMemsetAsync(b->d_cqi_bad, 0xFF, 8, b->stream));
    b->cqi_bad_armed = true;
  }
  HIP_TRY(rs_launch_pack_cqi(d_cqi, q.epochs, b->d_cqi_bad, b->n_cells, n, first, q.n_epochs, b->U, b->R, rs_upad_of(b->U), q.grid_stride, b->stream));
  return RS_OK;
}

/* waits for the stream and reads the error word: RS_OK (*bad_byte = -1), or RS_ERR_INVALID with the word cleared and the batch
 * left without a CQI source (the stored values are clamped to CQI 1, not the caller's) */
static int cqi_report(rs_batch* b, int64_t* bad_byte, int32_t* bad_value) {
  HIP_TRY(hipStreamSynchronize(b->stream));
  unsigned long long w = ~0ull;
  if (b->d_cqi_bad && b->cqi_bad_armed) HIP_TRY(b->d_cqi_bad.download(&w));
  if (bad_byte) *bad_byte = -1;
  if (bad_value) *bad_value = 0;
  if (w == ~0ull) return RS_OK;
  HIP_TRY(hipMemsetAsync(b->d_cqi_bad, 0xFF, 8, b->stream));
  b->cqi.clear();
  if (bad_byte) *bad_byte = (int64_t)(w >> 8);
  if (bad_value) *bad_value = (int32_t)(w & 0xFF);
  return fail(RS_ERR_INVALID, "CQI %d at byte %lld outside 1..15", (int)(w & 0xFF), (long long)(w >> 8));
}

int rs_batch_set_cqi_epochs_device(rs_batch* b, const uint8_t* d_cqi, size_t d_bytes, int32_t n_epochs) {
  if (!b || !d_cqi || n_epochs < 1) return fail(RS_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  int rc = cqi_device_source(b, d_cqi, d_bytes, (size_t)b->n_cells * n_epochs * b->U * b->R);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  rc = cqi_replace(b, RS_CQI_EPOCHS, [&](rs_batch::CqiSource& q) -> int {
    HIP_TRY(q.epochs.alloc((size_t)b->n_cells * n_epochs * grid_stride_of(b)));
    q.grid_stride = (int64_t)grid_stride_of(b);
    q.n_epochs = n_epochs;
    return cqi_pack(b, q, d_cqi, 0, n_epochs);
  });
  return rc ? rc : cqi_report(b, nullptr, nullptr); /* (a value outside 1..15: the report leaves the batch without a source) */
}

int rs_batch_write_cqi_epochs_device(rs_batch* b, int32_t first_epoch, int32_t n, const uint8_t* d_cqi, size_t d_bytes, uint32_t flags) {
  if (!b || !d_cqi) return fail(RS_ERR_INVALID, "bad argument");
  if (flags & ~RS_CQI_WRITE_ASYNC) return fail(RS_ERR_INVALID, "unknown flags 0x%x", flags);
  const rs_batch::CqiSource& q = b->cqi;
  if (q.mode != RS_CQI_EPOCHS) return fail(RS_ERR_STATE, "no epoch grids on the device");
  if (q.epochs_prb) return fail(RS_ERR_STATE, "the batch has a per-PRB twin of its grids, which a write would leave behind");
  if (n < 1 || n > q.n_epochs) return fail(RS_ERR_INVALID, "n %d outside 1..%d", n, q.n_epochs);
  if (first_epoch < 0 || first_epoch >= q.n_epochs) return fail(RS_ERR_INVALID, "first_epoch %d outside 0..%d", first_epoch, q.n_epochs - 1);
  if (!b->cfg.cqi_epoch_wrap && first_epoch + n > q.n_epochs)
    return fail(RS_ERR_RANGE, "epochs %d..%d run past the last epoch %d (no cqi_epoch_wrap)", first_epoch, first_epoch + n - 1, q.n_epochs - 1);
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  int rc = cqi_device_source(b, d_cqi, d_bytes, (size_t)b->n_cells * n * b->U * b->R);
  if (rc) return rc;
  rc = cqi_pack(b, q, d_cqi, first_epoch, n);
  if (rc || (flags & RS_CQI_WRITE_ASYNC)) return rc;
  return cqi_report(b, nullptr, nullptr);
}

int rs_batch_cqi_write_status(rs_batch* b, int64_t* bad_byte, int32_t* bad_value) {
  if (!b || !bad_byte || !bad_value) return fail(RS_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  return cqi_report(b, bad_byte, bad_value);
}

int rs_batch_debug_cqi_image(rs_batch* b, int32_t cell, int32_t epoch, uint8_t* h_image, size_t bytes) {
  if (!b || !h_image || cell < 0 || cell >= b->n_cells) return fail(RS_ERR_INVALID, "bad argument");
  const rs_batch::CqiSource& q = b->cqi;
  if (q.mode != RS_CQI_EPOCHS) return fail(RS_ERR_STATE, "no epoch grids on the device");
  if (epoch < 0 || epoch >= q.n_epochs) return fail(RS_ERR_INVALID, "epoch %d outside 0..%d", epoch, q.n_epochs - 1);
  if (bytes != (size_t)q.grid_stride) return fail(RS_ERR_INVALID, "bytes is %zu, a grid's image has %lld", bytes, (long long)q.grid_stride);
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(h_image, q.epochs + ((size_t)cell * q.n_epochs + epoch) * bytes, bytes, hipMemcpyDeviceToHost));
  return RS_OK;
}

/* trace tables from host memory [n_traces][n_rows][R] with every user's trace id, and -- h_trace_prb -- their per-PRB twin */
static int upload_trace(rs_batch* b, const uint8_t* h_trace, int32_t n_traces, int32_t n_rows, int32_t row_modulus, const int32_t* h_user_trace,
                        const uint8_t* h_trace_prb) {
  if (!b || !h_trace || !h_user_trace || n_traces < 1 || n_rows < 1 || row_modulus < 1)
    return fail(RS_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  const size_t tb = (size_t)n_traces * n_rows * b->R;
  for (size_t i = 0; i < tb; i++)
    if (h_trace[i] < 1 || h_trace[i] > 15) return fail(RS_ERR_INVALID, "trace CQI %d outside 1..15", h_trace[i]);
  const size_t nu = (size_t)b->n_cells * b->U;
  for (size_t i = 0; i < nu; i++)
    if (h_user_trace[i] < 0 || h_user_trace[i] >= n_traces) return fail(RS_ERR_INVALID, "trace id %d out of range", h_user_trace[i]);
  return cqi_replace(b, RS_CQI_TRACE, [&](rs_batch::CqiSource& q) -> int {
    HIP_TRY(q.trace.assign(h_trace, tb));
    HIP_TRY(q.user_trace.assign(h_user_trace, nu));
    q.n_traces = n_traces; q.n_rows = n_rows; q.row_mod = row_modulus;
    if (h_trace_prb) HIP_TRY(q.trace_prb.assign(h_trace_prb, tb * b->G));
    return RS_OK;
  });
}

int rs_batch_set_trace(rs_batch* b, const uint8_t* h_trace, int32_t n_traces, int32_t n_rows, int32_t row_modulus,
                       const int32_t* h_user_trace) {
  return upload_trace(b, h_trace, n_traces, n_rows, row_modulus, h_user_trace, nullptr);
}

int rs_batch_set_trace_prb(rs_batch* b, const uint8_t* h_trace_prb, int32_t n_traces, int32_t n_rows, int32_t row_modulus,
                           const int32_t* h_user_trace) {
  if (!b || !h_trace_prb || n_traces < 1 || n_rows < 1) return fail(RS_ERR_INVALID, "bad argument");
  const size_t per_row = (size_t)b->R * b->G, rows = (size_t)n_traces * n_rows;
  for (size_t i = 0; i < rows * per_row; i++)
    if (h_trace_prb[i] < 1 || h_trace_prb[i] > 15) return fail(RS_ERR_INVALID, "trace CQI %d outside 1..15", h_trace_prb[i]);
  std::vector<uint8_t> rbg(rows * b->R);
  for (size_t q = 0; q < rows; q++)
    for (size_t r = 0; r < (size_t)b->R; r++) rbg[q * b->R + r] = h_trace_prb[q * per_row + r * b->G];
  return upload_trace(b, rbg.data(), n_traces, n_rows, row_modulus, h_user_trace, h_trace_prb);
}

int rs_batch_run_async(rs_batch* b, int32_t n_ttis) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  return launch(b, LaunchReq(n_ttis));
}

int rs_batch_sync(rs_batch* b) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return check_device_err(b);
}

int rs_batch_run(rs_batch* b, int32_t n_ttis) {
  int rc = rs_batch_run_async(b, n_ttis);
  if (rc) return rc;
  return rs_batch_sync(b);
}

int rs_batch_run_logged(rs_batch* b, int32_t n_ttis, int16_t* h_map, int32_t* h_tbs, int16_t* h_quota,
                        int16_t* h_target, int32_t* h_uinfo) {
  rs_batch_log lg;
  memset(&lg, 0, sizeof lg);
  lg.rbg_to_user = h_map; lg.tbs_bits = h_tbs; lg.quota = h_quota; lg.target = h_target; lg.uinfo = h_uinfo;
  return rs_batch_run_logged_ex(b, n_ttis, &lg);
}

int rs_batch_run_logged_ex(rs_batch* b, int32_t n_ttis, const rs_batch_log* lg) { return rs_batch_run_logged_bearers(b, n_ttis, lg, nullptr); }

int rs_batch_run_logged_bearers(rs_batch* b, int32_t n_ttis, const rs_batch_log* lg, const rs_batch_bearer_log* blg) {
  if (!b || !lg) return fail(RS_ERR_INVALID, "null argument");
  const bool bearers = blg && (blg->bytes || blg->hol_delay);
  if (bearers && !b->queues) return fail(RS_ERR_STATE, "per-bearer log rows: the batch has no bearers (rs_batch_set_bearers)");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  if (n_ttis < 1) return fail(RS_ERR_INVALID, "n_ttis %d < 1", n_ttis);
  const bool transport = b->sched == RS_SCHED_SEQUENTIAL || b->sched == RS_SCHED_MAXCELL || b->sched == RS_SCHED_UPPERBOUND ||
                         b->sched == RS_SCHED_SUBOPT || b->sched == RS_SCHED_VOGEL;
  if (lg->slice_keys && !transport) return fail(RS_ERR_INVALID, "slice_keys: only the DownlinkTransportScheduler policies have them");
  const size_t rows = (size_t)b->n_cells * n_ttis;
  int16_t *d_map = nullptr, *d_quota = nullptr, *d_target = nullptr;
  int32_t *d_tbs = nullptr, *d_uinfo = nullptr;
  uint32_t* d_keys = nullptr;
  ScratchBuffers scratch;
  HIP_TRY(scratch.alloc(&d_map, 2 * rows * b->R));
  HIP_TRY(scratch.alloc(&d_quota, 2 * rows * b->S));
  HIP_TRY(scratch.alloc(&d_target, 2 * rows * b->S));
  HIP_TRY(scratch.alloc(&d_tbs, 4 * rows * b->U));
  HIP_TRY(scratch.alloc(&d_uinfo, 4 * rows * b->U));
  if (lg->slice_keys) HIP_TRY(scratch.alloc(&d_keys, 4 * rows * b->R * b->S));
  HIP_TRY(hipMemsetAsync(d_tbs, 0, 4 * rows * b->U, b->stream));
  HIP_TRY(hipMemsetAsync(d_uinfo, 0, 4 * rows * b->U, b->stream));
  int32_t* d_bbytes = nullptr;
  double* d_bhol = nullptr;
  if (bearers) {
    HIP_TRY(scratch.alloc(&d_bbytes, 4 * rows * b->U * 2));
    HIP_TRY(scratch.alloc(&d_bhol, 8 * rows * b->U * 2));
    HIP_TRY(hipMemsetAsync(d_bbytes, 0, 4 * rows * b->U * 2, b->stream));
    HIP_TRY(hipMemsetAsync(d_bhol, 0, 8 * rows * b->U * 2, b->stream));
  }
  LaunchReq rq(n_ttis);
  rq.map = d_map; rq.quota = d_quota; rq.target = d_target; rq.tbs = d_tbs; rq.uinfo = d_uinfo; rq.keys = d_keys;
  rq.bbytes = d_bbytes; rq.bhol = d_bhol;
  int rc = launch(b, rq);
  if (!rc) rc = rs_batch_sync(b);
  if (!rc) {
    if (lg->rbg_to_user) HIP_TRY(hipMemcpy(lg->rbg_to_user, d_map, 2 * rows * b->R, hipMemcpyDeviceToHost));
    if (lg->quota) HIP_TRY(hipMemcpy(lg->quota, d_quota, 2 * rows * b->S, hipMemcpyDeviceToHost));
    if (lg->target) HIP_TRY(hipMemcpy(lg->target, d_target, 2 * rows * b->S, hipMemcpyDeviceToHost));
    if (lg->tbs_bits) HIP_TRY(hipMemcpy(lg->tbs_bits, d_tbs, 4 * rows * b->U, hipMemcpyDeviceToHost));
    if (lg->uinfo) HIP_TRY(hipMemcpy(lg->uinfo, d_uinfo, 4 * rows * b->U, hipMemcpyDeviceToHost));
    if (lg->slice_keys) HIP_TRY(hipMemcpy(lg->slice_keys, d_keys, 4 * rows * b->R * b->S, hipMemcpyDeviceToHost));
    if (bearers && blg->bytes) HIP_TRY(hipMemcpy(blg->bytes, d_bbytes, 4 * rows * b->U * 2, hipMemcpyDeviceToHost));
    if (bearers && blg->hol_delay) HIP_TRY(hipMemcpy(blg->hol_delay, d_bhol, 8 * rows * b->U * 2, hipMemcpyDeviceToHost));
  }
  return rc;
}

/* What rs_batch_run_records and rs_batch_run_grant_records share: a launch of n_ttis TTIs that writes records of rec_size bytes, at most
 * `bound` per cell and TTI, into the batch's device block, and the copy back into the caller's lists (cap places per cell); `what` opens
 * the messages.  The lists come back unsorted.  A wait that ended in a range error (`rc`) and a cell that counted more than its list
 * holds (`over`) are the caller's to report, once the lists are complete. */
struct RecordsRun {
  std::vector<uint32_t> count;    /* per cell, as the device counted */
  int64_t cap_dev = 0, over = -1; /* one cell's places in the device block; the first cell that counted more (-1: none) */
  int rc = RS_OK;
  std::chrono::steady_clock::time_point t0, t1, t2; /* before the launch, after the wait, after the copy back */
  size_t used(size_t c) const { return (size_t)std::min((int64_t)count[c], cap_dev); }
};
static int run_with_records(rs_batch* b, int n_ttis, int64_t cap, int bound, size_t rec_size, const char* what, void* recs, int64_t* n_recs,
                            RecordsRun* out) {
  /* the device block: no cell can count more than n_ttis * bound, so a larger capacity of the caller's needs no larger list there */
  const size_t cells = (size_t)b->n_cells;
  const int64_t cap_dev = out->cap_dev = std::min(cap, (int64_t)n_ttis * bound);
  const size_t list_bytes = cells * (size_t)cap_dev * rec_size, need = list_bytes + 4 * cells;
  if (need > b->d_recs.bytes()) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->d_recs.release(); /* (the old block first: the two together may be more than the device has) */
    /* RS_RECORDS_MAX_BYTES: the largest device block a call may ask for (unset: what the device gives).  A block above it is a failed
     * allocation, by the very path of one: it is how the tests reach this refusal without asking a card for memory it does not have. */
    const char* const e_max = getenv("RS_RECORDS_MAX_BYTES");
    const bool too_large = e_max && (unsigned long long)need > strtoull(e_max, nullptr, 10);
    if (too_large || b->d_recs.alloc(need) != hipSuccess) {
      if (!too_large) (void)hipGetLastError();
      return fail(RS_ERR_HIP, "%s: no device block of %zu bytes (%zu cells x %lld records)", what, need, cells, (long long)cap_dev);
    }
  }
  uint32_t* const d_count = (uint32_t*)(b->d_recs + list_bytes);
  HIP_TRY(hipMemsetAsync(d_count, 0, 4 * cells, b->stream));
  out->t0 = std::chrono::steady_clock::now();
  LaunchReq rq(n_ttis);
  rq.recs = b->d_recs.get();
  rq.rec_cap = cap_dev;
  int rc = launch(b, rq);
  if (rc) return rc;
  rc = out->rc = rs_batch_sync(b);
  if (rc == RS_ERR_HIP) return rc;
  out->t1 = std::chrono::steady_clock::now();
  /* the copy back: the counts, then of every list the places that were written (copies queued on the stream, one wait) */
  out->count.resize(cells);
  HIP_TRY(hipMemcpy(out->count.data(), d_count, 4 * cells, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < cells; c++) {
    n_recs[c] = (int64_t)out->count[c];
    if (n_recs[c] > cap_dev && out->over < 0) out->over = (int64_t)c; /* (cap_dev < cap only where nothing can exceed it) */
    if (out->used(c))
      HIP_TRY(hipMemcpyAsync((char*)recs + c * (size_t)cap * rec_size, b->d_recs + c * (size_t)cap_dev * rec_size, out->used(c) * rec_size,
                             hipMemcpyDeviceToHost, b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  out->t2 = std::chrono::steady_clock::now();
  return RS_OK;
}

/* most bearers DoStopSchedule can credit in one TTI of one cell.  A credit needs a grant and a grant needs an RBG.
 * Scheduler 1 gives an RBG to one FLOW (a bearer): min(2 U, R).  The transport schedulers and NVS give it to one USER, whose grant
 * DoStopSchedule splits over at most its two bearers: 2 min(U, R). */
int rs_batch_record_bound(rs_batch* b) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (!b->queues) return fail(RS_ERR_STATE, "bearer records: the batch has no queue model (rs_batch_set_bearers / rs_batch_set_arrivals)");
  return b->sched == RS_SCHED_PF ? std::min(2 * b->U, b->R) : 2 * std::min(b->U, b->R);
}

int rs_batch_run_records(rs_batch* b, int32_t n_ttis, int64_t cap, rs_bearer_record* recs, int64_t* n_recs) {
  static_assert(sizeof(rs_bearer_record) == sizeof(RsBearerRecord) && offsetof(rs_bearer_record, hol_delay) == offsetof(RsBearerRecord, hol_delay),
                "the device writes the ABI's record");
  if (!b || !recs || !n_recs) return fail(RS_ERR_INVALID, "null argument");
  if (cap < 1) return fail(RS_ERR_INVALID, "cap %lld < 1", (long long)cap);
  if (n_ttis < 1) return fail(RS_ERR_INVALID, "n_ttis %d < 1", n_ttis);
  if (n_ttis > RS_MAX_TTIS_PER_LAUNCH) return fail(RS_ERR_INVALID, "runs with records are limited to %d TTIs per call", RS_MAX_TTIS_PER_LAUNCH);
  if (!b->queues || !b->d_arr_off)
    return fail(RS_ERR_STATE, "bearer records: the batch has no queue model (rs_batch_set_bearers / rs_batch_set_arrivals)");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  RecordsRun run;
  if (const int rc = run_with_records(b, n_ttis, cap, rs_batch_record_bound(b), sizeof(RsBearerRecord), "bearer records", recs, n_recs, &run)) return rc;
  const size_t cells = (size_t)b->n_cells;
  /* BearerLogWriter's order: TTI, user, then the reference's loop over the user's bearers -- priority 1 first in DoStopSchedule of the
   * transport schedulers and NVS (downlink-transport-scheduler.cpp:179), flow 0 first in DL_PF's FlowsToSchedule.  A (TTI, user, bearer)
   * occurs once, so the result does not depend on the order the device handed the places out in.  The device hands out all places of
   * TTI k before any of TTI k + 1 (rs_phase_queues.inc), and inside a TTI nearly in user order: an insertion sort per TTI's stretch, a
   * few dozen records that are almost in place; a list whose TTIs do not ascend -- it would mean that guarantee broke -- is sorted in full. */
  const bool pf = b->sched == RS_SCHED_PF;
  auto key = [pf](const rs_bearer_record& x) { return ((uint64_t)(uint32_t)x.user << 1) | (uint64_t)(pf ? x.bearer : 1 - x.bearer); };
  for (size_t c = 0; c < cells; c++) {
    rs_bearer_record* const r = recs + c * (size_t)cap;
    const size_t n = run.used(c);
    bool ascending = true;
    for (size_t i = 0, j; i < n; i = j) {
      if (i && r[i].tti < r[i - 1].tti) ascending = false;
      for (j = i + 1; j < n && r[j].tti == r[i].tti; j++) {
        const rs_bearer_record x = r[j];
        size_t k = j;
        for (; k > i && key(r[k - 1]) > key(x); k--) r[k] = r[k - 1];
        r[k] = x;
      }
    }
    if (!ascending)
      std::sort(r, r + n, [&key](const rs_bearer_record& x, const rs_bearer_record& y) { return x.tti != y.tti ? x.tti < y.tti : key(x) < key(y); });
  }
  if (run.rc) return run.rc;
  if (run.over >= 0)
    return fail(RS_ERR_RANGE, "bearer records: cell %lld credited %lld bearers in these %d TTIs, the lists hold %lld (state, flow record and the other cells' lists are complete)",
                (long long)run.over, (long long)n_recs[run.over], n_ttis, (long long)cap);
  return RS_OK;
}

int rs_batch_grant_bound(rs_batch* b) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (b->queues) return fail(RS_ERR_STATE, "grant records: the batch has the queue model, whose records are the bearers' (rs_batch_record_bound / rs_batch_run_records)");
  if (b->sched == RS_SCHED_NVS_NONGREEDY) return fail(RS_ERR_INVALID, "grant records: scheduler %d runs on another kernel, which writes none", b->sched);
  return grant_bound(b);
}

int rs_batch_run_grant_records(rs_batch* b, int32_t n_ttis, int64_t cap, rs_batch_grant_record* recs, int64_t* n_recs) {
  static_assert(sizeof(rs_batch_grant_record) == sizeof(RsBatchGrantRecord) && offsetof(rs_batch_grant_record, rbg_mask) == offsetof(RsBatchGrantRecord, rbg_mask) &&
                    offsetof(rs_batch_grant_record, nprb) == offsetof(RsBatchGrantRecord, nprb) && offsetof(rs_batch_grant_record, mcs) == offsetof(RsBatchGrantRecord, mcs),
                "the device writes the ABI's record");
  if (!b || !recs || !n_recs) return fail(RS_ERR_INVALID, "null argument");
  if (cap < 1) return fail(RS_ERR_INVALID, "cap %lld < 1", (long long)cap);
  if (n_ttis < 1) return fail(RS_ERR_INVALID, "n_ttis %d < 1", n_ttis);
  if (n_ttis > RS_MAX_TTIS_PER_LAUNCH) return fail(RS_ERR_INVALID, "runs with records are limited to %d TTIs per call", RS_MAX_TTIS_PER_LAUNCH);
  if (b->queues) return fail(RS_ERR_STATE, "grant records: the batch has the queue model, whose records are the bearers' (rs_batch_run_records)");
  if (b->sched == RS_SCHED_NVS_NONGREEDY) return fail(RS_ERR_INVALID, "grant records: scheduler %d runs on another kernel, which writes none", b->sched);
  if (b->direct) return fail(RS_ERR_INVALID, "grant records: not a batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  RecordsRun run;
  if (const int rc = run_with_records(b, n_ttis, cap, grant_bound(b), sizeof(RsBatchGrantRecord), "grant records", recs, n_recs, &run)) return rc;
  const size_t cells = (size_t)b->n_cells;
  {
    /* the cells' lists are sorted side by side: up to 8 host threads (RS_RECORDS_SORT_THREADS; 1: on the caller's thread) */
    const char* const e_thr = getenv("RS_RECORDS_SORT_THREADS");
    size_t n_thr = e_thr ? (size_t)std::max(1, atoi(e_thr)) : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
    size_t total = 0;
    for (size_t c = 0; c < cells; c++) total += run.used(c);
    if (total < 65536) n_thr = 1; /* (a thread's start costs more than sorting a few thousand records) */
    n_thr = std::min(n_thr, cells);
    const auto work = [&](size_t first) {
      for (size_t c = first; c < cells; c += n_thr) sort_grant_records(recs + c * (size_t)cap, run.used(c));
    };
    std::vector<std::thread> pool;
    for (size_t k = 1; k < n_thr; k++) pool.emplace_back(work, k);
    work(0);
    for (std::thread& th : pool) th.join();
  }
  if (getenv("RS_RECORDS_TIMING")) { /* where a call's time goes (tools/bench_grant_records.py, profiles/batch_grant_records.md) */
    const auto ms = [](auto a, auto z) { return std::chrono::duration<double, std::milli>(z - a).count(); };
    fprintf(stderr, "rs_batch_run_grant_records: launch and wait %.3f ms, copy back %.3f ms, host sort %.3f ms\n", ms(run.t0, run.t1), ms(run.t1, run.t2), ms(run.t2, std::chrono::steady_clock::now()));
  }
  if (run.rc) return run.rc;
  if (run.over >= 0)
    return fail(RS_ERR_RANGE, "grant records: cell %lld counted %lld grants in these %d TTIs, the lists hold %lld (state and the other cells' lists are complete)",
                (long long)run.over, (long long)n_recs[run.over], n_ttis, (long long)cap);
  return RS_OK;
}

int rs_batch_run_timed(rs_batch* b, int32_t n_ttis, int32_t launches, float* ms) {
  if (!b || !ms || launches < 1) return fail(RS_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  ScratchEvents events;
  HIP_TRY(events.create(launches + 1));
  std::vector<hipEvent_t>& ev = events.ev;
  int rc = RS_OK;
  HIP_TRY(hipEventRecord(ev[0], b->stream));
  for (int i = 0; i < launches && !rc; i++) {
    rc = launch(b, LaunchReq(n_ttis));
    if (!rc) HIP_TRY(hipEventRecord(ev[i + 1], b->stream));
  }
  if (!rc) rc = rs_batch_sync(b);
  if (!rc)
    for (int i = 0; i < launches; i++) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  return rc;
}

int rs_batch_read_state(rs_batch* b, double* avg, int64_t* cum_bytes, int64_t* cum_rbs, double* slice_state) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (avg) HIP_TRY(b->d_avg.download(avg));
  if (cum_bytes) HIP_TRY(b->d_cumb.download(cum_bytes));
  if (cum_rbs) HIP_TRY(b->d_cumr.download(cum_rbs));
  if (slice_state) HIP_TRY(b->d_sstate.download(slice_state));
  return RS_OK;
}

/* The domain of slice state that comes from outside (rs_set_slice_offset, rs_group_set_slice_offset, rs_batch_write_state;
 * include/radiosaber_hip.h states it), one cell's S values at a time.
 *   every scheduler: finite values.
 *   transport schedulers: every surface hands targets and quotas out as int16 (RsLaunch::log_target / log_quota: the drop-in and
 *     group outputs too), so |target| and |quota| must stay below 2^15.  With W = nb_rbs * (1 + sum |w|) and A = sum |offset|:
 *     in the call that reads the offsets |raw target| <= nb_rbs |w| + |offset|, |extra_rbs| <= W + A and every target lies within
 *     W + A; afterwards |offset'| <= |target| + nb_rbs, the offsets sum to the PRBs of the RBGs left unallocated, so |extra_rbs| <=
 *     W + nb_rbs and the next targets lie within A + 4 W; from there the offsets move toward the weights' shares.  Hence the rule
 *     5 W + A < 2^15.  It also keeps the numerators of the quota step's idiv_small (rs_wave.h; measured in tests/test_quota_edge_inputs.py: C
 *     division below 2^25 + 2, wrong at 2^25 + 2) a factor of a thousand inside that bound.
 *   schedulers 7 and 11: EWMAs are >= 0.  The reference's scan ('>=' from 0, :127-131) never picks a negative score and the
 *     kernel's integer-pair maximum orders negative doubles the other way round. */
static int check_slice_state(const rs_batch* b, const double* v, size_t cell, const double* weight, int n_slices) {
  if (!weight) weight = b->cell_cfg ? b->cc_weight.data() + cell * (size_t)b->S : b->weight.data(); /* (per-cell rows: the cell's own weights) */
  /* (a cell of fewer slices than the batch: the rule covers its own slices; an absent slice's word is stored as given and never read) */
  const int S = n_slices > 0 ? n_slices : (b->cell_cfg && !b->cc_slices.empty()) ? b->cc_slices[cell] : b->S;
  const bool transport = b->sched == RS_SCHED_SEQUENTIAL || b->sched == RS_SCHED_MAXCELL || b->sched == RS_SCHED_SUBOPT ||
                         b->sched == RS_SCHED_VOGEL || b->sched == RS_SCHED_UPPERBOUND;
  const bool nvs = b->sched == RS_SCHED_NVS || b->sched == RS_SCHED_NVS_NONGREEDY;
  const double nb = (double)b->R * b->G;
  double w = nb, a = 0;
  for (int s = 0; s < S; s++) {
    if (!std::isfinite(v[s])) return fail(RS_ERR_INVALID, "slice state [%zu][%d] = %g is not finite", cell, s, v[s]);
    if (nvs && !(v[s] >= 0)) return fail(RS_ERR_INVALID, "slice EWMA [%zu][%d] = %g is negative (slice_ewma_time_ is an average of 0s and 1s)", cell, s, v[s]);
    w += nb * fabs(weight[s]);
    a += fabs(v[s]);
  }
  if (transport && !(5 * w + a < 32768.0))
    return fail(RS_ERR_INVALID, "slice offsets of cell %zu: 5 nb_rbs (1 + sum |weight|) + sum |offset| = %g, at or above 2^15 = 32768: targets and "
                "quotas are handed out as int16 (and the quota step's divisions are exact for numerators below 2^25 + 2 only)", cell, 5 * w + a);
  return RS_OK;
}

/* the inverse of rs_batch_read_state for the two arrays a restart needs set: PF averages (RadioBearer::m_averageTransmissionRate,
 * ref: src/flows/radio-bearer.cpp:54 starts them at 100 000) and slice_rbs_offset_ / slice_ewma_time_ */
int rs_batch_write_state(rs_batch* b, const double* avg, const double* slice_state) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (b->direct) return fail(RS_ERR_INVALID, "drop-in contexts take the averages per call");
  if (b->queues) return fail(RS_ERR_STATE, "the queue model keeps one average per bearer: not settable through this call");
  if (avg)
    for (size_t i = 0; i < b->d_avg.count(); i++)
      if (!(avg[i] >= 1.0) || !(avg[i] <= 1e300)) return fail(RS_ERR_INVALID, "avg_rate[%zu] = %g: the EWMA keeps averages at or above 1 (radio-bearer.cpp:160-162)", i, avg[i]);
  if (slice_state)
    for (int c = 0; c < b->n_cells; c++)
      if (const int rc = check_slice_state(b, slice_state + (size_t)c * b->S, (size_t)c)) return rc;
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (avg) HIP_TRY(b->d_avg.upload(avg));
  if (slice_state) HIP_TRY(b->d_sstate.upload(slice_state));
  return RS_OK;
}

/* ---- finite queues ---- */
int rs_batch_set_bearers(rs_batch* b, const uint8_t* bearer_kind) {
  if (!b || !bearer_kind) return fail(RS_ERR_INVALID, "null argument");
  if (b->direct) return fail(RS_ERR_INVALID, "drop-in contexts take the queue state per TTI (rs_tti_in.hol_delay / prio_has_data)");
  if (b->ttis_done) return fail(RS_ERR_STATE, "rs_batch_set_bearers after TTIs were run");
  if (b->cell_cfg) return fail(RS_ERR_STATE, "rs_batch_set_bearers after rs_batch_set_cell_configs: the queue model keeps one configuration for every cell");
  if (b->sched != RS_SCHED_SEQUENTIAL && b->sched != RS_SCHED_MAXCELL && b->sched != RS_SCHED_SUBOPT && b->sched != RS_SCHED_VOGEL &&
      b->sched != RS_SCHED_PF && b->sched != RS_SCHED_NVS)
    return fail(RS_ERR_INVALID, "finite queues: schedulers 1, 7, 8, 9, 101 and 103 only (sched %d)", b->sched);
  const size_t U = b->U;
  for (size_t u = 0; u < U; u++) {
    for (int k = 0; k < 2; k++)
      if (bearer_kind[u * 2 + k] > 2) return fail(RS_ERR_INVALID, "bearer kind %d of user %zu", bearer_kind[u * 2 + k], u);
    if (!bearer_kind[u * 2] && !bearer_kind[u * 2 + 1]) return fail(RS_ERR_INVALID, "user %zu has no bearer", u);
  }
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  /* validate the queue model's LDS carve and build its kernel BEFORE the batch changes: on failure it stays as it was */
  /* Where the bearers' hot words live (RS_QSTATE_BYTES_PER_USER per user).  LDS when they fit the CU's 160 KB -- measured on
   * exp-customize-20slices x 512 cells (profiles/r03_queue_mode.md) -- unless that is what pushes the cell over 80 KB while the
   * batch has more cells than the chip has CUs: then residency would halve the cells per CU, and the words stay in HBM.
   * rs_batch_config.queue_state_lds overrides (1: LDS whenever it fits, -1: HBM). */
  int qmode = 2;
  {
    const RsCarve lds_c = rs_carve(b->S, b->U, b->R, b->sched, b->threads, 2), hbm_c = rs_carve(b->S, b->U, b->R, b->sched, b->threads, 3);
    const bool halves = lds_c.q_lds && lds_c.lds_bytes > 80 * 1024 && hbm_c.lds_bytes <= 80 * 1024 && b->n_cells > device_cus(b->cfg.cell.device);
    if (b->cfg.queue_state_lds < 0 || (b->cfg.queue_state_lds == 0 && halves)) qmode = 3;
    const RsCarve qc = qmode == 2 ? lds_c : hbm_c;
    if (qc.lds_bytes > 160 * 1024) return fail(RS_ERR_INVALID, "cell needs %d B of LDS with the queue model (> 160 KiB)", qc.lds_bytes);
  }
  RsJitKernel* qjit = nullptr;
  char qmsg[sizeof b->jit_msg] = {0};
  if (b->jit_wanted) { /* the shape-specialised kernel of the queue model is a different code object */
    BuildAs as;
    as.qmode = qmode;
    qjit = batch_build(b, rs_batch::kGeneral, qmsg, sizeof qmsg, nullptr, as);
    if (!qjit && !qmsg[0]) snprintf(qmsg, sizeof qmsg, "hiprtc build of the queue-model kernel failed");
    if (!qjit && b->threads > 512) return fail(RS_ERR_INVALID, "threads_per_cell %d needs the shape-specialised queue-model kernel: %s", b->threads, qmsg);
  }
  /* the six queue arrays, all or none (still before the batch changes); a later call writes into them.  nu: one [cells][U] array of
   * per-user words, n: one [cells][2][U] array of per-bearer words */
  const size_t nu = (size_t)b->n_cells * U, n = 2 * nu;
  if (!b->d_bearer_kind)
    HIP_TRY(dev_alloc_all(b->d_bearer_kind, 2 * U, b->d_qi, 7 * n, b->d_bavg, n, b->d_bcum, 2 * n, b->d_qflags, nu, b->d_qhol, nu));
  HIP_TRY(b->d_bearer_kind.upload(bearer_kind));
  HIP_TRY(b->d_qi.zero());
  HIP_TRY(b->d_bcum.zero());
  HIP_TRY(b->d_qflags.zero());
  HIP_TRY(b->d_qhol.zero());
  const std::vector<double> avg(n, 100000.0); /* radio-bearer.cpp:54 */
  HIP_TRY(b->d_bavg.upload(avg.data()));
  /* commit: mode, carve and kernel together (the queue = 0 kernel must never run with queue arguments) */
  b->queues = true;
  b->qmode = qmode;
  carve_lds(b, &b->base); /* schedulers 1 and 7 keep per-bearer scratch in LDS in this mode */
  /* the queue-model build is another code object: what an earlier self-check (rs_batch_prepare_launch) found says nothing about it, and
   * its lean build is compiled on demand */
  if (b->jit_wanted) reset_builds(b, qjit, qmsg);
  return RS_OK;
}

int rs_batch_set_arrivals(rs_batch* b, const int64_t* offsets, const double* time, const int32_t* n_full, const int32_t* last_bytes) {
  if (!b || !offsets) return fail(RS_ERR_INVALID, "null argument");
  if (!b->queues) return fail(RS_ERR_STATE, "rs_batch_set_bearers first");
  if (b->ttis_done) return fail(RS_ERR_STATE, "rs_batch_set_arrivals after TTIs were run");
  const size_t nb = (size_t)b->n_cells * b->U * 2;
  if (offsets[0] != 0) return fail(RS_ERR_INVALID, "offsets[0] must be 0");
  for (size_t i = 0; i < nb; i++) {
    if (offsets[i + 1] < offsets[i]) return fail(RS_ERR_INVALID, "offsets must not decrease (bearer %zu)", i);
    for (int64_t k = offsets[i]; k < offsets[i + 1]; k++) {
      if (k > offsets[i] && !(time[k] >= time[k - 1])) return fail(RS_ERR_INVALID, "arrival times of bearer %zu are not ascending", i);
      if (n_full[k] < 0 || last_bytes[k] < 0 || last_bytes[k] > RS_FULL_PACKET || n_full[k] + last_bytes[k] == 0)
        return fail(RS_ERR_INVALID, "burst %lld of bearer %zu: n_full %d, last %d", (long long)k, i, n_full[k], last_bytes[k]);
    }
  }
  const size_t total = (size_t)offsets[nb];
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  /* the four lists and the flow completion record (-1 = not completed; its length is the burst count): built and filled beside the
   * batch's present ones, which stay in place if anything fails, then committed together.  (A list of no bursts: blocks of one byte.) */
  DevBuf<int64_t> off;
  DevBuf<double> at, flow_time;
  DevBuf<int32_t> nfull, last, flow_tti;
  HIP_TRY(dev_alloc_all(off, nb + 1, at, total, nfull, total, last, total, flow_tti, total, flow_time, total));
  const std::vector<int32_t> none_tti(total, -1);
  const std::vector<double> none_time(total, -1.0);
  HIP_TRY(off.upload(offsets));
  HIP_TRY(at.upload(time));
  HIP_TRY(nfull.upload(n_full));
  HIP_TRY(last.upload(last_bytes));
  HIP_TRY(flow_tti.upload(none_tti.data()));
  HIP_TRY(flow_time.upload(none_time.data()));
  b->d_arr_off = std::move(off); b->d_arr_time = std::move(at); b->d_arr_nfull = std::move(nfull); b->d_arr_last = std::move(last);
  b->d_flow_tti = std::move(flow_tti); b->d_flow_time = std::move(flow_time);
  return RS_OK;
}

int rs_batch_flow_record(rs_batch* b, int32_t* done_tti, double* done_time) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (!b->queues || !b->d_flow_tti) return fail(RS_ERR_STATE, "no flow completion record: the batch has no arrivals (rs_batch_set_bearers / rs_batch_set_arrivals)");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (done_tti) HIP_TRY(b->d_flow_tti.download(done_tti));
  if (done_time) HIP_TRY(b->d_flow_time.download(done_time));
  return RS_OK;
}

int rs_batch_read_bearer_state(rs_batch* b, double* avg, int64_t* cum_bytes, int64_t* cum_rbs, int32_t* queue_bytes,
                               int32_t* queue_packets) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (!b->queues) return fail(RS_ERR_STATE, "the batch has no bearers (rs_batch_set_bearers)");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  const size_t U = b->U, n = b->d_bavg.count();
  /* device layout [cells][2][U] -> [cells][U][2] */
  auto gather = [&](auto* dst, const auto* src_dev, auto zero) -> int {
    std::vector<decltype(zero)> tmp(n);
    HIP_TRY(hipMemcpy(tmp.data(), src_dev, sizeof(zero) * n, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < (size_t)b->n_cells; c++)
      for (size_t k = 0; k < 2; k++)
        for (size_t u = 0; u < U; u++) dst[(c * U + u) * 2 + k] = tmp[(c * 2 + k) * U + u];
    return RS_OK;
  };
  int rc = RS_OK;
  if (avg && !rc) rc = gather(avg, b->d_bavg.get(), 0.0);
  if (cum_bytes && !rc) rc = gather(cum_bytes, plane(b, b->d_bcum, 0), (int64_t)0);
  if (cum_rbs && !rc) rc = gather(cum_rbs, plane(b, b->d_bcum, 1), (int64_t)0);
  if (queue_bytes && !rc) rc = gather(queue_bytes, plane(b, b->d_qi, 4), (int32_t)0);
  if (queue_packets && !rc) rc = gather(queue_packets, plane(b, b->d_qi, 5), (int32_t)0);
  return rc;
}

/* InternetFlow's arrival process (ref: src/flows/application/InternetFlow.cpp:41-58, 83-90, 155-200): exponential
 * inter-arrival times from libstdc++'s std::exponential_distribution over a default-constructed std::default_random_engine
 * (every InternetFlow object owns one, so every flow of a rate sees the same intervals), rounded up to whole
 * milliseconds; heavy-tailed flow sizes from the table's CDF with one rand() per flow.  The reference draws the sizes from the
 * process-wide libc stream it shares with the scheduler; a batch has no such global event order, so each bearer gets its
 * own libc-compatible stream seeded with size_seed (documented deviation of the batched traffic model). */
int rs_internet_flow_arrivals(double rate_mbps, double start_time, double stop_time, uint32_t size_seed, int32_t max_bursts,
                              double* time, int32_t* n_full, int32_t* last_bytes) {
  if (!(rate_mbps > 0) || !(stop_time > start_time) || max_bursts < 1 || !time || !n_full || !last_bytes)
    return fail(RS_ERR_INVALID, "bad argument");
  static const int kFlowSize[11] = {1460, 2920, 4380, 7300, 10220, 58400, 105120, 200020, 389820, 1733020, 3076220};
  static const double kFlowCdf[11] = {0.5, 0.6, 0.7, 0.75, 0.8, 0.8125, 0.825, 0.85, 0.9, 0.95, 1};
  double avg_flowsize = 0;
  for (int i = 0; i < 11; i++) avg_flowsize += (i == 0 ? kFlowCdf[0] : kFlowCdf[i] - kFlowCdf[i - 1]) * kFlowSize[i];
  const int avg_size = (int)avg_flowsize;
  const double interval_mean = avg_size / rate_mbps * 8 / 1000000;
  const double lambda = 1 / interval_mean;
  std::exponential_distribution<double> distribute(lambda);
  std::default_random_engine generator;
  HostRng sizes;
  sizes.seed(size_seed);
  double now = start_time; /* DoStart schedules the first Send at +0.0 from the application's start */
  int n = 0;
  for (;;) {
    /* Send(): one flow */
    const double cdf = (double)sizes.next() / 2147483647; /* rand() / RAND_MAX */
    int flow_size = kFlowSize[10];
    for (int i = 0; i < 11; i++)
      if (kFlowCdf[i] >= cdf) { flow_size = kFlowSize[i]; break; }
    const int last_pkt = flow_size % 1490;
    const int n_pkts = (int)std::ceil(flow_size / (double)1490);
    if (n >= max_bursts) return fail(RS_ERR_INVALID, "more than max_bursts = %d flows before stop_time", max_bursts);
    time[n] = now;
    /* every packet gets its headers, then the last one is SET to the remainder (no headers on top): :133-136 */
    n_full[n] = last_pkt != 0 ? n_pkts - 1 : n_pkts;
    last_bytes[n] = last_pkt;
    n++;
    /* ScheduleTransmit(GetInterval()) */
    const double interval = std::ceil(distribute(generator) * 1000) / 1000.0;
    if (!((now + interval) < stop_time)) break;
    now = interval + now; /* Simulator::DoSchedule: timeStamp = time + Now() */
  }
  return n;
}

int rs_batch_read_clock(rs_batch* b, double* t, double* last_update) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::vector<RsCellScalars> sc;
  if (const int rc = read_scalars(b, &sc)) return rc;
  for (int c = 0; c < b->n_cells; c++) {
    if (t) t[c] = sc[c].t;
    if (last_update) last_update[c] = sc[c].last_update;
  }
  return RS_OK;
}

int rs_batch_debug_heap_sorts(rs_batch* b, int64_t* out) {
  if (!b || !out) return fail(RS_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::vector<RsCellScalars> sc;
  if (const int rc = read_scalars(b, &sc)) return rc;
  for (int c = 0; c < b->n_cells; c++)
    for (int k = 0; k < 3; k++) out[c * 3 + k] = sc[c].heap_sorts[k];
  return RS_OK;
}

/* ---- checkpoint / resume (ABI 10): everything a batch carries from one launch to the next, as one host block ----
 * header: magic "RSCK2", the shape it belongs to (S, U, R, G, sched, cells, queue model, threads are NOT part of it: any workgroup
 * size continues a run), the number of scheduled TTIs so far, the kernel family that wrote the pending-grant words; then the device
 * arrays verbatim.  The CQI source (epoch grids / trace tables / arrival bursts) is configuration, not state: the caller sets it
 * again on the batch that resumes. */
namespace {
struct CkptHeader {
  char magic[8];
  int32_t S, U, R, G, sched, n_cells, queues, packed_tx; /* packed_tx: the pending-grant words were left by a shape-specialised kernel */
  int64_t ttis_done;
  uint64_t bytes; /* of the whole block */
  /* round 6: FNV-1a over everything else that decides how the run continues -- the users' slices, the slices' weights and
   * algorithm parameters, cqi_refresh, first_tti, phy_error_draws, synthetic_exp -- and over the layout of the block itself (ABI
   * version, sizeof(RsCellScalars)): a checkpoint of a batch whose results would differ is refused, not continued silently */
  uint64_t config_hash;
};
uint64_t ckpt_config_hash(const rs_batch* b) {
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&h](const void* q, size_t n) {
    const unsigned char* c = (const unsigned char*)q;
    for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; }
    h ^= 0xffu; h *= 1099511628211ull; /* field boundary */
  };
  const int32_t scalars[6] = {RS_ABI_VERSION, (int32_t)sizeof(RsCellScalars), b->cfg.cqi_refresh, b->cfg.first_tti, b->cfg.phy_error_draws ? 1 : 0,
                              b->synthetic ? 1 : 0};
  mix(scalars, sizeof scalars);
  mix(b->u2s.data(), 4 * b->u2s.size());
  mix(b->weight.data(), 8 * b->weight.size());
  mix(b->alpha.data(), 4 * b->alpha.size());
  mix(b->beta.data(), 4 * b->beta.size());
  mix(b->eps.data(), 4 * b->eps.size());
  mix(b->psi.data(), 4 * b->psi.size());
  if (b->cell_cfg) { /* the cells' own rows: a checkpoint continues only in a batch that was given the same ones */
    mix(b->cc_u2s.data(), 4 * b->cc_u2s.size());
    mix(b->cc_weight.data(), 8 * b->cc_weight.size());
    mix(b->cc_eps.data(), 4 * b->cc_eps.size());
    mix(b->cc_psi.data(), 4 * b->cc_psi.size());
    if (b->ragged_slices) mix(b->cc_slices.data(), 4 * b->cc_slices.size()); /* (named only where a cell has fewer slices: other batches' hashes stay) */
  }
  return h;
}
}  // namespace

int64_t rs_batch_checkpoint_bytes(rs_batch* b) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (b->direct) return fail(RS_ERR_INVALID, "drop-in contexts carry slice_rbs_offset_ only: rs_get_slice_offset / rs_set_slice_offset");
  size_t n = sizeof(CkptHeader);
  for (const StatePart& q : state_parts(b)) n += q.n;
  return (int64_t)n;
}

int rs_batch_checkpoint_save(rs_batch* b, void* buf, size_t buflen) {
  const int64_t need = rs_batch_checkpoint_bytes(b);
  if (need < 0) return (int)need;
  if (!buf || buflen < (size_t)need) return fail(RS_ERR_INVALID, "checkpoint buffer of %zu bytes, %lld needed", buflen, (long long)need);
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  CkptHeader h{};
  memcpy(h.magic, "RSCK2\0\0", 8);
  h.S = b->S; h.U = b->U; h.R = b->R; h.G = b->G; h.sched = b->sched; h.n_cells = b->n_cells; h.queues = b->queues ? 1 : 0;
  h.packed_tx = (b->general() && !b->queues) ? 1 : 0;
  h.ttis_done = b->ttis_done;
  h.bytes = (uint64_t)need;
  h.config_hash = ckpt_config_hash(b);
  memcpy(buf, &h, sizeof h);
  char* out = (char*)buf + sizeof h;
  for (const StatePart& q : state_parts(b)) {
    HIP_TRY(hipMemcpy(out, q.p, q.n, hipMemcpyDeviceToHost));
    out += q.n;
  }
  return RS_OK;
}

int rs_batch_checkpoint_load(rs_batch* b, const void* buf, size_t buflen) {
  const int64_t need = rs_batch_checkpoint_bytes(b);
  if (need < 0) return (int)need;
  if (!buf || buflen < sizeof(CkptHeader)) return fail(RS_ERR_INVALID, "no checkpoint");
  CkptHeader h;
  memcpy(&h, buf, sizeof h);
  if (memcmp(h.magic, "RSCK2\0\0", 8) != 0) return fail(RS_ERR_INVALID, "not a checkpoint of this library version (magic)");
  if (h.S != b->S || h.U != b->U || h.R != b->R || h.G != b->G || h.sched != b->sched || h.n_cells != b->n_cells || h.queues != (b->queues ? 1 : 0))
    return fail(RS_ERR_INVALID, "checkpoint of another batch: %d slices x %d UEs x %d RBGs x %d PRBs, sched %d, %d cells, queue model %d", h.S, h.U, h.R,
                h.G, h.sched, h.n_cells, h.queues);
  if (h.bytes != (uint64_t)need || buflen < (size_t)need) return fail(RS_ERR_INVALID, "checkpoint of %llu bytes, this batch's are %lld", (unsigned long long)h.bytes, (long long)need);
  if (h.config_hash != ckpt_config_hash(b))
    return fail(RS_ERR_INVALID, "checkpoint of a batch configured differently (users per slice, slice weights / algorithm parameters, per-cell rows, cqi_refresh, first_tti, "
                                "phy_error_draws, synthetic_exp or the library's state layout): the run would not continue as it began");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  const char* in = (const char*)buf + sizeof h;
  for (const StatePart& q : state_parts(b)) {
    if (q.p == (void*)b->d_tx && !b->queues) {
      /* the pending-grant words follow the kernel family that will consume them: a shape-specialised kernel wants bytes | PRBs << 20 with
       * "counted" set (the grant is in the cumulative totals already, whoever wrote it), the built-in kernels want plain bytes */
      std::vector<int32_t> tx(q.n / 4);
      memcpy(tx.data(), in, q.n);
      const bool want_packed = b->general() != nullptr;
      for (int32_t& w : tx) {
        if (want_packed && !h.packed_tx) w = w ? (w | RS_TX_COUNTED) : 0; /* (no PRB count: it is in the totals, nothing reads it again) */
        else if (!want_packed && h.packed_tx) w &= RS_TX_BYTES_MASK;
      }
      HIP_TRY(hipMemcpy(q.p, tx.data(), q.n, hipMemcpyHostToDevice));
    } else {
      HIP_TRY(hipMemcpy(q.p, in, q.n, hipMemcpyHostToDevice));
    }
    in += q.n;
  }
  b->ttis_done = h.ttis_done;
  return RS_OK;
}

int rs_batch_debug_clocks(rs_batch* b, double* shader_mhz, double* kernel_ms) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::vector<RsCellScalars> sc;
  if (const int rc = read_scalars(b, &sc)) return rc;
  for (int c = 0; c < b->n_cells; c++) {
    const double real = (double)(sc[c].real_end - sc[c].real_begin), clk = (double)(sc[c].clk_end - sc[c].clk_begin);
    if (shader_mhz) shader_mhz[c] = real > 0 ? clk / real * 100.0 : 0.0; /* s_memrealtime ticks at 100 MHz */
    if (kernel_ms) kernel_ms[c] = real / 1e5;
  }
  return RS_OK;
}

int rs_batch_autotune_report(rs_batch* b, char* msg, size_t msglen) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (msg && msglen) snprintf(msg, msglen, "%s", b->autotune_msg);
  return b->autotune_n;
}

int rs_batch_prepare_launch(rs_batch* b, int32_t n_ttis) {
  if (!b || n_ttis < 1) return fail(RS_ERR_INVALID, "bad argument");
  if (b->cqi.mode == RS_CQI_NONE) return fail(RS_ERR_STATE, "no CQI source set");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  (void)lean_kernel(b, n_ttis > RS_MAX_TTIS_PER_LAUNCH ? RS_MAX_TTIS_PER_LAUNCH : n_ttis, false);
  if (!b->builds.checked) {
    const int rc = selfcheck(b, n_ttis > RS_MAX_TTIS_PER_LAUNCH ? RS_MAX_TTIS_PER_LAUNCH : n_ttis, false);
    if (rc) return rc;
  }
  if (b->cfg.autotune && !b->builds.autotuned) {
    const int rc = autotune(b, n_ttis > RS_MAX_TTIS_PER_LAUNCH ? RS_MAX_TTIS_PER_LAUNCH : n_ttis);
    if (rc) return rc;
  }
  return RS_OK;
}

int rs_batch_jit_status(rs_batch* b, char* msg, size_t msglen) {
  if (!b) return fail(RS_ERR_INVALID, "null batch");
  if (msg && msglen) snprintf(msg, msglen, "%s", b->jit_msg);
  if (b->builds.rejected || b->builds.rec_rejected) return -2; /* (rec_rejected: the records launches alone lost their run-time build) */
  if (msg && msglen && b->general() && !b->jit_msg[0] && b->selfcheck_msg[0]) snprintf(msg, msglen, "%s", b->selfcheck_msg);
  return b->general() ? 1 : (b->jit_wanted ? -1 : 0);
}

int rs_batch_slice_bytes_device(rs_batch* b, uint64_t* d_out) {
  if (!b || !d_out) return fail(RS_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  /* (each cell's own map once rs_batch_set_cell_configs gave it one) */
  HIP_TRY(rs_launch_slice_bytes(b->d_cumb, b->cell_cfg ? b->d_cc_user_slice : b->d_user_slice, b->cell_cfg ? b->U : 0, b->n_cells, b->U, b->S,
                                (unsigned long long*)d_out, b->stream));
  return RS_OK;
}

int rs_batch_slice_bytes(rs_batch* b, uint64_t* h_out) {
  if (!b || !h_out) return fail(RS_ERR_INVALID, "null argument");
  int rc = rs_batch_slice_bytes_device(b, b->d_slice_bytes);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(h_out, b->d_slice_bytes, 8 * b->S, hipMemcpyDeviceToHost));
  return RS_OK;
}

int rs_batch_debug_stamps(rs_batch* b, int32_t cell, uint64_t* out20) {
  if (!b || !out20 || cell < 0 || cell >= b->n_cells) return fail(RS_ERR_INVALID, "bad argument");
  if (!b->d_stamps) return fail(RS_ERR_STATE, "not a diagnostic (-DRS_STAMPS) build");
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out20, b->d_stamps + (size_t)cell * 20, 8 * 20, hipMemcpyDeviceToHost));
  return RS_OK;
}

int64_t rs_batch_ttis_done(rs_batch* b) { return b ? b->ttis_done : -1; }
void* rs_batch_stream(rs_batch* b) { return b ? (void*)b->stream : nullptr; }
const char* rs_batch_kernel_name(rs_batch* b) {
  if (!b) return "";
  /* after a launch with grant records: the build that served it (its records variant; the built-in kernels once the variants are gone) */
  const int last = b->builds.last;
  if (last == rs_batch::kRecGeneral || last == rs_batch::kRecLean) {
    const bool streamed = b->cfg.cqi_refresh <= 4;
    return last == rs_batch::kRecLean ? (streamed ? "rs_cell_kernel_jit[lean,streamed,records]" : "rs_cell_kernel_jit[lean,records]")
                                : (streamed ? "rs_cell_kernel_jit[streamed,records]" : "rs_cell_kernel_jit[records]");
  }
  if (b->general() && last != rs_batch::kBuiltinRecords) return "rs_cell_kernel_jit";
  switch (b->sched) {
    case 1: return "rs_cell_kernel<1, 0, false>";
    case 7: return "rs_cell_kernel<7, 0, false>";
    case 8: return "rs_cell_kernel<8, 0, false>";
    case RS_SCHED_SUBOPT: return "rs_cell_kernel<101, 0, false>";
    case RS_SCHED_VOGEL: return "rs_cell_kernel<103, 0, false>";
    case RS_SCHED_NVS_NONGREEDY: return "rs_cell_kernel<11, 0, false>";
    case RS_SCHED_UPPERBOUND: {
      const int ept = (b->R * b->S + b->threads - 1) / b->threads;
      return ept <= 1 ? "rs_cell_kernel<10, 1, false>" : ept <= 2 ? "rs_cell_kernel<10, 2, false>" : ept <= 3 ? "rs_cell_kernel<10, 3, false>" : "rs_cell_kernel<10, 4, false>";
    }
    default: {
      const int ept = (b->R * b->S + b->threads - 1) / b->threads;
      return ept <= 1 ? "rs_cell_kernel<9, 1, false>" : ept <= 2 ? "rs_cell_kernel<9, 2, false>" : ept <= 3 ? "rs_cell_kernel<9, 3, false>" : ept <= 4 ? "rs_cell_kernel<9, 4, false>" : "rs_cell_kernel<9, 0, false>";
    }
  }
}

}  // extern "C"

/* ===================================================================================== */
/* drop-in mode: one RBsAllocation() per call on a one-cell batch                        */

namespace {
/* rs_tti_in.cqi_epoch: what one cell's device-resident CQI image holds -- the reports of the cell's last call that stored them (mode 1:
 * the number, the user count, the kind of report, the user list), and whether a later call may still be served from them.  One per
 * context, one per cell of a group.  The record says what the image holds; WHEN it stops being valid is its owner's rule (a context:
 * ctx_pack, ctx_commit_image; a group: ImageGuard, group_commit_images). */
struct CqiImage {
  bool valid = false, prb = false, has_ids = false;
  uint64_t epoch = 0;
  int n = 0;
  std::vector<int32_t> ids;
  /* A call's RsLaunch / RsGroupCell image_mode under the number that counts for it (`epoch`; 0: the call makes no promise) -- 0: the
   * caller's block is read and nothing is kept; 1: it is read and stored as the image; 2: the same reports for the same users as the
   * stored call's -- the block is neither checked, copied nor read, the kernel reads the image (and the device copy of a per-PRB block) */
  int mode(const rs_tti_in& in, bool per_prb, uint64_t epoch_that_counts) const {
    if (epoch_that_counts == 0) return 0;
    const bool same = valid && epoch == epoch_that_counts && n == in.n_users && prb == per_prb && has_ids == (in.user_id != nullptr) &&
                      (!in.user_id || memcmp(ids.data(), in.user_id, 4 * (size_t)n) == 0);
    return same ? 2 : 1;
  }
  /* a mode-1 call has completed: the device holds its reports now */
  void stored(const rs_tti_in& in, bool per_prb) {
    valid = true;
    epoch = in.cqi_epoch;
    n = in.n_users;
    prb = per_prb;
    has_ids = in.user_id != nullptr;
    if (in.user_id) ids.assign(in.user_id, in.user_id + in.n_users);
  }
};

/* A pair of run-time builds of one kernel -- index 0: the general build, 1: the lean build for the plain call -- and their check
 * against the built-in kernel: calls still to be checked, calls that agreed so far (jit_pair_build .. jit_pair_drop below).  A
 * specialised context has one, a group one per form. */
struct JitPair {
  RsJitKernel* jit[2] = {nullptr, nullptr};
  bool wanted = false, dropped = false;
  int chk_left[2] = {0, 0}, chk_agreed[2] = {0, 0};
  char msg[512] = ""; /* why no build serves: the failed build's, the failed check's */
};
}  // namespace

struct rs_ctx {
  rs_batch* b = nullptr;
  /* one pinned staging block each way, mirrored by one device block each way:
   *   in : [ CQI grid, stride bytes | user slice ids, round16(U) | avg_rate f64[U] ]
   *   out: [ tbs i32[U] | uinfo i32[U] | map i16[R] | quota i16[S] | target i16[S] ] */
  uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
  size_t in_bytes = 0, out_bytes = 0;
  /* zero-copy: the kernel reads the pinned input block and writes the pinned output block itself (a few KB over the host
   * link inside one launch) instead of two hipMemcpyAsync around it; RS_DROPIN_COPY=1 restores the copies */
  uint8_t *z_in = nullptr, *z_out = nullptr; /* device-side addresses of h_in / h_out; null: copy path */
  /* RS_DROPIN_TIMING=1: host-side breakdown of the calls (prepare / enqueue / wait / unpack), printed by rs_destroy.
   * (Polling hipStreamQuery instead of hipStreamSynchronize was measured: no faster, the runtime already waits actively.) */
  bool timing = false;
  double t_prep = 0, t_enq = 0, t_wait = 0, t_unpack = 0;
  long n_calls = 0;
  /* Completion by a word in the pinned output block (round 5): the kernel's last store writes the call's sequence number there and
   * the host spins on it -- the stream's completion signal (interrupt or the runtime's own polling, then its bookkeeping) costs a
   * few microseconds more per call (profiles/r05_dropin_split.md).  Zero-copy calls only; RS_DROPIN_POLL=0 keeps
   * hipStreamSynchronize; a call that does not see its number within RS_DROPIN_POLL_US (default 2 000) microseconds falls back to
   * it (and reports whatever error the stream holds). */
  bool poll = false;
  uint32_t seq = 0;
  size_t flag_off = 0; /* offset of the word in h_out / z_out: behind the largest layout, on its own cache line */
  long poll_us = 2000;
  long n_polled = 0, n_fallback = 0;
  /* rs_tti_in.cqi_epoch (round 6): the grid of the last call whose reports were new, kept on the device as the LDS image ([R][Upad]);
   * a call with the same epoch number and the same user list reads it instead of the caller's block (RsLaunch::image_mode) */
  uint8_t* d_img = nullptr;
  CqiImage img;
  long n_img_reused = 0;
  /* rs_ctx_specialize: the context's own builds of the one-TTI kernel (the batch's jit fields stay empty: a context's batch is never
   * launched as a batch), and the blocks of their checked calls -- the built-in kernel's output block; slice state + scalars before
   * / after it (TwinState) */
  JitPair pair;
  uint8_t *d_out2 = nullptr, *d_chk = nullptr;
  std::vector<uint8_t> h_out2;
};

namespace {
/* drop-in contexts alive in this process: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the
 * environment says otherwise), and one-TTI kernels of contexts that share a hardware queue run one after the other
 * (profiles/r06_dropin_concurrency.md: nine threads, four queues, at most four kernels in flight) */
std::atomic<int> g_live_ctx{0};
struct CtxLayout {
  size_t grid, slice, avg, hol, prio, gate, draws, prb, in_total, tbs, uinfo, map, quota, target, upper, out_total;
};
/* first CQI outside 1..15, or null: a branch-free pass (vectorised by the compiler: 12.5 KB per call at 500 UEs x 25 RBGs),
 * the offender is only looked for when there is one */
const uint8_t* first_bad_cqi(const uint8_t* q, size_t n) {
  unsigned bad = 0;
  for (size_t i = 0; i < n; i++) bad |= (unsigned)((uint8_t)(q[i] - 1) > 14);
  if (!bad) return nullptr;
  for (size_t i = 0; i < n; i++)
    if (q[i] < 1 || q[i] > 15) return q + i;
  return nullptr;
}
CtxLayout ctx_layout(int n, int R, int S, int G, bool with_draws) {
  CtxLayout l;
  l.grid = 0;
  l.slice = round_up(n * R, 16);
  l.avg = l.slice + round_up(n, 16);
  l.hol = l.avg + 8 * (size_t)n;
  l.prio = l.hol + 8 * (size_t)n;
  l.gate = l.prio + round_up(n, 16);
  l.draws = l.gate + round_up(4 * n, 16);
  l.prb = l.draws + (with_draws ? round_up(RS_NVS_SAMPLES * n, 16) : 0);
  l.in_total = l.prb + round_up(n * R * G, 16);
  l.tbs = 0;
  l.uinfo = 4 * (size_t)n;
  l.map = 8 * (size_t)n;
  l.quota = l.map + round_up(2 * R, 8);
  l.target = l.quota + round_up(2 * S, 8);
  l.upper = l.target + round_up(2 * S, 8);
  l.out_total = l.upper + 4 * (size_t)S * R; /* sched 10 only uses it */
  return l;
}

/* What packing one rs_tti_in leaves for the launch (pack_tti). */
struct TtiPack {
  CtxLayout l;              /* the block layout for the call's n users */
  size_t in_bytes = 0;      /* bytes of the input block that travel (the per-PRB block only when given) */
  bool exact_scan = false;  /* an input lies outside the FP32 filter's safe range (or general exponents): FP64 scan of every user */
  const int32_t* gate = nullptr; /* the scheduler's gate array of this call, or null */
  bool grid_touched = false;     /* the block's grid area was written (a context's device-resident CQI image no longer mirrors it) */
};

/* One cell's rs_tti_in validated and packed into a staging input block `h_in` (the layout of ctx_layout for its n users): slice
 * bytes, the CQI grid with its zero padding (reuse_grid: left alone -- rs_tti_in.cqi_epoch), averages or the general exponents'
 * denominators, the exact-scan test, draws, gate, HoL delays and priority flags.  Shared by rs_schedule_tti (its one block) and
 * rs_group_schedule_tti (one slot per cell): the two paths cannot drift apart.  Touches nothing but `h_in` and `pk`. */
int pack_tti(const rs_batch* b, const rs_tti_in* in, const rs_tti_out* out, uint8_t* h_in, bool reuse_grid, TtiPack* pk, bool resident_avg = false,
             bool flows = false) {
  const int n = in->n_users, R = b->R, S = b->S;
  if (n < 1 || n > b->U) return fail(RS_ERR_INVALID, "n_users %d outside 1..%d", n, b->U);
  /* resident_avg (rs_group_schedule_tti_at): the cell's averages are on the device -- none are given, and the place of the averages in
   * the block carries the call's user ids instead when it names them (4 of the 8 bytes per user) */
  if (resident_avg && in->avg_rate) return fail(RS_ERR_INVALID, "avg_rate must be NULL: the cell's averages are resident on the device");
  if ((!in->cqi && !in->cqi_prb) || (!in->avg_rate && !resident_avg)) return fail(RS_ERR_INVALID, "null cqi/avg_rate");
  if (out && (!out->rbg_to_user || !out->user_tbs_bits)) return fail(RS_ERR_INVALID, "null output array"); /* (out == null: a run without outputs) */
  const CtxLayout l = ctx_layout(n, R, S, b->G, b->sched == RS_SCHED_NVS_NONGREEDY);
  pk->l = l;
  uint8_t* h_slice = h_in + l.slice;
  for (int i = 0; i < n; i++) {
    int id = in->user_id ? in->user_id[i] : i;
    if (id < 0 || id >= b->U) return fail(RS_ERR_INVALID, "user id %d out of range", id);
    /* (flows, rs_group_schedule_tti_flows: a user's two bearers are two adjacent positions -- the caller has checked the pairs) */
    if (i && in->user_id && (flows ? in->user_id[i] < in->user_id[i - 1] : in->user_id[i] <= in->user_id[i - 1])) return fail(RS_ERR_INVALID, "user_id must ascend");
    h_slice[i] = (uint8_t)b->u2s[id];
    if ((b->sched == RS_SCHED_NVS || b->sched == RS_SCHED_NVS_NONGREEDY) && h_slice[i] != h_slice[0])
      return fail(RS_ERR_INVALID, "RS_SCHED_NVS*: pass only the users of the served slice");
  }
  const int G = b->G;
  pk->in_bytes = l.prb; /* the per-PRB block travels only when given */
  if (in->cqi_prb) {
    const size_t np = (size_t)n * R * G;
    if (!reuse_grid) {
      if (const uint8_t* bad = first_bad_cqi(in->cqi_prb, np)) return fail(RS_ERR_INVALID, "CQI %d outside 1..15", *bad);
      memcpy(h_in + l.prb, in->cqi_prb, np);
      for (int i = 0; i < n; i++)
        for (int r = 0; r < R; r++) h_in[l.grid + (size_t)i * R + r] = in->cqi_prb[((size_t)i * R + r) * G];
    }
    pk->in_bytes = l.prb + np;
  } else if (!reuse_grid) {
    if (const uint8_t* bad = first_bad_cqi(in->cqi, (size_t)n * R)) return fail(RS_ERR_INVALID, "CQI %d outside 1..15", *bad);
    memcpy(h_in + l.grid, in->cqi, (size_t)n * R);
  }
  if (!reuse_grid) memset(h_in + l.grid + (size_t)n * R, 0, l.slice - (size_t)n * R);
  pk->grid_touched = true;
  if (resident_avg) {
    if (in->user_id) memcpy(h_in + l.avg, in->user_id, 4 * (size_t)n);
  } else {
    memcpy(h_in + l.avg, in->avg_rate, 8 * (size_t)n);
  }
  if (b->gen_exp && !resident_avg) { /* (a resident call of such a config is refused before it gets here) */
    /* general exponents: pow(averageRate / 1000.0, psi) with averageRate = 1 + the caller's sum (ref: :681-693), host libm */
    double* den = (double*)(h_in + l.avg);
    for (int i = 0; i < n; i++) {
      double k = 1;
      k += in->avg_rate[i];
      k /= 1000.0;
      den[i] = pow(k, b->psi[h_slice[i]]);
    }
  }
  /* The metric scan ranks users with an FP32 product first; its error bound needs every factor to be an
   * ordinary FP32 number.  The reference takes any double (downlink-transport-scheduler.cpp:677-713: a non-finite, huge, tiny
   * or negative average simply flows through the division and the strict '>' scan), so inputs outside the safe range switch
   * this call to the exact FP64 scan of every user instead of being rejected.  (The EWMA keeps real averages in [1, ~1e12].) */
  bool exact_scan = b->gen_exp; /* (powers of any size: no FP32 ranking, every user is compared with the reference's expression) */
  if (!exact_scan) {
    auto ordinary = [](double x, double lo, double hi) { return x >= lo && x <= hi; }; /* false for NaN */
    /* (resident averages are inside the range by construction: kResidentAvgMax / kResidentMinDt below) */
    for (int i = 0; i < n && !resident_avg; i++) {
      const double a = in->avg_rate[i];
      const double k = b->sched == RS_SCHED_PF ? a : (1 + a) / 1000.0;
      exact_scan |= !ordinary(k, 0x1p-60, 0x1p60);
    }
    if (b->any_alpha && in->hol_delay)
      for (int i = 0; i < n; i++) {
        const double h = in->hol_delay[i];
        exact_scan |= !(h == 0 || ordinary(h, 0x1p-40, 0x1p40));
      }
  }
  pk->exact_scan = exact_scan;
  if (b->sched == RS_SCHED_NVS_NONGREEDY) {
    if (!in->rand_draws) return fail(RS_ERR_INVALID, "RS_SCHED_NVS_NONGREEDY needs rand_draws (%d x n_users values)", RS_NVS_SAMPLES);
    const size_t nd = (size_t)RS_NVS_SAMPLES * n;
    for (size_t i = 0; i < nd; i++) {
      if (in->rand_draws[i] < 0) return fail(RS_ERR_INVALID, "rand_draws[%zu] = %d is not a rand() value", i, in->rand_draws[i]);
      h_in[l.draws + i] = (uint8_t)(in->rand_draws[i] % 4); /* downlink-nvs-scheduler.cpp:438 */
    }
  }
  const int32_t* gate = b->sched == RS_SCHED_NVS ? in->required_rbs : (b->sched == RS_SCHED_PF ? in->data_to_transmit : nullptr);
  pk->gate = gate;
  if (gate) {
    for (int i = 0; i < n; i++)
      if (gate[i] < 0) return fail(RS_ERR_INVALID, "%s[%d] = %d is negative", b->sched == RS_SCHED_NVS ? "required_rbs" : "data_to_transmit", i, gate[i]);
    memcpy(h_in + l.gate, gate, 4 * (size_t)n);
  }
  if (b->any_alpha) {
    bool need_hol = false;
    for (int i = 0; i < n; i++) {
      const int sl = h_slice[i];
      need_hol |= b->alpha[sl] && (b->sched == RS_SCHED_NVS || b->sched == RS_SCHED_NVS_NONGREEDY || b->beta[sl]);
    }
    if (need_hol && !in->hol_delay) return fail(RS_ERR_INVALID, "hol_delay is required by a customised (alpha=1, beta=1) slice");
    if (in->hol_delay) memcpy(h_in + l.hol, in->hol_delay, 8 * (size_t)n);
    else memset(h_in + l.hol, 0, 8 * (size_t)n);
    if (in->prio_has_data) memcpy(h_in + l.prio, in->prio_has_data, (size_t)n);
    else memset(h_in + l.prio, 1, (size_t)n);
  }
  return RS_OK;
}

/* One cell's output block `h_out` (layout `l`) unpacked into the caller's rs_tti_out: call positions back to user ids, the packed
 * per-user word split.  Shared by rs_schedule_tti and rs_group_schedule_tti. */
void unpack_tti(const rs_batch* b, const rs_tti_in* in, rs_tti_out* out, const uint8_t* h_out, const CtxLayout& l, bool want_upper,
                const uint8_t* flow_bearer = nullptr) {
  const int n = in->n_users, R = b->R, S = b->S;
  const int16_t* h_map = (const int16_t*)(h_out + l.map);
  const int16_t* h_quota = (const int16_t*)(h_out + l.quota);
  const int16_t* h_target = (const int16_t*)(h_out + l.target);
  const int32_t* h_tbs = (const int32_t*)(h_out + l.tbs);
  const int32_t* h_uinfo = (const int32_t*)(h_out + l.uinfo);
  for (int r = 0; r < R; r++) {
    int o = h_map[r];
    out->rbg_to_user[r] = o < 0 ? -1 : (in->user_id ? in->user_id[o] : o);
    if (flow_bearer && o >= 0) out->rbg_to_user[r] = 2 * out->rbg_to_user[r] + flow_bearer[o]; /* (a flows call: the flow id 2 * user + bearer) */
  }
  if (want_upper) {
    const int32_t* h_upper = (const int32_t*)(h_out + l.upper);
    for (int i = 0; i < S * R; i++) {
      const int32_t v = h_upper[i];
      if (out->upper_rbg) out->upper_rbg[i] = v < 0 ? -1 : (v & 63);
      if (out->upper_user) out->upper_user[i] = v < 0 ? -1 : (in->user_id ? in->user_id[v >> 8] : (v >> 8));
    }
  } else {
    if (out->upper_rbg) for (int i = 0; i < S * R; i++) out->upper_rbg[i] = -1;
    if (out->upper_user) for (int i = 0; i < S * R; i++) out->upper_user[i] = -1;
  }
  for (int s = 0; s < S; s++) {
    if (out->target_rbs) out->target_rbs[s] = h_target[s];
    if (out->quota_rbgs) out->quota_rbgs[s] = h_quota[s];
  }
  for (int i = 0; i < n; i++) {
    int32_t ui = h_uinfo[i];
    if (out->user_nprb) out->user_nprb[i] = ui & 0xFFFF;
    if (out->user_final_cqi) out->user_final_cqi[i] = (ui >> 16) & 0xFF;
    if (out->user_mcs) out->user_mcs[i] = (ui >> 24) & 0xFF;
    out->user_tbs_bits[i] = h_tbs[i];
  }
}

/* The self-check of a run-time build, one call's output block (layout `l`, n users): `mine` against the built-in kernel's `ref`, field
 * by field; the first difference is the message (`what` stays empty when there is none).  cell >= 0: a group's slot, named in front;
 * tti >= 0: a run's TTI, named behind the cell.  Shared by rs_schedule_tti and rs_group_schedule_tti. */
void compare_out_block(const uint8_t* mine, const uint8_t* ref, const CtxLayout& l, int R, int S, int n, bool want_upper, int cell, char* what,
                       size_t len, int tti = -1) {
  char pre[40] = "";
  if (cell >= 0 && tti >= 0) snprintf(pre, sizeof pre, "cell %d, TTI %d: ", cell, tti);
  else if (cell >= 0) snprintf(pre, sizeof pre, "cell %d: ", cell);
  auto differ = [&](const char* name, size_t off, int count, auto elem) {
    using T = decltype(elem);
    const T *a = (const T*)(mine + off), *r = (const T*)(ref + off);
    for (int i = 0; i < count && !what[0]; i++)
      if (a[i] != r[i]) snprintf(what, len, "%s%s[%d] = %d, the built-in kernel's %d", pre, name, i, (int)a[i], (int)r[i]);
  };
  differ("rbg_to_user (call position)", l.map, R, int16_t());
  differ("quota_rbgs", l.quota, S, int16_t());
  differ("target_rbs", l.target, S, int16_t());
  differ("user_tbs_bits", l.tbs, n, int32_t());
  differ("user_nprb | final_cqi << 16 | mcs << 24", l.uinfo, n, int32_t());
  if (want_upper) differ("upper lists", l.upper, S * R, int32_t());
}

/* Completion by the pinned word: the kernel's last store publishes the call's sequence number behind its outputs (release, system
 * scope; a group: the last workgroup to finish, behind every workgroup's).  Spins on the word for at most `limit_us`; true when the
 * number was seen -- then the stream's own bookkeeping is settled without waiting: every 64th such call asks it, so that nothing piles
 * up in the runtime. */
bool poll_done_word(const uint8_t* word, uint32_t seq, long limit_us, long* n_polled, hipStream_t st) {
  using clk = std::chrono::steady_clock;
  const clk::time_point give_up = clk::now() + std::chrono::microseconds(limit_us);
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n((const uint32_t*)word, __ATOMIC_ACQUIRE) == seq) break;
    __builtin_ia32_pause();
    if ((spins & 255u) == 255u && clk::now() > give_up) return false;
  }
  if ((++*n_polled & 63) == 0) (void)hipStreamQuery(st);
  return true;
}

/* How many calls a run-time build serves beside the built-in kernel before it is trusted (see rs_ctx_jit_status in the header): none for
 * a build that came from the cache with the mark of an earlier process's check, or that is not there at all */
int selfcheck_calls(RsJitKernel* k) {
  int calls = 8;
  if (const char* e = getenv("RS_DROPIN_SELFCHECK_CALLS")) calls = atoi(e) > 0 ? atoi(e) : 0;
  const char* pol = getenv("RS_JIT_SELFCHECK");
  const bool never = pol && pol[0] == '0', always = pol && pol[0] == '2';
  return (k && !never && (always || !rs_jit_is_verified(k))) ? calls : 0;
}
/* one build's part of a *_jit_status message: how it earned (or is still earning) its trust; ref: what its checked calls agree with */
void selfcheck_state(RsJitKernel* k, int left, int agreed, const char* ref, char* out, size_t n) {
  if (!k) snprintf(out, n, "not built");
  else if (left > 0) snprintf(out, n, "%d checked call(s) agreed with %s, %d to go", agreed, ref, left);
  else if (agreed > 0) snprintf(out, n, "verified (%d checked calls agreed with %s)", agreed, ref);
  else if (rs_jit_is_verified(k)) snprintf(out, n, "carries the self-check mark of an earlier check (cache file)");
  else snprintf(out, n, "unchecked (RS_JIT_SELFCHECK=0)");
}

/* A pair's two builds for the config of `b`: rs_jit_get with `flags` (general) and `flags | 4` (lean; RS_JIT_LEAN=0: none, the general
 * build serves every call), and how many calls each serves beside the built-in kernel.  A failed general build leaves its message in
 * the pair. */
int jit_pair_build(JitPair* p, const rs_batch* b, int flags) {
  RsJitSpec spec = {.S = b->S, .U = b->U, .R = b->R, .G = b->G, .NT = b->threads, .sched = b->sched,
                    .qmode = (b->sched == RS_SCHED_PF || b->sched == RS_SCHED_NVS) ? 1 : 0, /* (the gate scratch of a drop-in carve: carve_lds) */
                    .flags = flags};
  char msg[512] = "";
  p->wanted = true;
  p->jit[0] = rs_jit_get(b->cfg.cell.device, spec, msg, sizeof msg);
  if (!p->jit[0]) {
    snprintf(p->msg, sizeof p->msg, "%s", msg[0] ? msg : "hiprtc build failed");
    return fail(RS_ERR_HIP, "%s", p->msg);
  }
  p->msg[0] = 0;
  const char* const e_on = getenv("RS_JIT_LEAN");
  spec.flags |= 4;
  if (!e_on || atoi(e_on) != 0) p->jit[1] = rs_jit_get(b->cfg.cell.device, spec, msg, sizeof msg);
  for (int w = 0; w < 2; w++) {
    p->chk_agreed[w] = 0;
    p->chk_left[w] = selfcheck_calls(p->jit[w]);
  }
  return RS_OK;
}
/* the message and the code of a *_jit_status function; ref: what the pair's checked calls agree with */
int jit_pair_status(const JitPair& p, const char* ref, char* msg, size_t msglen) {
  if (msg && msglen) {
    if (p.dropped || !p.jit[0]) {
      snprintf(msg, msglen, "%s", p.msg);
    } else {
      char ge[220], le[220];
      selfcheck_state(p.jit[0], p.chk_left[0], p.chk_agreed[0], ref, ge, sizeof ge);
      selfcheck_state(p.jit[1], p.chk_left[1], p.chk_agreed[1], ref, le, sizeof le);
      snprintf(msg, msglen, "general build: %s; lean build: %s", ge, le);
    }
  }
  if (p.dropped) return -2;
  return p.jit[0] ? 1 : (p.wanted ? -1 : 0);
}
/* a checked call of build `which` agreed with the built-in kernel; the last one earns the build its mark */
void jit_pair_agreed(JitPair* p, int which) {
  p->chk_agreed[which]++;
  if (--p->chk_left[which] == 0) rs_jit_mark_verified(p->jit[which]);
}
/* a checked call disagreed: one wrong build of a shape and neither is trusted -- both are rejected (and their cache files unlinked) */
void jit_pair_drop(JitPair* p) {
  for (int w = 0; w < 2; w++) {
    if (p->jit[w]) rs_jit_reject(p->jit[w]);
    p->jit[w] = nullptr;
    p->chk_left[w] = 0;
  }
  p->dropped = true;
}

/* The state of a checked call's twin run.  `d_chk` holds two halves, each the [n_cells][S] slice state and then the [n_cells]
 * RsCellScalars of batch `b` (256-byte aligned): the first half is what the built-in kernel found, the second what it left.  A context
 * is n_cells = 1; a group's form with stores keeps those the same way around these calls (group_copy_stores). */
struct TwinState {
  rs_batch* b;
  uint8_t* d_chk;
  int n_cells;
  std::vector<double> mine, kept; /* fetch(): the slice state the run-time build left, and the kept half's */
  size_t ss_bytes() const { return 8 * (size_t)b->S * n_cells; }
  size_t sc_bytes() const { return sizeof(RsCellScalars) * (size_t)n_cells; }
  size_t sc_off() const { return round_up((int)ss_bytes(), 256); }
  size_t half() const { return sc_off() + round_up((int)sc_bytes(), 256); }
  /* before the built-in kernel runs */
  int save() const {
    HIP_TRY(hipMemcpyAsync(d_chk, b->d_sstate, ss_bytes(), hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(d_chk + sc_off(), b->d_scal, sc_bytes(), hipMemcpyDeviceToDevice, b->stream));
    return RS_OK;
  }
  /* behind it: keep what it left, put back what it found -- the run-time build starts from the same state */
  int keep_and_put_back() const {
    HIP_TRY(hipMemcpyAsync(d_chk + half(), b->d_sstate, ss_bytes(), hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->d_sstate, d_chk, ss_bytes(), hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->d_scal, d_chk + sc_off(), sc_bytes(), hipMemcpyDeviceToDevice, b->stream));
    return RS_OK;
  }
  /* the call has completed: both slice states to the host ... */
  int fetch() {
    mine.resize((size_t)b->S * n_cells);
    kept.resize(mine.size());
    HIP_TRY(hipMemcpy(mine.data(), b->d_sstate, ss_bytes(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(kept.data(), d_chk + half(), ss_bytes(), hipMemcpyDeviceToHost));
    return RS_OK;
  }
  /* ... and cell `row`'s compared bit for bit; the first difference is the message, named as compare_out_block names a cell (`cell`) */
  void compare(int row, int cell, char* what, size_t len) const {
    char pre[24] = "";
    if (cell >= 0) snprintf(pre, sizeof pre, "cell %d: ", cell);
    for (int i = 0; i < b->S && !what[0]; i++) {
      const double a = mine[(size_t)row * b->S + i], r = kept[(size_t)row * b->S + i];
      if (to_bits(a) != to_bits(r)) snprintf(what, len, "%sslice state[%d] = %a, the built-in kernel's %a", pre, i, a, r);
    }
  }
  /* the pair is dropped: the call leaves the built-in kernel's state */
  int restore_kept() const {
    HIP_TRY(hipMemcpy(b->d_sstate, d_chk + half(), ss_bytes(), hipMemcpyDeviceToDevice));
    return RS_OK;
  }
};

/* the drop-in switches of the environment, read when a context or a group is created */
struct DropinEnv {
  bool force_copy, timing, poll; /* RS_DROPIN_COPY=1, RS_DROPIN_TIMING=1, not RS_DROPIN_POLL=0 */
  long poll_us;                  /* RS_DROPIN_POLL_US, default 2 000 */
};
DropinEnv dropin_env() {
  auto is = [](const char* name, char v) { const char* e = getenv(name); return e && e[0] == v; };
  DropinEnv env = {is("RS_DROPIN_COPY", '1'), is("RS_DROPIN_TIMING", '1'), !is("RS_DROPIN_POLL", '0'), 2000};
  if (const char* pu = getenv("RS_DROPIN_POLL_US")) env.poll_us = atol(pu) > 0 ? atol(pu) : 2000;
  return env;
}
}  // namespace

extern "C" {

int rs_ctx_debug_heap_sorts(rs_ctx* ctx, int64_t* out) {
  if (!ctx || !ctx->b) return fail(RS_ERR_INVALID, "null context");
  return rs_batch_debug_heap_sorts(ctx->b, out);
}

rs_ctx* rs_create_checked(const rs_config* cfg, int abi_version, size_t cfg_size) {
  return abi_matches(abi_version, cfg_size, sizeof(rs_config), "rs_config") ? rs_create(cfg) : nullptr;
}

rs_ctx* rs_create(const rs_config* cfg) {
  rs_batch_config bc;
  memset(&bc, 0, sizeof bc);
  if (!cfg) { fail(RS_ERR_INVALID, "null config"); return nullptr; }
  bc.cell = *cfg;
  bc.n_cells = 1;
  bc.cqi_refresh = 1;
  rs_batch* b = batch_new(&bc, true);
  if (!b) return nullptr;
  rs_ctx* c = new (std::nothrow) rs_ctx();
  if (!c) { rs_batch_destroy(b); fail(RS_ERR_INVALID, "out of memory"); return nullptr; }
  c->b = b;
  const CtxLayout l = ctx_layout(b->U, b->R, b->S, b->G, b->sched == RS_SCHED_NVS_NONGREEDY);
  c->in_bytes = l.in_total;
  c->flag_off = round_up(l.out_total, 64);
  c->out_bytes = c->flag_off + 64;
  const size_t img_bytes = round_up(rs_upad_of(b->U) * b->R, 16);
  bool ok = hipMalloc(&c->d_in, c->in_bytes) == hipSuccess && hipMalloc(&c->d_out, c->out_bytes) == hipSuccess &&
            hipMalloc(&c->d_img, img_bytes) == hipSuccess && hipMalloc(&c->d_out2, c->out_bytes) == hipSuccess &&
            hipMalloc(&c->d_chk, 2 * TwinState{b, nullptr, 1}.half()) == hipSuccess &&
            hipHostMalloc((void**)&c->h_in, c->in_bytes, hipHostMallocMapped) == hipSuccess &&
            hipHostMalloc((void**)&c->h_out, c->out_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
  const DropinEnv env = dropin_env();
  if (ok && !env.force_copy) {
    void *zi = nullptr, *zo = nullptr;
    if (hipHostGetDevicePointer(&zi, c->h_in, 0) == hipSuccess && hipHostGetDevicePointer(&zo, c->h_out, 0) == hipSuccess) {
      c->z_in = (uint8_t*)zi;
      c->z_out = (uint8_t*)zo;
    }
  }
  if (!ok) { fail(RS_ERR_HIP, "allocation of the staging blocks failed"); rs_destroy(c); return nullptr; }
  c->timing = env.timing;
  c->poll = c->z_out != nullptr && env.poll;
  c->poll_us = env.poll_us;
  if (c->h_out) memset(c->h_out + c->flag_off, 0, 64);
  c->h_out2.assign(c->out_bytes, 0);
  g_err[0] = 0;
  if (cfg->link_tables == RS_LINK_DEFAULT) {
    /* a drop-in context follows THIS host's libm (the reference beside it does); when that is not the libm of the fixtures, say so once */
    char where[300] = "";
    const int diff = rs_link_tables_compare(where, sizeof where);
    if (diff > 0)
      snprintf(g_err, sizeof g_err, "warning: this host's libm gives %d EESM constant(s) that differ from the pinned glibc-2.35 set (%.300s): the context "
               "follows the host (RS_LINK_HOST_LIBM); RS_LINK_PINNED_GLIBC_2_35 reproduces the fixtures", diff, where);
  }
  {
    const int live = ++g_live_ctx;
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    const int hwq = e && atoi(e) > 0 ? atoi(e) : 4;
    if (live > hwq && !cfg->stream) {
      const size_t at = strlen(g_err);
      snprintf(g_err + at, sizeof g_err - at, "%swarning: %d drop-in contexts in this process share %d hardware queues (GPU_MAX_HW_QUEUES, read by the HIP "
               "runtime at its first call): their one-TTI kernels run %d at a time; export GPU_MAX_HW_QUEUES=%d (or more) before the process starts",
               at ? "; " : "", live, hwq, hwq, live);
    }
  }
  return c;
}

void rs_destroy(rs_ctx* c) {
  if (!c) return;
  if (c->h_out2.size()) --g_live_ctx; /* (counted by rs_create once it got that far) */
  if (c->timing && c->n_calls)
    fprintf(stderr, "rs_schedule_tti x %ld: prepare %.2f us, enqueue %.2f us, wait %.2f us, unpack %.2f us per call (%ld completed by the polled word, %ld fell back to the stream, %ld read the device-resident CQI image)\n", c->n_calls,
            c->t_prep / c->n_calls, c->t_enq / c->n_calls, c->t_wait / c->n_calls, c->t_unpack / c->n_calls, c->n_polled, c->n_fallback, c->n_img_reused);
  if (c->b && c->b->stream) (void)hipStreamSynchronize(c->b->stream);
  if (c->d_in) (void)hipFree(c->d_in);
  if (c->d_out) (void)hipFree(c->d_out);
  if (c->d_img) (void)hipFree(c->d_img);
  if (c->d_out2) (void)hipFree(c->d_out2);
  if (c->d_chk) (void)hipFree(c->d_chk);
  if (c->h_in) (void)hipHostFree(c->h_in);
  if (c->h_out) (void)hipHostFree(c->h_out);
  rs_batch_destroy(c->b);
  delete c;
}

namespace {
/* One context call: what the caller gave, then what the phases of rs_schedule_tti decide along the way.  (The phases are static:
 * inside extern "C" the unnamed namespace alone would not keep their names out of the library's exports.) */
struct CtxCall {
  const rs_tti_in* in;
  rs_tti_out* out;
  /* ctx_pack: RsLaunch::image_mode of the call, what pack_tti left for the launch */
  int image_mode;
  TtiPack pk;
  /* rs_schedule_tti: the kernel reads and writes the pinned blocks in place; the caller wants UpperBound's lists.  ctx_run: completion
   * by the polled word; the run-time build that serves the call (null: the built-in kernel; which: 0 general, 1 lean) and whether the
   * built-in kernel ran beside it */
  bool zc, want_upper, poll, checked;
  RsJitKernel* kd;
  int which;
};

/* The call's image mode -- the same reports for the same users as the call before?  then the caller's block is not touched -- and its
 * input block.  Writes c->h_in.  The image's term ends as soon as the block's grid area was written (also when pack_tti then refuses
 * the call) and begins again when this call has gone through (ctx_commit_image). */
static int ctx_pack(rs_ctx* c, CtxCall& call) {
  call.image_mode = c->img.mode(*call.in, call.in->cqi_prb != nullptr, call.in->cqi_epoch);
  const int rc = pack_tti(c->b, call.in, call.out, c->h_in, call.image_mode == 2, &call.pk);
  if (call.pk.grid_touched) c->img.valid = false;
  return rc;
}

/* a launch block's output pointers: into one output block of layout l */
static void ctx_point_outputs(RsLaunch* L, uint8_t* out, const CtxLayout& l, bool want_upper) {
  L->log_tbs = (int32_t*)(out + l.tbs);
  L->log_uinfo = (int32_t*)(out + l.uinfo);
  L->log_map = (int16_t*)(out + l.map);
  L->log_quota = (int16_t*)(out + l.quota);
  L->log_target = (int16_t*)(out + l.target);
  L->log_upper = want_upper ? (int32_t*)(out + l.upper) : nullptr;
}

/* the call's launch block: the config's, then the call's input and output block.  (Direct mode: the kernel clears its per-user outputs
 * itself and reads the single grid on every call.) */
static void ctx_fill_launch(const rs_ctx* c, const CtxCall& call, RsLaunch* launch) {
  const rs_batch* b = c->b;
  const rs_tti_in* in = call.in;
  const CtxLayout& l = call.pk.l;
  uint8_t* const dev_in = call.zc ? c->z_in : c->d_in;
  RsLaunch& L = *launch;
  L = b->base;
  L.U = in->n_users;
  L.Upad = upad_of(in->n_users);
  L.n_ttis = 1;
  L.direct = 1;
  L.rand0 = in->rand0;
  L.rand1 = in->rand1;
  L.cqi_mode = RS_CQI_EPOCHS;
  L.refresh = 1;
  L.epochs = dev_in + l.grid;
  L.grid_stride = (int64_t)l.slice;
  L.n_epochs = 1;
  L.user_slice = dev_in + l.slice;
  L.avg = (double*)(dev_in + l.avg);
  L.prb_cqi = in->cqi_prb ? dev_in + l.prb : nullptr;
  L.grid_image = c->d_img;
  L.image_mode = call.image_mode;
  L.queue_mode = b->any_alpha ? 1 : 0;
  L.hol = (const double*)(dev_in + l.hol);
  L.prio = dev_in + l.prio;
  L.draws = dev_in + l.draws;
  L.gate = call.pk.gate ? (const int32_t*)(dev_in + l.gate) : nullptr;
  L.exact_scan = call.pk.exact_scan ? 1 : 0;
  L.gen_exp = b->gen_exp ? 1 : 0;
  L.gen_num = b->d_gen_num;
  if (b->sched == RS_SCHED_PF) { L.n_seg = (in->n_users + RS_PF_SEG - 1) / RS_PF_SEG; L.n_items = b->R * L.n_seg; }
  ctx_point_outputs(&L, call.zc ? c->z_out : c->d_out, l, call.want_upper);
}

/* A checked call: the built-in kernel first, on the same inputs and the same slice state, its outputs into a block of its own.  (A call
 * with new reports: BOTH kernels transpose the caller's block and store the image -- the same bytes when the build is right; a wrong
 * image would show in the checked calls that read it.) */
static int ctx_run_twin(rs_ctx* c, const CtxCall& call, const RsLaunch& L) {
  rs_batch* b = c->b;
  const TwinState tw{b, c->d_chk, 1};
  if (const int rc = tw.save()) return rc;
  RsLaunch Lb = L;
  ctx_point_outputs(&Lb, c->d_out2, call.pk.l, call.want_upper);
  Lb.done_flag = nullptr;
  HIP_TRY(rs_launch_cells(&Lb, b->threads, b->stream));
  HIP_TRY(hipMemcpyAsync(c->h_out2.data(), c->d_out2, call.pk.l.out_total, hipMemcpyDeviceToHost, b->stream));
  return tw.keep_and_put_back();
}

/* The copies in, the launch, the copy back.  rs_ctx_specialize: this context's own build of the one-TTI kernel serves the call -- its
 * lean form the plain call (per-RBG CQI, no customised slices, no gates, exponents in {0, 1}, every input inside the FP32 filter's
 * range), the general one every other.  A build that does not carry the self-check mark serves its first calls beside the built-in
 * kernel (rs_ctx_jit_status): same inputs, same slice state; every output field and the slice state left behind must agree. */
static int ctx_run(rs_ctx* c, CtxCall& call, RsLaunch& L) {
  rs_batch* b = c->b;
  hipStream_t st = b->stream;
  const CtxLayout& l = call.pk.l;
  if (!call.zc) {
    /* (an unchanged report set: the grid and the per-PRB block are on the device already; the per-call words lie between them) */
    if (call.image_mode == 2) HIP_TRY(hipMemcpyAsync(c->d_in + l.slice, c->h_in + l.slice, l.prb - l.slice, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemcpyAsync(c->d_in, c->h_in, call.pk.in_bytes, hipMemcpyHostToDevice, st));
  }
  const JitPair& p = c->pair;
  const bool lean = p.jit[1] && !L.prb_cqi && !L.queue_mode && !L.gate && !L.exact_scan && !L.gen_exp && !L.log_upper && !L.synthetic;
  call.which = lean ? 1 : 0;
  call.kd = p.jit[call.which];
  call.checked = call.kd != nullptr && p.chk_left[call.which] > 0;
  if (call.checked)
    if (const int rc = ctx_run_twin(c, call, L)) return rc;
  call.poll = call.zc && c->poll && !call.checked;
  if (call.poll) {
    if (++c->seq == 0) c->seq = 1; /* (0 is the word's initial value) */
    L.done_flag = (uint32_t*)(c->z_out + c->flag_off);
    L.done_seq = c->seq;
  }
  if (call.kd) HIP_TRY(rs_jit_launch(call.kd, &L, st));
  else HIP_TRY(rs_launch_cells(&L, b->threads, st));
  if (!call.zc) HIP_TRY(hipMemcpyAsync(c->h_out, c->d_out, l.out_total, hipMemcpyDeviceToHost, st));
  return RS_OK;
}

/* by the polled word (the kernel's last store), else by the stream */
static int ctx_wait(rs_ctx* c, const CtxCall& call) {
  bool seen = false;
  if (call.poll) {
    seen = poll_done_word(c->h_out + c->flag_off, c->seq, c->poll_us, &c->n_polled, c->b->stream);
    if (!seen) c->n_fallback++; /* (a context counts the polled calls that fell back, not every stream wait) */
  }
  if (!seen) HIP_TRY(hipStreamSynchronize(c->b->stream));
  return RS_OK;
}

/* A checked call's end: every output field and the slice state left behind against the built-in kernel's, field by field -- the first
 * difference is the message.  Then the build is wrong: both are dropped (and their cache files), this call returns the built-in
 * kernel's outputs and leaves its state, all later ones run the built-in kernel. */
static int ctx_check(rs_ctx* c, const CtxCall& call) {
  const rs_batch* b = c->b;
  JitPair& p = c->pair;
  TwinState tw{c->b, c->d_chk, 1};
  if (const int rc = tw.fetch()) return rc;
  char what[200] = "";
  compare_out_block(c->h_out, c->h_out2.data(), call.pk.l, b->R, b->S, call.in->n_users, call.want_upper, -1, what, sizeof what);
  tw.compare(0, -1, what, sizeof what);
  if (!what[0]) {
    jit_pair_agreed(&p, call.which);
    return RS_OK;
  }
  jit_pair_drop(&p);
  memcpy(c->h_out, c->h_out2.data(), call.pk.l.out_total);
  if (const int rc = tw.restore_kept()) return rc;
  snprintf(p.msg, sizeof p.msg, "self-check of the specialised %s build, checked call %d: %s; the build is dropped, the built-in kernel serves this "
           "context (lint the code object: tools/lint_exec_restore.py)", call.which ? "lean" : "general", p.chk_agreed[call.which] + 1, what);
  snprintf(g_err, sizeof g_err, "%s", p.msg);
  return RS_OK;
}

/* the call has gone through under a number: the device holds its reports now */
static void ctx_commit_image(rs_ctx* c, const CtxCall& call) {
  if (call.image_mode == 1) c->img.stored(*call.in, call.in->cqi_prb != nullptr);
  if (call.image_mode == 2) {
    c->img.valid = true;
    c->n_img_reused++;
  }
}
}  // namespace

/* one context call, phase by phase; RS_DROPIN_TIMING splits it into prepare, enqueue, wait and unpack */
int rs_schedule_tti(rs_ctx* c, const rs_tti_in* in, rs_tti_out* out) {
  if (!c || !in || !out) return fail(RS_ERR_INVALID, "null argument");
  rs_batch* b = c->b;
  using clk = std::chrono::steady_clock;
  const clk::time_point t0 = c->timing ? clk::now() : clk::time_point();
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  CtxCall call = {in, out};
  int rc = ctx_pack(c, call);
  if (rc) return rc;
  const clk::time_point t1 = c->timing ? clk::now() : clk::time_point();
  /* per-PRB reports and queue state are read again and again inside the TTI: those calls keep the device copies */
  call.zc = c->z_in != nullptr && !in->cqi_prb && !b->any_alpha;
  call.want_upper = b->sched == RS_SCHED_UPPERBOUND && (out->upper_rbg || out->upper_user);
  RsLaunch L;
  ctx_fill_launch(c, call, &L);
  if ((rc = ctx_run(c, call, L))) return rc;
  const clk::time_point t2 = c->timing ? clk::now() : clk::time_point();
  if ((rc = ctx_wait(c, call))) return rc;
  if (call.checked && (rc = ctx_check(c, call))) return rc;
  ctx_commit_image(c, call);
  const clk::time_point t3 = c->timing ? clk::now() : clk::time_point();
  unpack_tti(b, in, out, c->h_out, call.pk.l, call.want_upper);
  if (c->timing) {
    const clk::time_point t4 = clk::now();
    auto us = [](clk::time_point a, clk::time_point b2) { return std::chrono::duration<double, std::micro>(b2 - a).count(); };
    c->t_prep += us(t0, t1);
    c->t_enq += us(t1, t2);
    c->t_wait += us(t2, t3);
    c->t_unpack += us(t3, t4);
    c->n_calls++;
  }
  return RS_OK;
}

/* Shape specialisation of a drop-in context (round 4): the one-TTI kernel compiled for this context's slices, RBGs, PRBs per RBG,
 * scheduler and user CAPACITY (the LDS carve), the users of a call staying a launch argument, in a general and a lean build (the
 * per-call options of the plain call as constants).  About two seconds per shape and process (cached); results are identical.  On
 * failure the context keeps the kernels built into the library. */
int rs_ctx_specialize(rs_ctx* c) {
  if (!c) return fail(RS_ERR_INVALID, "null context");
  if (c->pair.jit[0]) return RS_OK;
  if (c->pair.dropped) return fail(RS_ERR_STATE, "%s", c->pair.msg);
  HIP_TRY(hipSetDevice(c->b->cfg.cell.device));
  return jit_pair_build(&c->pair, c->b, 1); /* (1: the one-TTI form) */
}

int rs_ctx_jit_status(rs_ctx* c, char* msg, size_t msglen) {
  if (!c) return fail(RS_ERR_INVALID, "null context");
  return jit_pair_status(c->pair, "the built-in kernel field by field", msg, msglen);
}


int rs_get_slice_offset(rs_ctx* c, double* offset) {
  if (!c || !offset) return fail(RS_ERR_INVALID, "null argument");
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  HIP_TRY(hipMemcpy(offset, c->b->d_sstate, 8 * c->b->S, hipMemcpyDeviceToHost));
  return RS_OK;
}

int rs_set_slice_offset(rs_ctx* c, const double* offset) {
  if (!c || !offset) return fail(RS_ERR_INVALID, "null argument");
  if (const int rc = check_slice_state(c->b, offset, 0)) return rc; /* (a refused call leaves the state as it was) */
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  HIP_TRY(hipMemcpy(c->b->d_sstate, offset, 8 * c->b->S, hipMemcpyHostToDevice));
  return RS_OK;
}

/* ---- a group of drop-in cells: one TTI of K cells in one launch (include/radiosaber_hip.h) ---- */

namespace {
/* One cell's residency.  A cell is resident in one form at a time or in none; the form's counters -- the per-user counters of the
 * averages, the bearer counters of the bearers (a flow-resident cell always has its counters: no state of its own) -- exist only
 * on top of their form, so a cell in no form has none.  Beside it the host's mirror of the cell's clock: the time of its last
 * update, and whether no byte can be waiting for the next one (nothing served since the form's setter or an all-zero
 * rs_group_set_pending).  Only the transitions below change the record. */
struct GroupCellState {
  enum Form : uint8_t { kNone, kAverages, kBearers, kFlows };
  bool in(Form f) const { return form_ == f; }
  bool counted(Form f) const { return form_ == f && counted_; } /* f's counters exist */
  bool pending_zero() const { return pending_zero_; }
  double last_update() const { return last_update_; }
  /* a setter of form f starts its copies: the cell is in no form until enter().  Returns whether f's counters and their term
   * go on behind it (the cell was in f, counted: the setter of a form keeps that form's counters and ends the other's) */
  bool leave_for(Form f) {
    const bool keep = counted(f);
    leave();
    return keep;
  }
  void leave() { /* (a failed call too: the stores half written, perhaps) */
    form_ = kNone;
    counted_ = false;
  }
  void enter(Form f, bool counters, double last_update) {
    form_ = f;
    counted_ = counters && (f == kAverages || f == kBearers);
    pending_zero_ = true;
    last_update_ = last_update;
  }
  void end_counters() { counted_ = false; }
  void start_counters() { counted_ = form_ == kAverages || form_ == kBearers; }
  void set_pending_zero(bool zero) { pending_zero_ = zero; }
  /* a served call: dated `last` (a run: its last TTI's clock -- a step of 0 repeats the value before it), and grants may be waiting.
   * (An update-only slot credits nothing: behind an update no byte is waiting, without one nothing changed.) */
  void served(bool credited, double first, double last) {
    if (credited) pending_zero_ = false;
    else if (first != last_update_) pending_zero_ = true;
    last_update_ = last;
  }

 private:
  Form form_ = kNone;
  bool counted_ = false, pending_zero_ = false;
  double last_update_ = 0.0;
};

/* A pinned block of words that travels beside the call slots: the kernel reads or writes it in place through its mapping (z) when
 * the group's main block on that side is mapped, else through a device twin (d) and a copy on the stream. */
struct GroupStaged {
  int32_t *h = nullptr, *z = nullptr, *d = nullptr;
  int32_t* dev() const { return z ? z : d; } /* the pointer the kernel gets */
  bool copied() const { return !z; }         /* a stream copy between h and d is needed */
  bool make(size_t bytes, unsigned flags, bool map) { /* all or none; zeroed */
    bool ok = hipHostMalloc((void**)&h, bytes, flags) == hipSuccess;
    void* m = nullptr;
    if (ok && map && hipHostGetDevicePointer(&m, h, 0) == hipSuccess) z = (int32_t*)m;
    if (ok && !z) ok = hipMalloc(&d, bytes) == hipSuccess;
    if (ok) memset(h, 0, bytes);
    else release();
    return ok;
  }
  void release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    h = z = d = nullptr;
  }
};

/* the device stores of the resident forms: the rows of kGroupStores, the indices of rs_group::store */
enum GroupStoreId { kRavg, kRpend, kRlast, kRgather, kRuid, kQavg, kQpend, kQdata, kQhas, kCbytes, kCrbs, kAcbytes, kAcrbs, kGroupNStores };
}  // namespace

struct rs_group {
  rs_batch* b = nullptr;    /* a direct-mode batch of n_cells cells: the config's device tables, [cells][S] slice state, [cells] scalars, the stream */
  int n_cells = 0;
  /* one mapped pinned block each way, n_cells call slots each, and their device twins for the calls that copy (per-PRB reports,
   * customised slices: read again and again inside the TTI).  Input slot: RsGroupCell header | the single call's input block;
   * output slot: the single call's output block.  The completion word lies behind the last output slot, on its own cache line. */
  uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr, *z_in = nullptr, *z_out = nullptr;
  size_t in_stride = 0, out_stride = 0, flag_off = 0;
  /* runs (rs_group_run_at): the slots' per-TTI tables -- [n_cells][RS_GROUP_MAX_RUN] rows of clock, rand0, rand1 -- lie behind the last
   * input slot, at run_table_off of h_in / d_in; the output blocks hold out_slots slots (n_cells at first, grown to slots x TTIs of the
   * largest run so far: group_grow_out), the completion word behind the last of them */
  size_t run_table_off = 0, out_slots = 0;
  uint32_t* d_count = nullptr; /* the launch's completion counter (rs_group_kernel) */
  bool poll = false;
  uint32_t seq = 0;
  long poll_us = 2000;
  int64_t launches = 0;
  std::vector<uint8_t> named; /* cell_ids check: which cells this call has named so far */
  std::vector<TtiPack> packs;
  /* rs_tti_in.cqi_epoch, per CELL (not per call slot): the grid of the cell's last call under a non-zero number, kept on the device as
   * the LDS image ([R][Upad of that call's n], d_img: [n_cells][img_stride]), its per-PRB block beside it when that call gave one
   * (d_prb: [n_cells][prb_stride], allocated by the first call that needs it), and the record that decides whether a later call may
   * be served from them (CqiImage).  A record changes only after its launch has completed.
   * RS_GROUP_IMAGE=0 (read at create): every cqi_epoch counts as 0. */
  bool image_on = true, prb_store_failed = false;
  uint8_t *d_img = nullptr, *d_prb = nullptr;
  size_t img_stride = 0, prb_stride = 0;
  std::vector<CqiImage> img;
  std::vector<uint8_t> modes;  /* per call slot: RsGroupCell::image_mode of the call being served */
  int64_t n_reused = 0, n_stored = 0, n_plain = 0; /* cell-TTIs of successful calls in mode 2 / 1 / 0 (rs_group_image_stats) */
  /* RS_DROPIN_TIMING=1: the host-side split of the calls, printed by rs_group_destroy */
  bool timing = false;
  double t_prep = 0, t_enq = 0, t_wait = 0, t_unpack = 0;
  long n_calls = 0, n_cell_ttis = 0, n_polled = 0, n_fallback = 0;
  /* Run-time builds of a group call's kernel (rs_group_specialize, rs_group_specialize_resident, rs_group_specialize_queued,
   * rs_group_specialize_flows, rs_group_specialize_counted, rs_group_specialize_run): one pair
   * of builds per form (JitPair), checked against the form's built-in kernel.  The six pairs are independent: each
   * serves its own kind of call, is checked against its own built-in kernel and is dropped alone.  The check of a form with stores
   * (kGroupForms) also compares those: the pair's d_stores_chk holds them before the built-in kernel ran and as that kernel left them
   * (two halves, group_copy_stores). */
  JitPair pair[RS_GROUP_RUN + 1]; /* by GroupForm::pair: every form's but the counted run's, which has no run-time builds */
  uint8_t* d_stores_chk[RS_GROUP_RUN + 1] = {};
  /* every pair's: the built-in kernel's output slots (out_slots of them, as d_out: group_grow_out grows both for a run); the group's
   * slice state + scalars before / after it (TwinState) */
  uint8_t *d_out2 = nullptr, *d_chk = nullptr;
  std::vector<uint8_t> h_out2;
  /* Resident cells.  A cell is resident in one form at a time (GroupCellState: cells[cell] -- the form, whether the form's counters
   * exist on top of it, and the host's mirror of the cell's clock: the clock check needs no read-back).  What the forms keep on the
   * device lies in the stores of kGroupStores, one row per store, [n_cells][elements per cell] each: store[row] is the row's block,
   * null until the first setter of its allocation family makes the whole family (group_alloc_family).
   *   the cell family    rlast, rgather, ruid: a cell's last-update time, the gather rows of calls that name their users and the ids they
   *                      were gathered by -- every form's
   *   averages           ravg, rpend: [U] averages and pending bytes (rs_group_set_avg, rs_group_schedule_tti_at, rs_group_run_at)
   *   bearers            qavg, qpend, qhas, qdata: [U][2] averages, pending bytes and existence bytes of the users' two bearers and a
   *                      call's data words in call order (rs_group_set_bearers, rs_group_schedule_tti_queued); the flows form of
   *                      scheduler 1 keeps its flows in them too (rs_group_set_flows, rs_group_schedule_tti_flows)
   *   bearer counters    cbytes, crbs: [U][2] m_cumulateBytes / m_cumulateRBs beside the bearer stores (rs_group_set_counters,
   *                      rs_group_schedule_tti_counted; a flow-resident cell always has them)
   *   per-user counters  acbytes, acrbs: [U] m_cumulateBytes / m_cumulateRBs beside the averages (rs_group_set_avg_counters,
   *                      rs_group_run_counted_at: the launch block's grp_cbytes / grp_crbs point at them in a counted run) */
  void* store[kGroupNStores] = {};
  std::vector<GroupCellState> cells;
  /* The slots' rows that travel beside the slots, [n_cells][U][2] words each, so that the slots of the other calls keep their size
   * (GroupStaged): qin -- a queued call's data words, a flows call's bearer words (one per position), made with the bearer stores;
   * sent -- a counted call's sent rows, made with the bearer counters; sent2 -- the twin that the built-in kernel writes in a checked
   * call of the counted pair, made by the first such call (the counter stores, and with them sent, may not exist yet when the pair is
   * built).  has_bearer: the host's mirror of the existence bytes, [n_cells][U][2]. */
  GroupStaged qin, sent, sent2;
  std::vector<uint8_t> has_bearer, empty_slot; /* empty_slot: per call slot, n_users == 0 (an update-only slot of a queued call) */
  /* grant records (rs_group_run_records_at): the slots' record blocks -- per slot T lists of `cap` records, then T count words, see
   * RsGroupCell::run_rec_cap -- in device memory (the kernel adds to the count words), and the pinned twin they are copied back to.
   * Both grow to the largest call so far, as the output blocks do. */
  uint8_t *d_recs = nullptr, *h_recs = nullptr;
  size_t recs_bytes = 0;
  double t_recs = 0; /* RS_DROPIN_TIMING: the share of t_unpack spent on sorting and copying records */
  /* rs_group_kernel_name: the last call's form (a row of kGroupForms), whether a run-time build served it, the built-in kernels' names by row */
  int last_call_form = 0;
  bool last_call_jit = false;
  char kname[RS_GROUP_FORMS][56] = {}, kname_jit[RS_GROUP_FORMS][40] = {};
};

namespace {
/* The forms of a group call, one row each: what the HOST alone knows of a form.  What a form is -- the facts its kernels read, the
 * launch-block pointers they dereference, the flags and names of its run-time builds, the schedulers it exists for -- is its row of
 * rs_group_form (rs_device.h, the same row order); a call's row is its form. */
enum { kGroupPlain = RS_GROUP_PLAIN, kGroupResident = RS_GROUP_RESIDENT, kGroupQueued = RS_GROUP_QUEUED, kGroupFlows = RS_GROUP_FLOWS,
       kGroupCounted = RS_GROUP_COUNTED, kGroupRun = RS_GROUP_RUN, kGroupRunCounted = RS_GROUP_RUN_COUNTED };
struct GroupForm {
  bool slots0;     /* update-only slots (n_users == 0) are allowed */
  int pair;        /* rs_group::pair[] that serves the form; -1: the form has no run-time builds, its built-in kernel serves every call */
  int store_width; /* the stores its self-check saves, restores and compares: 0 none, 1 the resident stores [U], 2 the bearer stores [U][2]
                    * (a form with RS_GROUP_SET_COUNTERS: the counter stores [U][2] too; with RS_GROUP_SET_SENT: the slots' sent rows are compared as well) */
  /* the nouns of the pair's messages: "specialised <adj>%s build", "both <adj>builds are dropped, <serves>", "agreed with <ref>",
   * "copies of the <stores>", "scheduler %d <lacks>: nothing for <entry> to build" (null: every scheduler of a group has the form) */
  const char *adj, *serves, *ref, *stores, *lacks, *entry;
  unsigned sets() const; /* the form's row of rs_group_form */
};
const GroupForm kGroupForms[RS_GROUP_FORMS] = {
    {false, kGroupPlain, 0, "", "the built-in kernels serve this group", "the built-in kernel field by field", "", nullptr, "rs_group_specialize"},
    {false, kGroupResident, 1, "resident ",
     "the built-in resident kernel serves this group's resident calls", "the built-in resident kernel field by field, resident stores included", "resident stores",
     nullptr, "rs_group_specialize_resident"},
    {true, kGroupQueued, 2, "queued ",
     "the built-in queued kernel serves this group's queued calls", "the built-in queued kernel field by field, bearer stores included", "bearer stores",
     "has no queued form (rs_group_set_bearers)", "rs_group_specialize_queued"},
    {true, kGroupFlows, 2, "flows ",
     "the built-in flows kernel serves this group's flows calls", "the built-in flows kernel field by field, bearer stores and counters included", "bearer stores and counters",
     "has no flows form (rs_group_set_flows)", "rs_group_specialize_flows"},
    {true, kGroupCounted, 2, "counted ",
     "the built-in counted kernel serves this group's counted calls", "the built-in counted kernel field by field, bearer stores, counters and sent rows included",
     "bearer stores and counters", "has no counted form (rs_group_set_counters)", "rs_group_specialize_counted"},
    {false, kGroupRun, 1, "run ",
     "the built-in run kernel serves this group's runs", "the built-in run kernel field by field over every TTI, resident stores included", "resident stores",
     "is not served by a run (rs_group_run_at)", "rs_group_specialize_run"},
    /* (the counted run: the run's launcher, no pair -- group_specialize_pair and group_jit_pair_status never see the row) */
    {false, -1, 0, "counted run ", "", "", "", nullptr, nullptr},
};
unsigned GroupForm::sets() const { return rs_group_form((int)(this - kGroupForms)).sets; }


/* The device stores of the resident forms, one row each, by GroupStoreId: [n_cells][elements per cell] of one element kind.  A family
 * is allocated together, all or none, by the first setter that needs it (group_alloc_family); rs_group_destroy, the setters' and
 * getters' row copies and the self-check (group_stores) all read a store's shape here. */
enum GroupStoreKind { kStoreI32, kStoreF64, kStoreI64, kStoreU8 }; /* every kind is compared bitwise; the kind is the element's size and how a message prints it */
enum GroupFamilyId { kFamCell, kFamAverages, kFamBearers, kFamCounters, kFamAvgCounters };
struct GroupStoreRow {
  const char* name;
  GroupStoreKind kind;
  int per_user;      /* elements per cell: per_user x U of the config (the update touches every user id, of the bearer stores BOTH bearers); 0: one */
  int family;
  bool zeroed;       /* by its allocation: read before a setter has written every cell's row */
  const char* field; /* in a message of the self-check, followed by the element's index; null: never compared */
  size_t size() const { return kind == kStoreI32 ? 4 : kind == kStoreU8 ? 1 : 8; }
  size_t elems(const rs_group* g) const { return per_user ? (size_t)per_user * g->b->U : 1; }
  size_t row_bytes(const rs_group* g) const { return size() * elems(g); }
  size_t bytes(const rs_group* g) const { return row_bytes(g) * (size_t)g->n_cells; }
  size_t kept(const rs_group* g) const { return (size_t)round_up((int)bytes(g), 256); }
};
const GroupStoreRow kGroupStores[kGroupNStores] = {
    {"ravg", kStoreF64, 1, kFamAverages, false, "avg"},         {"rpend", kStoreI32, 1, kFamAverages, false, "pending_bytes"},
    {"rlast", kStoreF64, 0, kFamCell, false, "last_update"},    {"rgather", kStoreF64, 1, kFamCell, false, nullptr},
    {"ruid", kStoreI32, 1, kFamCell, false, nullptr},           {"qavg", kStoreF64, 2, kFamBearers, false, "avg"},
    {"qpend", kStoreI32, 2, kFamBearers, false, "pending_bytes"}, {"qdata", kStoreI32, 2, kFamBearers, false, nullptr},
    {"qhas", kStoreU8, 2, kFamBearers, false, nullptr},         {"cbytes", kStoreI64, 2, kFamCounters, true, "cum_bytes"},
    {"crbs", kStoreI64, 2, kFamCounters, true, "cum_rbs"},      {"acbytes", kStoreI64, 1, kFamAvgCounters, true, "cum_bytes"},
    {"acrbs", kStoreI64, 1, kFamAvgCounters, true, "cum_rbs"},
};
/* a family: the family it stands on (made first, and left standing when this one fails), and the staged block of the slots' rows that
 * is made with it -- mapped when the group's block on that side is: the group reads its slots in place, the data words too; its
 * outputs are written in place, the sent rows too */
struct GroupFamily {
  int needs;
  GroupStaged rs_group::*staged;
  unsigned pin_flags;
  bool out_side;
};
const GroupFamily kGroupFamilies[] = {
    {-1, nullptr, 0, false},
    {kFamCell, nullptr, 0, false},
    {kFamCell, &rs_group::qin, hipHostMallocMapped, false},
    {-1, &rs_group::sent, hipHostMallocMapped | hipHostMallocCoherent, true},
    {-1, nullptr, 0, false},
};
/* the slots' staged rows: [n_cells][U][2] words */
size_t group_staged_bytes(const rs_group* g) { return 8 * (size_t)g->b->U * (size_t)g->n_cells; }

/* A family's stores and its staged block, all or none (true: they exist); the stores that are read before they are written start
 * as zeros.  A failure leaves nothing of the family behind. */
bool group_alloc_family(rs_group* g, int fam) {
  const GroupFamily& f = kGroupFamilies[fam];
  for (int i = 0; i < kGroupNStores; i++)
    if (kGroupStores[i].family == fam && g->store[i]) return true;
  bool ok = f.needs < 0 || group_alloc_family(g, f.needs);
  for (int i = 0; i < kGroupNStores && ok; i++)
    if (kGroupStores[i].family == fam) ok = hipMalloc(&g->store[i], kGroupStores[i].bytes(g)) == hipSuccess;
  if (ok && f.staged) ok = (g->*f.staged).make(group_staged_bytes(g), f.pin_flags, (f.out_side ? g->z_out : g->z_in) != nullptr);
  for (int i = 0; i < kGroupNStores && ok; i++)
    if (kGroupStores[i].family == fam && kGroupStores[i].zeroed) ok = hipMemset(g->store[i], 0, kGroupStores[i].bytes(g)) == hipSuccess;
  if (ok) return true;
  (void)hipGetLastError();
  for (int i = 0; i < kGroupNStores; i++)
    if (kGroupStores[i].family == fam && g->store[i]) {
      (void)hipFree(g->store[i]);
      g->store[i] = nullptr;
    }
  if (f.staged) (g->*f.staged).release();
  return false;
}

/* The stores that a form's self-check saves, restores and compares -- rows of kGroupStores, in the order they lie in a half of
 * rs_group::d_stores_chk[its pair] (each rounded up to 256 bytes): the averages, the cells' last-update times, the pending bytes. */
struct GroupStores {
  const int* row;
  int n;       /* 0, 3, or 5: a form that keeps counters (RS_GROUP_SET_COUNTERS) has m_cumulateBytes / m_cumulateRBs behind the other three */
  size_t half; /* bytes of one half of the check block */
};
GroupStores group_stores(const rs_group* g, const GroupForm& f) {
  static const int rows[3][5] = {{}, {kRavg, kRlast, kRpend}, {kQavg, kRlast, kQpend, kCbytes, kCrbs}}; /* by store_width */
  GroupStores s = {rows[f.store_width], !f.store_width ? 0 : (f.sets() & RS_GROUP_SET_COUNTERS) ? 5 : 3, 0};
  for (int i = 0; i < s.n; i++) s.half += kGroupStores[s.row[i]].kept(g);
  return s;
}
/* a form's stores to (save) or from one half of its pair's check block */
hipError_t group_copy_stores(const rs_group* g, const GroupForm& f, int half, bool save) {
  const GroupStores s = group_stores(g, f);
  uint8_t* kept = s.n ? g->d_stores_chk[f.pair] + (size_t)half * s.half : nullptr;
  for (int i = 0; i < s.n; kept += kGroupStores[s.row[i++]].kept(g)) {
    void* const dev = g->store[s.row[i]];
    const hipError_t e = hipMemcpyAsync(save ? (void*)kept : dev, save ? dev : (void*)kept, kGroupStores[s.row[i]].bytes(g), hipMemcpyDeviceToDevice, g->b->stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

rs_group* rs_group_create_checked(const rs_config* cfg, int32_t n_cells, int abi_version, size_t cfg_size) {
  return abi_matches(abi_version, cfg_size, sizeof(rs_config), "rs_config") ? rs_group_create(cfg, n_cells) : nullptr;
}

rs_group* rs_group_create(const rs_config* cfg, int32_t n_cells) {
  if (!cfg) { fail(RS_ERR_INVALID, "null config"); return nullptr; }
  if (n_cells < 1 || n_cells > RS_GROUP_MAX_CELLS) { fail(RS_ERR_INVALID, "n_cells %d outside 1..%d", n_cells, RS_GROUP_MAX_CELLS); return nullptr; }
  if (cfg->sched == RS_SCHED_NVS_NONGREEDY) {
    fail(RS_ERR_INVALID, "RS_SCHED_NVS_NONGREEDY is not served by a group (its draw block and kernels differ): use one rs_ctx per cell");
    return nullptr;
  }
  rs_batch_config bc;
  memset(&bc, 0, sizeof bc);
  bc.cell = *cfg;
  bc.n_cells = n_cells;
  bc.cqi_refresh = 1;
  rs_batch* b = batch_new(&bc, true);
  if (!b) return nullptr;
  if (b->threads > 512) { /* (the built-in kernels serve a group until rs_group_specialize, and beside its builds' checked calls) */
    fail(RS_ERR_INVALID, "a group needs the built-in kernels: %d threads per cell exceed their 512", b->threads);
    rs_batch_destroy(b);
    return nullptr;
  }
  rs_group* g = new (std::nothrow) rs_group();
  if (!g) { rs_batch_destroy(b); fail(RS_ERR_INVALID, "out of memory"); return nullptr; }
  g->b = b;
  g->n_cells = n_cells;
  const CtxLayout l = ctx_layout(b->U, b->R, b->S, b->G, false);
  g->in_stride = round_up((int)(RS_GROUP_HDR_BYTES + l.in_total), 256);
  g->out_stride = round_up((int)l.out_total, 256);
  g->flag_off = g->out_stride * (size_t)n_cells;
  g->out_slots = (size_t)n_cells;
  g->run_table_off = g->in_stride * (size_t)n_cells;
  const size_t in_bytes = g->run_table_off + (size_t)RS_GROUP_MAX_RUN * RS_GROUP_RUN_ROW_BYTES * (size_t)n_cells, out_bytes = g->flag_off + 64;
  g->img_stride = round_up(rs_upad_of(b->U) * b->R, 16);
  g->prb_stride = round_up(b->U * b->R * b->G, 16);
  const bool ok = hipMalloc(&g->d_in, in_bytes) == hipSuccess && hipMalloc(&g->d_out, out_bytes) == hipSuccess &&
                  hipMalloc(&g->d_count, 64) == hipSuccess && hipMemset(g->d_count, 0, 64) == hipSuccess &&
                  hipMalloc(&g->d_img, g->img_stride * (size_t)n_cells) == hipSuccess &&
                  hipHostMalloc((void**)&g->h_in, in_bytes, hipHostMallocMapped) == hipSuccess &&
                  hipHostMalloc((void**)&g->h_out, out_bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
  if (!ok) { fail(RS_ERR_HIP, "allocation of the group's staging blocks failed (%zu + %zu bytes)", in_bytes, out_bytes); rs_group_destroy(g); return nullptr; }
  const DropinEnv env = dropin_env();
  if (!env.force_copy) {
    void *zi = nullptr, *zo = nullptr;
    if (hipHostGetDevicePointer(&zi, g->h_in, 0) == hipSuccess && hipHostGetDevicePointer(&zo, g->h_out, 0) == hipSuccess) {
      g->z_in = (uint8_t*)zi;
      g->z_out = (uint8_t*)zo;
    }
  }
  memset(g->h_in, 0, in_bytes);
  memset(g->h_out, 0, out_bytes);
  g->timing = env.timing;
  g->poll = g->z_out != nullptr && env.poll;
  g->poll_us = env.poll_us;
  g->named.assign(n_cells, 0);
  g->packs.resize(n_cells);
  const char* im = getenv("RS_GROUP_IMAGE");
  g->image_on = !(im && im[0] == '0');
  g->img.resize(n_cells);
  g->modes.assign(n_cells, 0);
  const int ept = (b->R * b->S + b->threads - 1) / b->threads;
  for (int row = 0; row < RS_GROUP_FORMS; row++) { /* (a form without a kernel for the scheduler is never called: its name says <sched, 0>) */
    const int e = rs_group_form_serves(row, b->sched) ? rs_group_form_ept(b->sched, ept) : 0;
    snprintf(g->kname[row], sizeof g->kname[0], "%s<%d, %d>", rs_group_form(row).stem, b->sched, e > 0 ? e : 0);
    snprintf(g->kname_jit[row], sizeof g->kname_jit[0], "%s_jit", rs_group_form(row).stem);
  }
  g->empty_slot.assign(n_cells, 0);
  g->cells.assign(n_cells, GroupCellState());
  g_err[0] = 0;
  return g;
}

void rs_group_destroy(rs_group* g) {
  if (!g) return;
  if (g->timing && g->n_calls)
    fprintf(stderr, "rs_group_schedule_tti x %ld (%.1f cells per call): prepare %.2f us, enqueue %.2f us, wait %.2f us, unpack %.2f us per call (%ld completed by the polled word, %ld by the stream; cell-TTIs served from the cell's CQI image %lld, that stored one %lld, without a cqi_epoch %lld)\n",
            g->n_calls, (double)g->n_cell_ttis / g->n_calls, g->t_prep / g->n_calls, g->t_enq / g->n_calls, g->t_wait / g->n_calls,
            g->t_unpack / g->n_calls, g->n_polled, g->n_fallback, (long long)g->n_reused, (long long)g->n_stored, (long long)g->n_plain);
  if (g->timing && g->n_calls && g->t_recs > 0)
    fprintf(stderr, "rs_group_run_records_at: of the unpack above, %.2f us per call sort and copy grant records\n", g->t_recs / g->n_calls);
  if (g->b && g->b->stream) (void)hipStreamSynchronize(g->b->stream);
  for (void* q : {(void*)g->d_in, (void*)g->d_out, (void*)g->d_count, (void*)g->d_img, (void*)g->d_prb, (void*)g->d_out2, (void*)g->d_chk, (void*)g->d_recs})
    if (q) (void)hipFree(q);
  for (void* q : g->d_stores_chk)
    if (q) (void)hipFree(q);
  for (void* q : g->store) /* (the rows of kGroupStores) */
    if (q) (void)hipFree(q);
  for (GroupStaged* s : {&g->qin, &g->sent, &g->sent2}) s->release();
  for (void* q : {(void*)g->h_in, (void*)g->h_out, (void*)g->h_recs})
    if (q) (void)hipHostFree(q);
  rs_batch_destroy(g->b);
  delete g;
}

namespace {
/* Resident averages and the FP32 filter.  The metric scan's filter needs (1 + a) / 1000 (scheduler 1: a) inside [2^-60, 2^60] for every
 * average a (pack_tti); a resident average is not on the host to be inspected, so the library keeps it inside by construction:
 *   below   every update ends with `if (a < 1) a = 1` and rs_group_set_avg refuses a < 1: a >= 1, so a >= 2^-60 and (1 + a) / 1000 >= 2^-9;
 *   above   an update makes a' = 0.98 a + 0.02 rate, a weighted mean: a' <= max(a, rate) up to three roundings (2^-51 relative).
 *           rate = (double)(pending * 8) / dt with pending * 8 an int32 product, as the reference's (the device forms it so that it
 *           wraps where grants of calls that repeat one clock value pile up past 2^28 bytes; rs_group_set_pending refuses such
 *           values), so |rate| < 2^31 / dt whatever pending holds, and a call is
 *           refused unless dt = now - last_update is 0 (no update) or at least kResidentMinDt = 2^-20 s (a TTI is 2^-10 s): rate < 2^51.
 *           (A shorter interval is accepted while no byte can be pending -- no resident call since rs_group_set_avg or an all-zero
 *           rs_group_set_pending: rate = 0 / dt = 0 whatever dt > 0 is.  A run that starts as the reference's does, m_lastUpdate = 0.1
 *           and a first TTI at the clock's hundredth tick, 0.1 + 7e-17, needs that.)
 *           rs_group_set_avg refuses a > kResidentAvgMax = 2^52.  So a <= 2^52 (1 + 2^-51)^k after k updates, and 2^52 to 2^60 is a
 *           factor the roundings would need more than 2^53 updates for; (1 + a) / 1000 is smaller still.
 *   NaN     a finite, dt finite and > 0: no operation of the update makes one.
 * hol_delay is still the caller's and still switches a call to the exact scan. */
constexpr double kResidentAvgMax = 0x1p52;
constexpr double kResidentMinDt = 0x1p-20;
/* Resident bearers: a call position's average is a[b] of the one bearer with data or ((1 + a0) + a1) - 1, whose 1 + x must give back
 * (1 + a0) + a1 exactly -- it does while that sum is below 2^53 -- and must stay inside the filter's range: rs_group_set_bearers refuses
 * a > 2^51, and the growth argument above carries over bearer by bearer (the same update, |rate| < 2^51): a <= 2^51 (1 + 2^-51)^k. */
constexpr double kBearerAvgMax = 0x1p51;

/* what a call, a setter or a getter needs a cell to be; its refusal reads "cell %d is not <unmet>" */
struct CellNeed {
  GroupCellState::Form form;
  bool counters; /* the form's counters too */
  const char* unmet;
  bool met(const GroupCellState& s) const { return counters ? s.counted(form) : s.in(form); }
};
const CellNeed kNeedAverages = {GroupCellState::kAverages, false, "resident (rs_group_set_avg first)"},
               kNeedAveragesForCounters = {GroupCellState::kAverages, false, "average-resident (rs_group_set_avg first)"},
               kNeedAvgCounters = {GroupCellState::kAverages, true, "avg-counted (rs_group_set_avg_counters first)"},
               kNeedBearers = {GroupCellState::kBearers, false, "bearer-resident (rs_group_set_bearers first)"},
               kNeedCounters = {GroupCellState::kBearers, true, "counted (rs_group_set_counters first)"},
               kNeedFlows = {GroupCellState::kFlows, false, "flow-resident (rs_group_set_flows first)"};

/* One group call: what the caller gave, then what the phases of group_schedule decide along the way.  now != null: a resident form --
 * averages (rs_group_schedule_tti_at) or, with qdata, bearers (rs_group_schedule_tti_queued; counted: its twin,
 * rs_group_schedule_tti_counted, which differs in the kernel it launches, the two counter stores and the sent rows) or, with flow,
 * scheduler 1's flows (rs_group_schedule_tti_flows: a call position is bearer flow[k][i] of user user_id[i]). */
struct GroupCall {
  int32_t n;
  const int32_t* cell_ids;
  const rs_tti_in* in;
  rs_tti_out* out;
  const double* now;            /* [n], the resident forms; a run: [n][n_ttis] */
  const int32_t* const* qdata;  /* [n][n_users][2], queued and counted */
  int32_t* const* sent;         /* [n][n_users][2] or null, counted */
  const uint8_t* const* flow;   /* [n][n_users], flows */
  int form;                     /* kGroupPlain .. kGroupFlows */
  bool counted;
  /* group_validate: the presence of optional inputs is a per-launch switch of the kernel, the same for every cell of the call */
  bool has_prb, has_hol, has_prio, has_gate, want_upper;
  /* group_pack_slots: one cell outside the FP32 filter's range, the exact scan for all (same results); the per-PRB store failed in this call */
  bool exact_scan, store_failed_now;
  /* group_schedule: the kernel reads and writes the pinned blocks in place.  group_run: completion by the polled word; the run-time
   * build that serves the call (null: the form's built-in kernel; which: 0 general, 1 lean) and whether the built-in kernel ran beside it */
  bool zc, poll, checked;
  RsJitKernel* kd;
  int which;
  /* a run (rs_group_run_at; form is kGroupResident): n_ttis consecutive TTIs per slot, `in` given once per slot, `now` and `out` per
   * (slot, TTI), the rand() pairs in rands ([n][n_ttis][2] or null) */
  bool run;
  int32_t n_ttis;
  const int32_t* rands;
  /* a counted run (rs_group_run_counted_at; with run): the named cells' per-user counters are credited too; no_out: the caller wants no
   * per-TTI outputs (out == null) -- none is written, copied or unpacked */
  bool run_counted, no_out;
  /* grant records (rs_group_run_records_at; with run_counted): recs != null -- one list of rec_cap records and one count per (slot,
   * TTI) go to the caller; rec_dev is the lists' capacity on the device, min(rec_cap, the config's users) */
  int32_t rec_cap, rec_dev;
  rs_grant_record* recs;
  int32_t* n_recs;
  size_t rec_stride() const { return ((size_t)n_ttis * (size_t)rec_dev * sizeof(rs_grant_record) + 4 * (size_t)n_ttis + 31) / 32 * 32; } /* bytes per slot */
  int cell(int k) const { return cell_ids ? cell_ids[k] : k; }
  bool resident() const { return form != kGroupPlain; }
  int row() const { return run ? (run_counted ? (int)kGroupRunCounted : (int)kGroupRun) : counted ? (int)kGroupCounted : form; }
  int ttis() const { return run ? n_ttis : 1; }
  size_t at(int k, int t = 0) const { return run ? (size_t)k * (size_t)n_ttis + (size_t)t : (size_t)k; } /* slot k's TTI t in `now` and `out` */
  double now_first(int k) const { return now[at(k)]; }
  double now_last(int k) const { return now[at(k, ttis() - 1)]; }
  const GroupForm& desc() const { return kGroupForms[row()]; }
};

int group_schedule(rs_group* g, GroupCall c);
}  // namespace

int rs_group_schedule_tti(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, rs_tti_out* out) {
  if (!g || !in || !out) return fail(RS_ERR_INVALID, "null argument");
  return group_schedule(g, {n, cell_ids, in, out, nullptr, nullptr, nullptr, nullptr, kGroupPlain, false});
}

int rs_group_schedule_tti_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, rs_tti_out* out, const double* now) {
  if (!g || !in || !out || !now) return fail(RS_ERR_INVALID, "null argument");
  return group_schedule(g, {n, cell_ids, in, out, now, nullptr, nullptr, nullptr, kGroupResident, false});
}

int rs_group_schedule_tti_queued(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, rs_tti_out* out, const double* now,
                                 const int32_t* const* data_to_transmit) {
  if (!g || !in || !out || !now || !data_to_transmit) return fail(RS_ERR_INVALID, "null argument");
  return group_schedule(g, {n, cell_ids, in, out, now, data_to_transmit, nullptr, nullptr, kGroupQueued, false});
}

int rs_group_schedule_tti_counted(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, rs_tti_out* out, const double* now,
                                  const int32_t* const* data_to_transmit, int32_t* const* sent) {
  if (!g || !in || !out || !now || !data_to_transmit) return fail(RS_ERR_INVALID, "null argument");
  return group_schedule(g, {n, cell_ids, in, out, now, data_to_transmit, sent, nullptr, kGroupQueued, true});
}

int rs_group_schedule_tti_flows(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, rs_tti_out* out, const double* now,
                                const uint8_t* const* flow_bearer) {
  if (!g || !in || !out || !now || !flow_bearer) return fail(RS_ERR_INVALID, "null argument");
  return group_schedule(g, {n, cell_ids, in, out, now, nullptr, nullptr, flow_bearer, kGroupFlows, false});
}

int rs_group_run_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, int32_t n_ttis, const double* now, const int32_t* rands,
                    rs_tti_out* out) {
  if (!g || !in || !out || !now) return fail(RS_ERR_INVALID, "null argument");
  GroupCall c = {n, cell_ids, in, out, now, nullptr, nullptr, nullptr, kGroupResident, false};
  c.run = true;
  c.n_ttis = n_ttis;
  c.rands = rands;
  return group_schedule(g, c);
}

int rs_group_run_counted_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, int32_t n_ttis, const double* now,
                            const int32_t* rands, rs_tti_out* out) {
  if (!g || !in || !now) return fail(RS_ERR_INVALID, "null argument");
  GroupCall c = {n, cell_ids, in, out, now, nullptr, nullptr, nullptr, kGroupResident, false};
  c.run = c.run_counted = true;
  c.no_out = out == nullptr;
  c.n_ttis = n_ttis;
  c.rands = rands;
  return group_schedule(g, c);
}

/* most positions with a grant in one TTI of one cell.  Schedulers 1, 8, 9, 101 and 103 give an RBG to one user, and a
 * grant needs an RBG: min(users, RBGs).  UpperBound (10) counts an RBG for every slice that took it: a slice takes at most R entries of
 * its own list (rs_phase_p4.inc: k < quota inside a segment of R), a granted user leads at least one of them and belongs to one slice
 * of the config, whatever subset a call names: the sum over the slices of min(the slice's users, R) -- the config's users when every
 * slice has at most R of them.  (Nothing tighter follows from the quotas without a bound on the slice offsets they carry.) */
int rs_group_grant_bound(const rs_group* g) {
  if (!g) return fail(RS_ERR_INVALID, "null group");
  const rs_batch* b = g->b;
  if (b->sched != RS_SCHED_UPPERBOUND) return std::min(b->U, b->R);
  std::vector<int> per_slice((size_t)b->S, 0);
  for (int u = 0; u < b->U; u++) per_slice[(size_t)b->u2s[(size_t)u]]++;
  int bound = 0;
  for (int n_s : per_slice) bound += std::min(n_s, b->R);
  return bound;
}

int rs_group_run_records_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in, int32_t n_ttis, const double* now,
                            const int32_t* rands, rs_tti_out* out, int32_t rec_cap, rs_grant_record* recs, int32_t* n_recs) {
  if (!g || !in || !now) return fail(RS_ERR_INVALID, "null argument");
  if (!recs || !n_recs) return fail(RS_ERR_INVALID, "recs and n_recs must both be given (rs_group_run_counted_at is the run without records)");
  GroupCall c = {n, cell_ids, in, out, now, nullptr, nullptr, nullptr, kGroupResident, false};
  c.run = c.run_counted = true;
  c.no_out = out == nullptr;
  c.n_ttis = n_ttis;
  c.rands = rands;
  c.rec_cap = rec_cap;
  c.recs = recs;
  c.n_recs = n_recs;
  return group_schedule(g, c);
}

namespace {
/* a flows call's slot k (cell `cell`): positions are flows, (user, bearer) pairs in RRC-container order, each an existing bearer with
 * data to transmit */
int group_validate_flows_slot(const rs_group* g, const GroupCall& c, int k, int cell) {
  const rs_batch* b = g->b;
  const rs_tti_in& in = c.in[k];
  const int nf = in.n_users;
  if (nf > b->U) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): n_users %d (the call's flows) outside 0..%d", k, cell, nf, b->U);
  if (in.hol_delay || in.prio_has_data || in.required_rbs)
    return fail(RS_ERR_INVALID, "cell slot %d (cell %d): %s must be NULL in a flows call", k, cell,
                in.hol_delay ? "hol_delay" : (in.prio_has_data ? "prio_has_data" : "required_rbs"));
  if (nf > 0 && !c.flow[k]) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): flow_bearer[%d] is NULL (only an update-only slot, n_users == 0, gives none)", k, cell, k);
  if (nf > 0 && !in.data_to_transmit) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): data_to_transmit is required: a flow is scheduled because it has data", k, cell);
  const uint8_t* const has = g->has_bearer.data() + (size_t)cell * 2 * (size_t)b->U;
  int prev = -1;
  for (int i = 0; i < nf; i++) {
    const int id = in.user_id ? in.user_id[i] : i, fb = c.flow[k][i];
    if (id < 0 || id >= b->U) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): user id %d out of range", k, cell, id);
    if (fb > 1) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): flow_bearer[%d] = %d is neither 0 nor 1", k, cell, i, fb);
    if (2 * id + fb <= prev)
      return fail(RS_ERR_INVALID, "cell slot %d (cell %d): call position %d (user %d, bearer %d) does not ascend: flows come in (user, bearer) order, each once", k, cell, i, id, fb);
    prev = 2 * id + fb;
    if (!has[prev]) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): call position %d names bearer %d of user %d, which does not exist (rs_group_set_flows)", k, cell, i, fb, id);
    if (in.data_to_transmit[i] <= 0)
      return fail(RS_ERR_INVALID, "cell slot %d (cell %d): data_to_transmit[%d] = %d: a flow without data is not scheduled", k, cell, i, in.data_to_transmit[i]);
  }
  return RS_OK;
}

/* Every cell is validated before the device is touched: a rejected call is a no-op (g->named is scratch, cleared again). */
int group_validate(rs_group* g, GroupCall& c) {
  const rs_batch* b = g->b;
  const int n = c.n;
  const int32_t* const cell_ids = c.cell_ids;
  const rs_tti_in* const in = c.in;
  const bool slots0 = c.desc().slots0;
  if (n < 1 || n > g->n_cells) return fail(RS_ERR_INVALID, "n %d outside 1..%d (the group's cells)", n, g->n_cells);
  if (cell_ids) {
    int bad = -1, dup = -1;
    for (int k = 0; k < n && bad < 0 && dup < 0; k++) {
      const int cell = cell_ids[k];
      if (cell < 0 || cell >= g->n_cells) bad = k;
      else if (g->named[cell]) dup = k;
      else g->named[cell] = 1;
    }
    for (int k = 0; k < n; k++)
      if (cell_ids[k] >= 0 && cell_ids[k] < g->n_cells) g->named[cell_ids[k]] = 0;
    if (bad >= 0) return fail(RS_ERR_INVALID, "cell_ids[%d] = %d outside 0..%d", bad, cell_ids[bad], g->n_cells - 1);
    if (dup >= 0) return fail(RS_ERR_INVALID, "cell_ids[%d] = %d names a cell twice", dup, cell_ids[dup]);
  }
  if (c.run) {
    /* a run's own rules: what the host would change from TTI to TTI has no place in it */
    if (c.n_ttis < 1 || c.n_ttis > RS_GROUP_MAX_RUN) return fail(RS_ERR_INVALID, "n_ttis %d outside 1..%d (RS_GROUP_MAX_RUN)", c.n_ttis, RS_GROUP_MAX_RUN);
    if (b->sched == RS_SCHED_NVS)
      return fail(RS_ERR_INVALID, "RS_SCHED_NVS is not served by a run: the host picks the served slice, and with it the user list, per TTI");
    if (b->any_alpha)
      return fail(RS_ERR_INVALID, "a config with a customised slice (algo_alpha != 0) is not served by a run: hol_delay and prio_has_data change per TTI and belong to the host");
    if (!c.rands && b->sched != RS_SCHED_PF) return fail(RS_ERR_INVALID, "rands is NULL: only RS_SCHED_PF draws no rand() pair per TTI");
    if (g->run_table_off + (size_t)RS_GROUP_MAX_RUN * RS_GROUP_RUN_ROW_BYTES * (size_t)g->n_cells > (size_t)INT32_MAX)
      return fail(RS_ERR_INVALID, "the group's input block is too large for a run's 32-bit table offsets");
    for (int k = 0; k < n; k++) {
      const char* what = in[k].hol_delay ? "hol_delay" : in[k].prio_has_data ? "prio_has_data" : in[k].required_rbs ? "required_rbs"
                       : in[k].data_to_transmit ? "data_to_transmit" : nullptr;
      if (what) return fail(RS_ERR_INVALID, "cell slot %d: %s must be NULL in a run: it changes per TTI and belongs to the host", k, what);
      for (int t = 0; t < c.n_ttis && !c.no_out; t++)
        if (!c.out[c.at(k, t)].rbg_to_user || !c.out[c.at(k, t)].user_tbs_bits) return fail(RS_ERR_INVALID, "cell slot %d, TTI %d: null output array", k, t);
    }
  }
  auto gate_of = [&](const rs_tti_in& t) { return b->sched == RS_SCHED_NVS ? t.required_rbs : (b->sched == RS_SCHED_PF ? t.data_to_transmit : nullptr); };
  /* (a run without outputs has no upper_* lists to be uniform about: `at` is not dereferenced then) */
  auto upper_of = [&](size_t at) { return !c.no_out && b->sched == RS_SCHED_UPPERBOUND && (c.out[at].upper_rbg || c.out[at].upper_user); };
  /* (a call's update-only slots, n_users == 0, give no inputs at all: the slots WITH users agree among themselves) */
  int k0 = 0;
  while (slots0 && k0 < n && in[k0].n_users == 0) k0++;
  const bool any_users = k0 < n;
  if (!any_users) k0 = 0;
  c.has_prb = any_users && in[k0].cqi_prb != nullptr;
  c.has_hol = any_users && in[k0].hol_delay != nullptr;
  c.has_prio = any_users && in[k0].prio_has_data != nullptr;
  c.has_gate = any_users && gate_of(in[k0]) != nullptr;
  c.want_upper = any_users && upper_of(c.at(k0));
  for (int k = k0 + 1; k < n; k++) {
    if (slots0 && in[k].n_users == 0) continue;
    const char* what = (in[k].cqi_prb != nullptr) != c.has_prb ? "cqi_prb" : (in[k].hol_delay != nullptr) != c.has_hol ? "hol_delay"
                     : (in[k].prio_has_data != nullptr) != c.has_prio ? "prio_has_data"
                     : (gate_of(in[k]) != nullptr) != c.has_gate ? (b->sched == RS_SCHED_NVS ? "required_rbs" : "data_to_transmit")
                     : upper_of(c.at(k)) != c.want_upper ? "upper_rbg / upper_user" : nullptr;
    if (what) return fail(RS_ERR_INVALID, "mixed call: cell slot %d and cell slot %d differ in whether they give %s (optional inputs are given by every cell of a call or by none)", k, k0, what);
  }
  for (int k = 0; c.run && k < n; k++) /* (a run: every TTI's output, the slot's first included) */
    for (int t = 0; t < c.n_ttis; t++)
      if (upper_of(c.at(k, t)) != c.want_upper)
        return fail(RS_ERR_INVALID, "mixed call: cell slot %d, TTI %d and cell slot 0, TTI 0 differ in whether they give upper_rbg / upper_user (optional outputs are given by every TTI of every cell of a run or by none)", k, t);
  if (!c.resident()) return RS_OK;
  /* a resident call's cells: the form each is resident in, the slots' own inputs, the clock rules */
  const bool que = c.form == kGroupQueued, flw = c.form == kGroupFlows;
  if (b->gen_exp)
    return fail(RS_ERR_INVALID, "resident averages need exponents in {0, 1}: the general exponents' pow() of the averages is taken on the host per call");
  for (int k = 0; k < n; k++) {
    const int cell = c.cell(k);
    if (in[k].avg_rate) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): avg_rate must be NULL: the cell's averages are resident on the device", k, cell);
    const GroupCellState& st = g->cells[cell];
    auto unmet = [&](const CellNeed& need) { return fail(RS_ERR_STATE, "cell slot %d: cell %d is not %s", k, cell, need.unmet); };
    if (flw && !kNeedFlows.met(st)) return unmet(kNeedFlows);
    if (!flw && st.in(GroupCellState::kFlows))
      return fail(RS_ERR_STATE, "cell slot %d: cell %d is flow-resident (rs_group_set_flows): rs_group_schedule_tti_flows serves it, or rs_group_set_avg makes it average-resident", k, cell);
    if (que && !kNeedBearers.met(st)) return unmet(kNeedBearers);
    if (c.counted && !kNeedCounters.met(st)) return unmet(kNeedCounters);
    if (!que && st.in(GroupCellState::kBearers))
      return fail(RS_ERR_STATE, "cell slot %d: cell %d is bearer-resident (rs_group_set_bearers): rs_group_schedule_tti_queued serves it, or rs_group_set_avg makes it average-resident", k, cell);
    if (st.in(GroupCellState::kNone)) return unmet(kNeedAverages);
    if (c.run_counted && !kNeedAvgCounters.met(st)) return unmet(kNeedAvgCounters);
    if (slots0 && in[k].n_users < 0) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): n_users %d is negative", k, cell, in[k].n_users);
    if (int rc = flw ? group_validate_flows_slot(g, c, k, cell) : RS_OK) return rc;
    if (que && in[k].n_users > 0 && !c.qdata[k]) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): data_to_transmit[%d] is NULL (only an update-only slot, n_users == 0, gives none)", k, cell, k);
    const double last = st.last_update();
    const double now0 = c.now_first(k);
    if (!std::isfinite(now0)) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): now is not finite", k, cell);
    if (now0 < last) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): now = %.17g lies before the cell's last update at %.17g", k, cell, now0, last);
    if (now0 != last && !(now0 - last >= kResidentMinDt) && !st.pending_zero())
      return fail(RS_ERR_INVALID, "cell slot %d (cell %d): now - last_update = %.3g s is neither 0 nor at least %.3g s, and the cell may have bytes pending", k, cell, now0 - last, kResidentMinDt);
    /* (a run: behind its first TTI bytes may be pending whatever the cell's state was: every later step is 0 or at least the bound) */
    for (int t = 1; t < c.ttis(); t++) {
      const double a = c.now[c.at(k, t - 1)], z = c.now[c.at(k, t)];
      if (!std::isfinite(z)) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): now of TTI %d is not finite", k, cell, t);
      if (z != a && !(z - a >= kResidentMinDt))
        return fail(RS_ERR_INVALID, "cell slot %d (cell %d): the clock step from TTI %d to TTI %d, %.3g s, is neither 0 nor at least %.3g s", k, cell, t - 1, t, z - a, kResidentMinDt);
    }
  }
  if (c.recs) { /* grant records: behind the counted run's own rules */
    const int bound = rs_group_grant_bound(g);
    if (c.rec_cap < bound) return fail(RS_ERR_INVALID, "rec_cap %d is below rs_group_grant_bound, %d: a TTI's grants might not fit", c.rec_cap, bound);
    c.rec_dev = std::min(c.rec_cap, b->U); /* (a TTI has at most one grant per position) */
    if ((size_t)n * c.rec_stride() / 4 > (size_t)INT32_MAX) return fail(RS_ERR_INVALID, "the call's record blocks are too large (%zu bytes per slot)", c.rec_stride());
  }
  return RS_OK;
}

/* slot k's header (RsGroupCell, rs_device.h); l == null: an update-only slot -- its workgroup reads the header's cell, user count and
 * clock and nothing behind the header */
void group_fill_header(const rs_group* g, const GroupCall& c, int k, const CtxLayout* l) {
  const rs_batch* b = g->b;
  const rs_tti_in& in = c.in[k];
  RsGroupCell h;
  memset(&h, 0, sizeof h);
  h.cell = c.cell(k);
  if (l) {
    const int nu = in.n_users;
    h.image_mode = g->modes[k];
    h.U = nu;
    h.Upad = upad_of(nu);
    h.n_seg = b->base.n_seg;
    h.n_items = b->base.n_items;
    if (b->sched == RS_SCHED_PF) { h.n_seg = (nu + RS_PF_SEG - 1) / RS_PF_SEG; h.n_items = b->R * h.n_seg; }
    h.rand0 = c.run ? 0 : in.rand0; /* (a run: the pairs travel in the slot's table) */
    h.rand1 = c.run ? 0 : in.rand1;
    h.in_slice = (int32_t)l->slice; h.in_avg = (int32_t)l->avg; h.in_hol = (int32_t)l->hol; h.in_prio = (int32_t)l->prio;
    h.in_gate = (int32_t)l->gate; h.in_prb = (int32_t)l->prb;
    h.out_uinfo = (int32_t)l->uinfo; h.out_map = (int32_t)l->map; h.out_quota = (int32_t)l->quota; h.out_target = (int32_t)l->target;
    h.out_upper = (int32_t)l->upper;
    if (c.resident()) h.in_uid = in.user_id ? (int32_t)l->avg : 0; /* (l.avg lies behind the grid and the slice ids: never 0) */
  }
  if (c.resident()) h.now = c.now_first(k);
  if (c.run) { /* the slot's table, one row per TTI: the clock, rand0, rand1 */
    const size_t table = g->run_table_off + (size_t)k * RS_GROUP_MAX_RUN * RS_GROUP_RUN_ROW_BYTES;
    h.run_ttis = c.n_ttis;
    h.run_table = (int32_t)(table - (size_t)k * g->in_stride);
    h.run_out_step = (int32_t)g->out_stride;
    h.run_no_out = c.no_out ? 1 : 0;
    h.run_rec_cap = c.recs ? c.rec_dev : 0;
    for (int t = 0; t < c.n_ttis; t++) {
      const int32_t pair[2] = {c.rands ? c.rands[2 * c.at(k, t)] : 0, c.rands ? c.rands[2 * c.at(k, t) + 1] : 0};
      memcpy(g->h_in + table + (size_t)t * RS_GROUP_RUN_ROW_BYTES, &c.now[c.at(k, t)], 8);
      memcpy(g->h_in + table + (size_t)t * RS_GROUP_RUN_ROW_BYTES + 8, pair, 8);
    }
  }
  memcpy(g->h_in + (size_t)k * g->in_stride, &h, sizeof h);
}

/* a queued call's slot k: its data words, m_dataToTransmit[2] per call position, checked against the host's mirror of the cell's
 * bearers and copied to the word block */
int group_pack_data_words(rs_group* g, const GroupCall& c, int k, int cell) {
  const rs_batch* b = g->b;
  const rs_tti_in& in = c.in[k];
  const int32_t* const d = c.qdata[k];
  const uint8_t* const has = g->has_bearer.data() + (size_t)cell * 2 * (size_t)b->U;
  for (int i = 0; i < in.n_users; i++) {
    const int id = in.user_id ? in.user_id[i] : i;
    for (int bb = 0; bb < 2; bb++) {
      if (d[2 * i + bb] < 0) return fail(RS_ERR_INVALID, "cell slot %d (cell %d): data_to_transmit[%d][%d] = %d is negative", k, cell, i, bb, d[2 * i + bb]);
      if (d[2 * i + bb] > 0 && !has[2 * id + bb])
        return fail(RS_ERR_INVALID, "cell slot %d (cell %d): data_to_transmit[%d][%d] = %d, but user %d has no bearer of priority %d (rs_group_set_bearers)", k, cell, i, bb, d[2 * i + bb], id, bb);
    }
    if (d[2 * i] == 0 && d[2 * i + 1] == 0)
      return fail(RS_ERR_INVALID, "cell slot %d (cell %d): user %d (call position %d) has no data in either bearer: the reference does not schedule such a user", k, cell, id, i);
  }
  memcpy(g->qin.h + (size_t)k * 2 * (size_t)b->U, d, 8 * (size_t)in.n_users);
  return RS_OK;
}

/* Every slot's image mode, input block, words and header; then the per-PRB store.  Writes the group's pinned blocks and per-slot scratch. */
int group_pack_slots(rs_group* g, GroupCall& c) {
  rs_batch* b = g->b;
  const rs_tti_in* const in = c.in;
  const bool slots0 = c.desc().slots0;
  for (int k = 0; k < c.n; k++) {
    TtiPack& pk = g->packs[k];
    pk = TtiPack();
    const int cell = c.cell(k);
    g->empty_slot[k] = slots0 && in[k].n_users == 0;
    if (g->empty_slot[k]) {
      g->modes[k] = 0;
      pk.l = ctx_layout(0, b->R, b->S, b->G, false);
      group_fill_header(g, c, k, nullptr);
      continue;
    }
    /* rs_tti_in.cqi_epoch, decided per cell against the cell's record; without the switch or the per-PRB store no number counts */
    const uint64_t epoch = (g->image_on && !(c.has_prb && g->prb_store_failed)) ? in[k].cqi_epoch : 0;
    g->modes[k] = (uint8_t)g->img[cell].mode(in[k], c.has_prb, epoch);
    int rc = pack_tti(b, &in[k], c.no_out ? nullptr : &c.out[c.at(k)], g->h_in + (size_t)k * g->in_stride + RS_GROUP_HDR_BYTES, g->modes[k] == 2, &pk, c.resident(), c.form == kGroupFlows);
    if (rc) {
      char msg[sizeof g_err];
      snprintf(msg, sizeof msg, "%s", g_err);
      return fail(rc, "cell slot %d (cell %d): %.400s", k, cell, msg);
    }
    c.exact_scan |= pk.exact_scan;
    if (c.form == kGroupQueued && (rc = group_pack_data_words(g, c, k, cell))) return rc;
    if (c.form == kGroupFlows) { /* the slot's bearer words, one per call position (checked by group_validate) */
      int32_t* const w = g->qin.h + (size_t)k * 2 * (size_t)b->U;
      for (int i = 0; i < in[k].n_users; i++) w[i] = c.flow[k][i];
    }
    group_fill_header(g, c, k, &pk.l);
  }
  /* the per-PRB store comes with the first call that gives per-PRB reports under a number.  (Until it exists no record says "per-PRB",
   * so such a call holds no reuse slot yet.)  Without it those calls are served as if they made no promise: same results. */
  if (c.has_prb && !g->d_prb && !g->prb_store_failed) {
    bool wanted = false;
    for (int k = 0; k < c.n; k++) wanted |= g->modes[k] != 0;
    if (wanted && hipMalloc(&g->d_prb, g->prb_stride * (size_t)g->n_cells) != hipSuccess) {
      (void)hipGetLastError();
      g->d_prb = nullptr;
      g->prb_store_failed = c.store_failed_now = true;
    }
  }
  if (c.has_prb && !g->d_prb)
    for (int k = 0; k < c.n; k++) {
      g->modes[k] = 0;
      ((RsGroupCell*)(g->h_in + (size_t)k * g->in_stride))->image_mode = 0;
    }
  return RS_OK;
}

/* from the first operation on the stream on, a failure leaves the named cells' images in an unknown state */
struct ImageGuard {
  rs_group* g;
  const GroupCall& c;
  bool ok;
  ~ImageGuard() {
    if (!ok) for (int k = 0; k < c.n; k++) {
      g->img[c.cell(k)].valid = false;
      if (c.resident()) g->cells[c.cell(k)].leave(); /* (averages half updated, perhaps: resident again with rs_group_set_avg; neither resident nor counted) */
    }
  }
};

/* the call's launch block: the config's, the group's stores, and of the form's stores those that its row names */
void group_fill_launch(const rs_group* g, const GroupCall& c, RsLaunch* launch) {
  const rs_batch* b = g->b;
  const unsigned sets = c.desc().sets();
  uint8_t* const dev_in = c.zc ? g->z_in : g->d_in;
  uint8_t* const dev_out = c.zc ? g->z_out : g->d_out;
  RsLaunch& L = *launch;
  L = b->base;
  L.n_cells = c.n; /* call slots of this launch */
  L.n_ttis = 1;
  L.direct = 1;
  L.cqi_mode = RS_CQI_EPOCHS;
  L.refresh = 1;
  L.n_epochs = 1;
  L.image_mode = 0; /* (per slot: RsGroupCell::image_mode) */
  L.grid_image = nullptr;
  L.grp_image = g->d_img;
  L.grp_image_stride = (int64_t)g->img_stride;
  L.grp_prb = g->d_prb;
  L.grp_prb_stride = (int64_t)g->prb_stride;
  L.queue_mode = b->any_alpha ? 1 : 0;
  L.exact_scan = c.exact_scan ? 1 : 0;
  L.gen_exp = b->gen_exp ? 1 : 0;
  L.gen_num = b->d_gen_num;
  /* given / not given; the workgroups take the addresses from their slots */
  L.prb_cqi = c.has_prb ? dev_in : nullptr;
  L.gate = c.has_gate ? (const int32_t*)dev_in : nullptr;
  L.log_upper = c.want_upper ? (int32_t*)dev_out : nullptr;
  L.grp_in = dev_in;
  L.grp_out = dev_out;
  L.grp_in_stride = (int64_t)g->in_stride;
  L.grp_out_stride = (int64_t)g->out_stride * c.ttis(); /* (a run: a slot's TTIs follow one another) */
  L.grp_count = g->d_count;
  if (sets & RS_GROUP_SET_CELL) {
    L.grp_last = (double*)g->store[kRlast];
    L.grp_gather = (double*)g->store[kRgather];
    L.grp_uid = (int32_t*)g->store[kRuid];
  }
  if (sets & RS_GROUP_SET_AVERAGES) {
    L.grp_avg = (double*)g->store[kRavg];
    L.grp_pending = (int32_t*)g->store[kRpend];
  }
  if (sets & RS_GROUP_SET_BEARERS) {
    L.grp_qavg = (double*)g->store[kQavg];
    L.grp_qpend = (int32_t*)g->store[kQpend];
    L.grp_qhas = (uint8_t*)g->store[kQhas];
    L.grp_qin = g->qin.dev();
    L.grp_qin_stride = 2 * (int64_t)b->U;
  }
  if (sets & RS_GROUP_SET_DATA) L.grp_qdata = (int32_t*)g->store[kQdata];
  if (sets & RS_GROUP_SET_COUNTERS) { /* (a cell is resident in one form at a time: the bearers' [U][2] stores, or a counted run's [U] stores) */
    L.grp_cbytes = (int64_t*)g->store[c.run_counted ? kAcbytes : kCbytes];
    L.grp_crbs = (int64_t*)g->store[c.run_counted ? kAcrbs : kCrbs];
  }
  if (sets & RS_GROUP_SET_SENT) {
    L.grp_sent = g->sent.dev();
    L.grp_sent_stride = 2 * (int64_t)b->U;
  }
  if (c.recs) { /* (a counted run has no sent rows: the two words carry its record blocks, device memory, words per slot) */
    L.grp_sent = (int32_t*)g->d_recs;
    L.grp_sent_stride = (int64_t)(c.rec_stride() / 4);
  }
}

/* A checked call -- one call, or one whole run --: the form's built-in kernel first, on the same slots and the same state, its outputs
 * into slots of its own.  What it
 * left is kept, what it found is put back: the run-time build starts from the same state.  (A mode-1 slot: BOTH kernels transpose the
 * slot's block and store the cell's image and per-PRB copy -- the same bytes when the build is right; a wrong image shows in the
 * checked calls that read it.) */
int group_run_twin(rs_group* g, const GroupCall& c, const RsLaunch& L) {
  rs_batch* b = g->b;
  hipStream_t st = b->stream;
  const GroupForm& f = c.desc();
  const TwinState tw{g->b, g->d_chk, g->n_cells}; /* (every cell of the group, named or not) */
  if (const int rc = tw.save()) return rc;
  HIP_TRY(group_copy_stores(g, f, 0, true));
  RsLaunch Lb = L;
  Lb.grp_out = g->d_out2;
  Lb.log_upper = c.want_upper ? (int32_t*)g->d_out2 : nullptr;
  Lb.done_flag = nullptr;
  if (f.sets() & RS_GROUP_SET_SENT) { /* (the sent rows are outputs too: the built-in kernel's go to the twin block, whatever the caller asked for) */
    /* (pinned and mapped when the first block is, else a device block copied back; made by the first checked call) */
    if (!g->sent2.h && !g->sent2.make(group_staged_bytes(g), hipHostMallocMapped | hipHostMallocCoherent, !g->sent.copied())) {
      (void)hipGetLastError();
      return fail(RS_ERR_HIP, "allocation of the self-check's twin sent block failed (%zu bytes)", group_staged_bytes(g));
    }
    Lb.grp_sent = g->sent2.dev();
  }
  HIP_TRY(rs_launch_group(&Lb, b->threads, c.row(), st));
  HIP_TRY(hipMemcpyAsync(g->h_out2.data(), g->d_out2, (size_t)c.n * c.ttis() * g->out_stride, hipMemcpyDeviceToHost, st)); /* (a run: slots x TTIs) */
  if ((f.sets() & RS_GROUP_SET_SENT) && g->sent2.copied()) HIP_TRY(hipMemcpyAsync(g->sent2.h, g->sent2.d, 8 * (size_t)c.n * b->U, hipMemcpyDeviceToHost, st));
  if (const int rc = tw.keep_and_put_back()) return rc;
  HIP_TRY(group_copy_stores(g, f, 1, true));
  HIP_TRY(group_copy_stores(g, f, 0, false));
  return RS_OK;
}

/* The copies in, the launch, the copies back.  The form's run-time pair serves the call when it has one -- its lean build when the call
 * is plain for every cell (the uniform-presence rules make that a fact of the launch; a call of update-only slots only has no facts
 * and takes the lean build too), the general one otherwise.  A build without the self-check mark serves its first calls beside the
 * built-in kernel of its form (group_run_twin, group_check). */
int group_run(rs_group* g, GroupCall& c, RsLaunch& L) {
  rs_batch* b = g->b;
  hipStream_t st = b->stream;
  const GroupForm& f = c.desc();
  /* per-PRB reports and queue state are read again and again inside the TTI: those calls keep the device copies.  (The copy sends
   * whole slots: a reuse slot's grid area and per-PRB block travel stale and are not read.) */
  if (!c.zc) HIP_TRY(hipMemcpyAsync(g->d_in, g->h_in, (size_t)c.n * g->in_stride, hipMemcpyHostToDevice, st));
  if (!c.zc && c.run)
    HIP_TRY(hipMemcpyAsync(g->d_in + g->run_table_off, g->h_in + g->run_table_off, (size_t)c.n * RS_GROUP_MAX_RUN * RS_GROUP_RUN_ROW_BYTES, hipMemcpyHostToDevice, st));
  if ((f.sets() & RS_GROUP_SET_BEARERS) && g->qin.copied()) HIP_TRY(hipMemcpyAsync(g->qin.d, g->qin.h, 8 * (size_t)c.n * b->U, hipMemcpyHostToDevice, st));
  c.poll = c.zc && g->poll && !c.recs; /* (records come back by a copy on the stream: the stream says when) */
  if (c.poll) {
    if (++g->seq == 0) g->seq = 1; /* (0 is the word's initial value) */
    L.done_flag = (uint32_t*)(g->z_out + g->flag_off);
    L.done_seq = g->seq;
  }
  static const JitPair no_pair{}; /* (a form without run-time builds: nothing wanted, nothing built) */
  const JitPair& p = f.pair >= 0 ? g->pair[f.pair] : no_pair;
  /* (a flows call always carries the data_to_transmit gate: its lean build keeps it) */
  const bool gate_free = c.form == kGroupFlows || !c.has_gate;
  const bool lean = p.jit[1] && !c.has_prb && !L.queue_mode && gate_free && !L.exact_scan && !L.gen_exp && !c.want_upper && !L.synthetic;
  c.which = lean ? 1 : 0;
  c.kd = p.jit[c.which];
  c.checked = c.kd != nullptr && p.chk_left[c.which] > 0;
  if (c.checked) {
    const int rc = group_run_twin(g, c, L);
    if (rc) return rc;
    L.done_flag = nullptr; /* completion by the stream */
  }
  if (c.kd) HIP_TRY(rs_jit_launch(c.kd, &L, st));
  else HIP_TRY(rs_launch_group(&L, b->threads, c.row(), st));
  g->launches++;
  g->last_call_form = c.row();
  g->last_call_jit = c.kd != nullptr;
  if (!c.zc && !c.no_out) HIP_TRY(hipMemcpyAsync(g->h_out, g->d_out, (size_t)c.n * c.ttis() * g->out_stride, hipMemcpyDeviceToHost, st));
  if ((f.sets() & RS_GROUP_SET_SENT) && g->sent.copied()) HIP_TRY(hipMemcpyAsync(g->sent.h, g->sent.d, 8 * (size_t)c.n * b->U, hipMemcpyDeviceToHost, st));
  if (c.recs) HIP_TRY(hipMemcpyAsync(g->h_recs, g->d_recs, (size_t)c.n * c.rec_stride(), hipMemcpyDeviceToHost, st));
  return RS_OK;
}

/* by the polled word (the last workgroup to finish publishes the sequence number behind every workgroup's outputs), else by the stream */
int group_wait(rs_group* g, const GroupCall& c) {
  bool seen = false;
  if (c.poll && !c.checked) seen = poll_done_word(g->h_out + g->flag_off, g->seq, g->poll_us, &g->n_polled, g->b->stream);
  if (!seen) {
    g->n_fallback++; /* (a group counts every stream wait) */
    HIP_TRY(hipStreamSynchronize(g->b->stream));
  }
  return RS_OK;
}

/* the form's stores of the named cells, as the run-time build left them against what the built-in kernel left (the second half of the
 * check block): per cell the averages, then the pending bytes, then the last-update time, then the two counters of a form that keeps them */
int group_compare_stores(const rs_group* g, const GroupCall& c, char* what, size_t len) {
  const GroupForm& f = c.desc();
  const GroupStores s = group_stores(g, f);
  if (!s.n) return RS_OK;
  std::vector<uint8_t> jit[5], ref[5];
  const uint8_t* kept = g->d_stores_chk[f.pair] + s.half;
  for (int i = 0; i < s.n; kept += kGroupStores[s.row[i++]].kept(g)) {
    const size_t bytes = kGroupStores[s.row[i]].bytes(g);
    jit[i].resize(bytes);
    ref[i].resize(bytes);
    HIP_TRY(hipMemcpy(jit[i].data(), g->store[s.row[i]], bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ref[i].data(), kept, bytes, hipMemcpyDeviceToHost));
  }
  for (int k = 0; k < c.n && !what[0]; k++) {
    const int cell = c.cell(k);
    for (const int i : {0, 2, 1, 3, 4}) {
      if (i >= s.n) continue;
      const GroupStoreRow& x = kGroupStores[s.row[i]];
      const size_t elems = x.elems(g);
      for (size_t j = 0; j < elems && !what[0]; j++) {
        const size_t at = ((size_t)cell * elems + j) * x.size();
        const void *a = jit[i].data() + at, *r = ref[i].data() + at;
        if (memcmp(a, r, x.size()) == 0) continue;
        char idx[48] = ""; /* (the element's index behind the store's name: "avg[3]", "avg[3][1]", "last_update") */
        if (elems > 1 && f.store_width == 2) snprintf(idx, sizeof idx, "[%zu][%zu]", j / 2, j % 2);
        else if (elems > 1) snprintf(idx, sizeof idx, "[%zu]", j);
        if (x.kind == kStoreF64) snprintf(what, len, "cell %d: %s%s = %a, the built-in kernel's %a", cell, x.field, idx, *(const double*)a, *(const double*)r);
        else if (x.kind == kStoreI64) snprintf(what, len, "cell %d: %s%s = %lld, the built-in kernel's %lld", cell, x.field, idx, (long long)*(const int64_t*)a, (long long)*(const int64_t*)r);
        else snprintf(what, len, "cell %d: %s%s = %d, the built-in kernel's %d", cell, x.field, idx, *(const int32_t*)a, *(const int32_t*)r);
      }
    }
  }
  return RS_OK;
}

/* A checked call disagreed: the pair is wrong, neither of its builds is trusted.  Both are dropped (and their cache files); the other
 * pairs stay.  This call returns the built-in kernel's outputs and leaves its state, the form's stores included; later calls of the
 * form run the built-in kernel. */
int group_drop_pair(rs_group* g, const GroupCall& c, const char* what) {
  rs_batch* b = g->b;
  const GroupForm& f = c.desc();
  JitPair& p = g->pair[f.pair];
  jit_pair_drop(&p);
  g->last_call_jit = false;
  memcpy(g->h_out, g->h_out2.data(), (size_t)c.n * c.ttis() * g->out_stride);
  if (f.sets() & RS_GROUP_SET_SENT) memcpy(g->sent.h, g->sent2.h, 8 * (size_t)c.n * b->U); /* (the built-in kernel's sent rows: what group_unpack hands out) */
  if (const int rc = TwinState{g->b, g->d_chk, g->n_cells}.restore_kept()) return rc;
  if (f.store_width) {
    HIP_TRY(group_copy_stores(g, f, 1, false));
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  snprintf(p.msg, sizeof p.msg, "self-check of the group's specialised %s%s build, checked call %d: %s; both %sbuilds are dropped, %s (lint the code object: "
           "tools/lint_exec_restore.py)", f.adj, c.which ? "lean" : "general", p.chk_agreed[c.which] + 1, what, f.adj, f.serves);
  snprintf(g_err, sizeof g_err, "%s", p.msg);
  return RS_OK;
}

/* a checked call's end: every named cell's output fields and the state left behind must agree with the built-in kernel's -- the slice
 * state and the form's stores; slot by slot, field by field, the first difference is the message */
int group_check(rs_group* g, const GroupCall& c) {
  const rs_batch* b = g->b;
  TwinState tw{g->b, g->d_chk, g->n_cells};
  if (const int rc = tw.fetch()) return rc;
  char what[240] = "";
  for (int k = 0; k < c.n && !what[0]; k++) {
    const int cell = c.cell(k);
    /* (an update-only slot: its workgroup wrote no output, the state alone is compared; a run: every TTI's block of the slot) */
    for (int t = 0; t < c.ttis() && !g->empty_slot[k] && !what[0]; t++) {
      const size_t at = c.at(k, t) * g->out_stride;
      compare_out_block(g->h_out + at, g->h_out2.data() + at, g->packs[k].l, b->R, b->S, c.in[k].n_users, c.want_upper, cell, what, sizeof what, c.run ? t : -1);
    }
    tw.compare(cell, cell, what, sizeof what);
    /* (a counted call: the slot's sent rows, whether or not the caller wants them; an update-only slot has none) */
    if ((c.desc().sets() & RS_GROUP_SET_SENT) && !g->empty_slot[k]) {
      const int32_t *a = g->sent.h + (size_t)k * 2 * (size_t)b->U, *r = g->sent2.h + (size_t)k * 2 * (size_t)b->U;
      for (int j = 0; j < 2 * c.in[k].n_users && !what[0]; j++)
        if (a[j] != r[j]) snprintf(what, sizeof what, "cell %d: sent[%d][%d] = %d, the built-in kernel's %d", cell, j / 2, j % 2, a[j], r[j]);
    }
  }
  if (!what[0]) {
    const int rc = group_compare_stores(g, c, what, sizeof what);
    if (rc) return rc;
  }
  if (what[0]) return group_drop_pair(g, c, what);
  jit_pair_agreed(&g->pair[c.desc().pair], c.which);
  return RS_OK;
}

/* the launch has completed: a resident call's updates are dated now[k], and grants may be waiting */
void group_commit_clocks(rs_group* g, const GroupCall& c) {
  if (!c.resident()) return;
  for (int k = 0; k < c.n; k++) g->cells[c.cell(k)].served(!g->empty_slot[k], c.now_first(k), c.now_last(k));
}

/* ... and the device holds these calls' reports now: the cells' image records, the statistics */
void group_commit_images(rs_group* g, const GroupCall& c) {
  for (int k = 0; k < c.n; k++) {
    if (g->empty_slot[k]) continue; /* (no reports, no image moved, not counted) */
    const int mode = g->modes[k];
    CqiImage& im = g->img[c.cell(k)];
    /* (a run, as the calls it stands for: its later TTIs read what TTI 0 read -- the slot's blocks again without a number, else the image) */
    const int64_t later = c.ttis() - 1;
    if (mode == 0) { g->n_plain += 1 + later; im.valid = false; continue; } /* (as a context: a call without a number ends the image's term) */
    if (mode == 2) { g->n_reused += 1 + later; continue; }
    g->n_stored++;
    g->n_reused += later;
    im.stored(c.in[k], c.has_prb);
  }
}

void group_unpack(const rs_group* g, const GroupCall& c) {
  const rs_batch* b = g->b;
  for (int k = 0; k < c.n; k++) {
    rs_tti_out& out = c.out[k];
    if (g->empty_slot[k]) { /* "nothing scheduled": the workgroup wrote no output */
      if (out.rbg_to_user) for (int r = 0; r < b->R; r++) out.rbg_to_user[r] = -1;
      for (int s = 0; s < b->S; s++) {
        if (out.target_rbs) out.target_rbs[s] = 0;
        if (out.quota_rbgs) out.quota_rbgs[s] = 0;
      }
      if (out.upper_rbg) for (int i = 0; i < b->S * b->R; i++) out.upper_rbg[i] = -1;
      if (out.upper_user) for (int i = 0; i < b->S * b->R; i++) out.upper_user[i] = -1;
      continue;
    }
    if (c.run) { /* output slot (k, t) is a single call's output block */
      for (int t = 0; t < c.n_ttis; t++) unpack_tti(b, &c.in[k], &c.out[c.at(k, t)], g->h_out + c.at(k, t) * g->out_stride, g->packs[k].l, c.want_upper);
      continue;
    }
    unpack_tti(b, &c.in[k], &out, g->h_out + (size_t)k * g->out_stride, g->packs[k].l, c.want_upper, c.form == kGroupFlows ? c.flow[k] : nullptr);
    /* (a counted call: the slot's sent rows, [n_users][2] in call order, written by the threads that credited the positions) */
    if (c.counted && c.sent && c.sent[k]) memcpy(c.sent[k], g->sent.h + (size_t)k * 2 * (size_t)b->U, 8 * (size_t)c.in[k].n_users);
  }
}

/* A run needs slots x TTIs output slots: the device block and the pinned, mapped block grow to the largest run so far, the completion word
 * moves behind the new last slot.  Between two calls the stream is idle and nothing points into the old blocks.  The new blocks are made
 * before the old ones go: a failure leaves the group as it was. */
int group_grow_out(rs_group* g, size_t slots) {
  if (slots <= g->out_slots) return RS_OK;
  const size_t flag_off = g->out_stride * slots, bytes = flag_off + 64;
  uint8_t *d = nullptr, *h = nullptr, *d2 = nullptr;
  void* z = nullptr;
  bool ok = hipMalloc(&d, bytes) == hipSuccess && hipHostMalloc((void**)&h, bytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
  if (ok && g->z_out) ok = hipHostGetDevicePointer(&z, h, 0) == hipSuccess;
  /* (the self-check's twin output slots, once a pair has made them: a checked run writes slots x TTIs of them too) */
  if (ok && g->d_out2) ok = hipMalloc(&d2, flag_off) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (d2) (void)hipFree(d2);
    return fail(RS_ERR_HIP, "allocation of the run's output blocks failed (%zu bytes each)", bytes);
  }
  memset(h, 0, bytes);
  if (d2) {
    (void)hipFree(g->d_out2);
    g->d_out2 = d2;
    g->h_out2.assign(flag_off, 0);
  }
  (void)hipFree(g->d_out);
  (void)hipHostFree(g->h_out);
  g->d_out = d;
  g->h_out = h;
  if (g->z_out) g->z_out = (uint8_t*)z;
  g->out_slots = slots;
  g->flag_off = flag_off;
  return RS_OK;
}

/* The record blocks of a call with grant records: device block and pinned twin grow to the largest call so far; new blocks first, a
 * failure leaves the group as it was. */
int group_grow_recs(rs_group* g, size_t bytes) {
  if (bytes <= g->recs_bytes) return RS_OK;
  uint8_t *d = nullptr, *h = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc((void**)&h, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    return fail(RS_ERR_HIP, "allocation of the run's record blocks failed (%zu bytes each)", bytes);
  }
  if (g->d_recs) (void)hipFree(g->d_recs);
  if (g->h_recs) (void)hipHostFree(g->h_recs);
  g->d_recs = d;
  g->h_recs = h;
  g->recs_bytes = bytes;
  return RS_OK;
}

/* The caller's records: per (slot, TTI) the count, and the list in ascending position -- the device fills a list in the order its waves
 * arrive, a position occurs once per TTI, so an insertion sort by position over at most rec_dev records makes the order the ABI
 * promises, whatever the arrival order was.  A count above the capacity: the device wrote nothing behind the capacity; the count goes
 * to the caller as it is and the call fails (the bound of rs_group_grant_bound would be wrong). */
int group_unpack_records(const rs_group* g, const GroupCall& c) {
  int bad_k = -1, bad_t = -1, bad_n = 0;
  for (int k = 0; k < c.n; k++) {
    const uint8_t* const slot = g->h_recs + (size_t)k * c.rec_stride();
    const int32_t* const counts = (const int32_t*)(slot + (size_t)c.n_ttis * (size_t)c.rec_dev * sizeof(rs_grant_record));
    for (int t = 0; t < c.n_ttis; t++) {
      const int count = counts[t];
      c.n_recs[c.at(k, t)] = count;
      if ((count < 0 || count > c.rec_dev) && bad_k < 0) { bad_k = k; bad_t = t; bad_n = count; }
      const int m = count < 0 ? 0 : std::min(count, (int)c.rec_dev);
      const rs_grant_record* const src = (const rs_grant_record*)slot + (size_t)t * (size_t)c.rec_dev;
      rs_grant_record* const dst = c.recs + c.at(k, t) * (size_t)c.rec_cap;
      for (int j = 0; j < m; j++) {
        int at = j;
        for (; at > 0 && dst[at - 1].pos > src[j].pos; at--) dst[at] = dst[at - 1];
        dst[at] = src[j];
      }
    }
  }
  if (bad_k >= 0)
    return fail(RS_ERR_STATE, "cell slot %d (cell %d), TTI %d: the device counted %d grants, the record list holds %d (rs_group_grant_bound is wrong for this config); the call's state and counters are complete, the TTI's records are not",
                bad_k, c.cell(bad_k), bad_t, bad_n, (int)c.rec_dev);
  return RS_OK;
}

/* one group call, phase by phase; RS_DROPIN_TIMING splits it into prepare, enqueue, wait and unpack */
int group_schedule(rs_group* g, GroupCall c) {
  rs_batch* b = g->b;
  using clk = std::chrono::steady_clock;
  const clk::time_point t0 = g->timing ? clk::now() : clk::time_point();
  int rc = group_validate(g, c);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  if ((rc = group_pack_slots(g, c))) return rc;
  ImageGuard guard{g, c, false};
  if (c.run && !c.no_out && (rc = group_grow_out(g, (size_t)c.n * (size_t)c.n_ttis))) return rc;
  if (c.recs && (rc = group_grow_recs(g, (size_t)c.n * c.rec_stride()))) return rc;
  const clk::time_point t1 = g->timing ? clk::now() : clk::time_point();
  c.zc = g->z_in != nullptr && !c.has_prb && !b->any_alpha;
  RsLaunch L;
  group_fill_launch(g, c, &L);
  if ((rc = group_run(g, c, L))) return rc;
  const clk::time_point t2 = g->timing ? clk::now() : clk::time_point();
  if ((rc = group_wait(g, c))) return rc;
  if (c.checked && (rc = group_check(g, c))) return rc;
  guard.ok = true;
  group_commit_clocks(g, c);
  const clk::time_point t3 = g->timing ? clk::now() : clk::time_point();
  group_commit_images(g, c);
  if (!c.no_out) group_unpack(g, c);
  const clk::time_point t3r = g->timing ? clk::now() : clk::time_point();
  const int rc_recs = c.recs ? group_unpack_records(g, c) : RS_OK;
  if (g->timing) {
    const clk::time_point t4 = clk::now();
    if (c.recs) g->t_recs += std::chrono::duration<double, std::micro>(t4 - t3r).count();
    auto us = [](clk::time_point a, clk::time_point b2) { return std::chrono::duration<double, std::micro>(b2 - a).count(); };
    g->t_prep += us(t0, t1);
    g->t_enq += us(t1, t2);
    g->t_wait += us(t2, t3);
    g->t_unpack += us(t3, t4);
    g->n_calls++;
    g->n_cell_ttis += (long)c.n * c.ttis();
  }
  if (c.store_failed_now && !rc_recs) /* (a failed record check keeps its own message) */
    snprintf(g_err, sizeof g_err, "note: the group's per-PRB report store (%zu bytes) could not be allocated: calls with cqi_prb are served as if "
             "cqi_epoch were 0 from now on (same results, the block is sent on every call)", g->prb_stride * (size_t)g->n_cells);
  return rc_recs;
}
}  // namespace

namespace {
/* The shared pieces of the setters and getters of a cell's resident state (none of them is part of a TTI).  The prelude: the group,
 * the cell, the state the call needs the cell in (null: any), then -- for a call with nothing to validate or allocate in between,
 * else by group_cell_sync behind that -- the device and an idle stream, before any copy. */
int group_cell_sync(rs_group* g) {
  HIP_TRY(hipSetDevice(g->b->cfg.cell.device));
  HIP_TRY(hipStreamSynchronize(g->b->stream));
  return RS_OK;
}
int group_cell_prelude(rs_group* g, int32_t cell, const CellNeed* need, bool sync) {
  if (!g) return fail(RS_ERR_INVALID, "null group");
  if (cell < 0 || cell >= g->n_cells) return fail(RS_ERR_INVALID, "cell %d outside 0..%d", cell, g->n_cells - 1);
  if (need && !need->met(g->cells[cell])) return fail(RS_ERR_STATE, "cell %d is not %s", cell, need->unmet);
  return sync ? group_cell_sync(g) : RS_OK;
}

/* row `cell` of a store of kGroupStores: put from the host (src == null: zeroed), or got (dst == null: not wanted) */
int group_row_put(rs_group* g, int store, int cell, const void* src) {
  const size_t n = kGroupStores[store].row_bytes(g);
  uint8_t* const row = (uint8_t*)g->store[store] + (size_t)cell * n;
  HIP_TRY(src ? hipMemcpy(row, src, n, hipMemcpyHostToDevice) : hipMemset(row, 0, n));
  return RS_OK;
}
int group_row_get(const rs_group* g, int store, int cell, void* dst) {
  const size_t n = kGroupStores[store].row_bytes(g);
  if (dst) HIP_TRY(hipMemcpy(dst, (const uint8_t*)g->store[store] + (size_t)cell * n, n, hipMemcpyDeviceToHost));
  return RS_OK;
}

/* a form's averages, pending bytes and the cell's last-update time; a pair of counter stores (the rbs store follows the bytes store) */
int group_get_state(const rs_group* g, int cell, int avg_store, int pend_store, double* avg, int32_t* pending_bytes, double* last_update) {
  int rc = group_row_get(g, avg_store, cell, avg);
  if (!rc) rc = group_row_get(g, pend_store, cell, pending_bytes);
  return rc ? rc : group_row_get(g, kRlast, cell, last_update);
}
int group_get_counters(const rs_group* g, int cell, int bytes_store, int64_t* cum_bytes, int64_t* cum_rbs) {
  const int rc = group_row_get(g, bytes_store, cell, cum_bytes);
  return rc ? rc : group_row_get(g, bytes_store + 1, cell, cum_rbs);
}
/* ... put: null gives zeros; with mask (the cell's existence bytes), a bearer that does not exist holds zeros */
int group_put_counters(rs_group* g, int cell, int bytes_store, const int64_t* cum_bytes, const int64_t* cum_rbs, const uint8_t* mask = nullptr) {
  const size_t n = kGroupStores[bytes_store].elems(g);
  const int64_t* src[2] = {cum_bytes, cum_rbs};
  for (int w = 0; w < 2; w++) {
    std::vector<int64_t> masked;
    if (src[w] && mask) {
      masked.assign(src[w], src[w] + n);
      for (size_t i = 0; i < n; i++)
        if (!mask[i]) masked[i] = 0;
      src[w] = masked.data();
    }
    if (const int rc = group_row_put(g, bytes_store + w, cell, src[w])) return rc;
  }
  return RS_OK;
}
/* element i of a setter's two counter arrays, [U] or [U][2] */
int group_check_counter(const int64_t* cum_bytes, const int64_t* cum_rbs, size_t i, bool two) {
  const int64_t* const v[2] = {cum_bytes, cum_rbs};
  for (int w = 0; w < 2; w++) {
    if (!v[w] || v[w][i] >= 0) continue;
    char idx[48];
    if (two) snprintf(idx, sizeof idx, "[%zu][%zu]", i / 2, i % 2);
    else snprintf(idx, sizeof idx, "[%zu]", i);
    return fail(RS_ERR_INVALID, "%s%s = %lld is negative", w ? "cum_rbs" : "cum_bytes", idx, (long long)v[w][i]);
  }
  return RS_OK;
}
/* bearer i of [U][2]: where it exists its average lies in 1..2^51 (false for NaN) */
int group_check_bearer_avg(const uint8_t* has_bearer, const double* avg, size_t i, const char* keeps) {
  if (!has_bearer[i] || (avg[i] >= 1 && avg[i] <= kBearerAvgMax)) return RS_OK;
  return fail(RS_ERR_INVALID, "avg[%zu][%zu] = %g outside 1..2^51 (an updated average is never below 1; the bound above keeps %s)", i / 2, i % 2, avg[i], keeps);
}
/* the bearer step of rs_group_set_bearers and rs_group_set_flows: the cell's row of the bearer stores and of the host's mirror.  A
 * bearer that does not exist holds zeros: the getter reports them, the kernel neither reads nor writes them. */
int group_put_bearers(rs_group* g, int cell, const uint8_t* has_bearer, const double* avg, double last_update) {
  const size_t n = 2 * (size_t)g->b->U;
  std::vector<double> a(n);
  std::vector<uint8_t> has(n);
  for (size_t i = 0; i < n; i++) {
    has[i] = has_bearer[i] ? 1 : 0;
    a[i] = has[i] ? avg[i] : 0.0;
  }
  int rc = group_row_put(g, kQavg, cell, a.data());
  if (!rc) rc = group_row_put(g, kQpend, cell, nullptr);
  if (!rc) rc = group_row_put(g, kQhas, cell, has.data());
  if (!rc) rc = group_row_put(g, kRlast, cell, &last_update);
  if (rc) return rc;
  if (g->has_bearer.empty()) g->has_bearer.assign(n * (size_t)g->n_cells, 0);
  memcpy(g->has_bearer.data() + (size_t)cell * n, has.data(), n);
  return RS_OK;
}
}  // namespace

int rs_group_set_avg(rs_group* g, int32_t cell, const double* avg, double last_update) {
  if (!g || !avg) return fail(RS_ERR_INVALID, "null argument");
  int rc = group_cell_prelude(g, cell, nullptr, false);
  if (rc) return rc;
  const size_t U = (size_t)g->b->U, nu = U * (size_t)g->n_cells;
  if (!std::isfinite(last_update)) return fail(RS_ERR_INVALID, "last_update is not finite");
  for (size_t u = 0; u < U; u++)
    if (!(avg[u] >= 1 && avg[u] <= kResidentAvgMax)) /* (false for NaN) */
      return fail(RS_ERR_INVALID, "avg[%zu] = %g outside 1..2^52 (an updated average is never below 1; the bound above keeps the FP32 filter's range)", u, avg[u]);
  if ((rc = group_cell_sync(g))) return rc;
  if (!group_alloc_family(g, kFamAverages))
    return fail(RS_ERR_HIP, "allocation of the group's resident averages failed (%zu bytes)", 24 * nu + 8 * (size_t)g->n_cells);
  GroupCellState& st = g->cells[cell];
  /* (an avg-counted cell keeps the state and its counters, as a counted cell does under rs_group_set_bearers; a cell that leaves the
   * bearer form ends its counters' term) */
  const bool keep = st.leave_for(GroupCellState::kAverages);
  if ((rc = group_row_put(g, kRavg, cell, avg)) || (rc = group_row_put(g, kRpend, cell, nullptr)) || (rc = group_row_put(g, kRlast, cell, &last_update))) return rc;
  st.enter(GroupCellState::kAverages, keep, last_update);
  return RS_OK;
}

int rs_group_get_avg(rs_group* g, int32_t cell, double* avg, int32_t* pending_bytes, double* last_update) {
  const int rc = group_cell_prelude(g, cell, &kNeedAverages, true);
  return rc ? rc : group_get_state(g, cell, kRavg, kRpend, avg, pending_bytes, last_update);
}

int rs_group_set_pending(rs_group* g, int32_t cell, const int32_t* pending_bytes) {
  if (!g || !pending_bytes) return fail(RS_ERR_INVALID, "null argument");
  int rc = group_cell_prelude(g, cell, &kNeedAverages, false);
  if (rc) return rc;
  bool all_zero = true;
  for (size_t u = 0; u < (size_t)g->b->U; u++) {
    if (pending_bytes[u] < 0 || pending_bytes[u] >= (1 << 28)) /* (times 8 it stays an int32) */
      return fail(RS_ERR_INVALID, "pending_bytes[%zu] = %d outside 0..2^28-1", u, pending_bytes[u]);
    all_zero &= pending_bytes[u] == 0;
  }
  if ((rc = group_cell_sync(g))) return rc;
  g->cells[cell].set_pending_zero(false); /* (until the copy is through) */
  if ((rc = group_row_put(g, kRpend, cell, pending_bytes))) return rc;
  g->cells[cell].set_pending_zero(all_zero);
  return RS_OK;
}

int rs_group_set_bearers(rs_group* g, int32_t cell, const uint8_t* has_bearer, const double* avg, double last_update) {
  if (!g || !has_bearer || !avg) return fail(RS_ERR_INVALID, "null argument");
  int rc = group_cell_prelude(g, cell, nullptr, false);
  if (rc) return rc;
  rs_batch* b = g->b;
  const size_t U = (size_t)b->U, nb = 2 * U * (size_t)g->n_cells;
  if (b->sched == RS_SCHED_PF)
    return fail(RS_ERR_INVALID, "resident bearers are not served for RS_SCHED_PF: it races flows, not users, and credits the whole block to the flow");
  if (b->sched == RS_SCHED_UPPERBOUND || b->sched == RS_SCHED_NVS_NONGREEDY)
    return fail(RS_ERR_INVALID, "resident bearers are not served for scheduler %d: no restatement of it with queues exists to check them against", b->sched);
  if (b->gen_exp)
    return fail(RS_ERR_INVALID, "resident bearers need exponents in {0, 1}: the general exponents' pow() of the averages is taken on the host per call");
  if (!std::isfinite(last_update)) return fail(RS_ERR_INVALID, "last_update is not finite");
  for (size_t i = 0; i < 2 * U; i++)
    if ((rc = group_check_bearer_avg(has_bearer, avg, i, "the sum of a user's two exact and inside the FP32 filter's range"))) return rc;
  if ((rc = group_cell_sync(g))) return rc;
  if (!group_alloc_family(g, kFamBearers)) return fail(RS_ERR_HIP, "allocation of the group's resident bearers failed (%zu bytes)", 25 * nb);
  GroupCellState& st = g->cells[cell];
  const bool keep = st.leave_for(GroupCellState::kBearers); /* (a cell that leaves the average form ends its per-user counters' term) */
  if ((rc = group_put_bearers(g, cell, has_bearer, avg, last_update))) return rc;
  st.enter(GroupCellState::kBearers, keep, last_update);
  return RS_OK;
}

int rs_group_get_bearers(rs_group* g, int32_t cell, double* avg, int32_t* pending_bytes, double* last_update) {
  const int rc = group_cell_prelude(g, cell, &kNeedBearers, true);
  return rc ? rc : group_get_state(g, cell, kQavg, kQpend, avg, pending_bytes, last_update);
}

namespace {
/* rs_group_set_counters and rs_group_set_avg_counters: the counters of the form the cell is in, [U][2] or [U] */
int group_set_form_counters(rs_group* g, int32_t cell, const CellNeed& need, int family, int bytes_store, const int64_t* cum_bytes, const int64_t* cum_rbs,
                            const char* alloc_failed, size_t bytes_per_user) {
  int rc = group_cell_prelude(g, cell, &need, false);
  if (rc) return rc;
  const GroupStoreRow& row = kGroupStores[bytes_store];
  for (size_t i = 0; i < row.elems(g); i++)
    if ((rc = group_check_counter(cum_bytes, cum_rbs, i, row.per_user == 2))) return rc;
  if ((rc = group_cell_sync(g))) return rc;
  if (!group_alloc_family(g, family)) return fail(RS_ERR_HIP, alloc_failed, bytes_per_user * (size_t)g->b->U * (size_t)g->n_cells);
  g->cells[cell].end_counters(); /* (until both copies are through) */
  if ((rc = group_put_counters(g, cell, bytes_store, cum_bytes, cum_rbs))) return rc;
  g->cells[cell].start_counters();
  return RS_OK;
}
}  // namespace

int rs_group_set_counters(rs_group* g, int32_t cell, const int64_t* cum_bytes, const int64_t* cum_rbs) {
  return group_set_form_counters(g, cell, kNeedBearers, kFamCounters, kCbytes, cum_bytes, cum_rbs,
                                 "allocation of the group's bearer counters failed (%zu bytes)", 40);
}

int rs_group_get_counters(rs_group* g, int32_t cell, int64_t* cum_bytes, int64_t* cum_rbs) {
  const int rc = group_cell_prelude(g, cell, &kNeedCounters, true);
  return rc ? rc : group_get_counters(g, cell, kCbytes, cum_bytes, cum_rbs);
}

int rs_group_set_avg_counters(rs_group* g, int32_t cell, const int64_t* cum_bytes, const int64_t* cum_rbs) {
  return group_set_form_counters(g, cell, kNeedAveragesForCounters, kFamAvgCounters, kAcbytes, cum_bytes, cum_rbs,
                                 "allocation of the group's per-user counters failed (%zu bytes)", 16);
}

int rs_group_get_avg_counters(rs_group* g, int32_t cell, int64_t* cum_bytes, int64_t* cum_rbs) {
  const int rc = group_cell_prelude(g, cell, &kNeedAvgCounters, true);
  return rc ? rc : group_get_counters(g, cell, kAcbytes, cum_bytes, cum_rbs);
}

/* the bearer step (rs_group_set_bearers') plus the counter step (rs_group_set_counters'), the counters masked as the averages are */
int rs_group_set_flows(rs_group* g, int32_t cell, const uint8_t* has_bearer, const double* avg, double last_update, const int64_t* cum_bytes,
                       const int64_t* cum_rbs) {
  if (!g || !has_bearer || !avg) return fail(RS_ERR_INVALID, "null argument");
  int rc = group_cell_prelude(g, cell, nullptr, false);
  if (rc) return rc;
  rs_batch* b = g->b;
  const size_t U = (size_t)b->U, nb = 2 * U * (size_t)g->n_cells;
  if (b->sched != RS_SCHED_PF)
    return fail(RS_ERR_INVALID, "resident flows are not served for scheduler %d: only RS_SCHED_PF races flows (rs_group_set_bearers serves the schedulers that race users)", b->sched);
  if (b->gen_exp)
    return fail(RS_ERR_INVALID, "resident flows need exponents in {0, 1}: the general exponents' pow() of the averages is taken on the host per call");
  if (!std::isfinite(last_update)) return fail(RS_ERR_INVALID, "last_update is not finite");
  for (size_t i = 0; i < 2 * U; i++)
    if ((rc = group_check_bearer_avg(has_bearer, avg, i, "the FP32 filter's range")) || (rc = group_check_counter(cum_bytes, cum_rbs, i, true))) return rc;
  if ((rc = group_cell_sync(g))) return rc;
  if (!group_alloc_family(g, kFamBearers) || !group_alloc_family(g, kFamCounters))
    return fail(RS_ERR_HIP, "allocation of the group's resident flows failed (%zu bytes)", 45 * nb);
  GroupCellState& st = g->cells[cell];
  st.leave_for(GroupCellState::kFlows); /* (whatever form the cell leaves, its counters' term ends) */
  if ((rc = group_put_bearers(g, cell, has_bearer, avg, last_update))) return rc;
  if ((rc = group_put_counters(g, cell, kCbytes, cum_bytes, cum_rbs, g->has_bearer.data() + (size_t)cell * 2 * U))) return rc;
  st.enter(GroupCellState::kFlows, false, last_update);
  return RS_OK;
}

int rs_group_get_flows(rs_group* g, int32_t cell, double* avg, int32_t* pending_bytes, double* last_update, int64_t* cum_bytes, int64_t* cum_rbs) {
  int rc = group_cell_prelude(g, cell, &kNeedFlows, true);
  if (!rc) rc = group_get_state(g, cell, kQavg, kQpend, avg, pending_bytes, last_update);
  return rc ? rc : group_get_counters(g, cell, kCbytes, cum_bytes, cum_rbs);
}

int rs_group_get_slice_offset(rs_group* g, int32_t cell, double* offset) {
  if (!g || !offset) return fail(RS_ERR_INVALID, "null argument");
  if (const int rc = group_cell_prelude(g, cell, nullptr, true)) return rc;
  HIP_TRY(hipMemcpy(offset, g->b->d_sstate + (size_t)cell * g->b->S, 8 * g->b->S, hipMemcpyDeviceToHost));
  return RS_OK;
}

int rs_group_set_slice_offset(rs_group* g, int32_t cell, const double* offset) {
  if (!g || !offset) return fail(RS_ERR_INVALID, "null argument");
  if (const int rc = group_cell_prelude(g, cell, nullptr, true)) return rc;
  if (const int rc = check_slice_state(g->b, offset, (size_t)cell)) return rc;
  HIP_TRY(hipMemcpy(g->b->d_sstate + (size_t)cell * g->b->S, offset, 8 * g->b->S, hipMemcpyHostToDevice));
  return RS_OK;
}

int64_t rs_group_launch_count(const rs_group* g) { return g ? g->launches : 0; }

int rs_group_image_stats(const rs_group* g, int64_t out[3]) {
  if (!g || !out) return fail(RS_ERR_INVALID, "null argument");
  out[0] = g->n_reused;
  out[1] = g->n_stored;
  out[2] = g->n_plain;
  return RS_OK;
}

const char* rs_group_kernel_name(rs_group* g) {
  if (!g) return "";
  /* (the kernel of the last call's form: the group's own build when one served it.  After a plain call: whatever serves the plain
   * calls now) */
  const int row = g->last_call_form;
  const bool jit = row == kGroupPlain ? g->pair[kGroupPlain].jit[0] != nullptr : g->last_call_jit;
  return jit ? g->kname_jit[row] : g->kname[row];
}

/* Shape specialisation of a group: rs_ctx_specialize for the group surface -- the one-TTI form compiled for the config's slices, RBGs,
 * PRBs per RBG, scheduler, workgroup size and user CAPACITY, one workgroup per call slot, in a general and a lean build.  Five pairs
 * (JitPair), each an option of its own: rs_group_specialize (entry point rs_group_kernel_jit, serves rs_group_schedule_tti),
 * rs_group_specialize_resident (rs_group_resident_kernel_jit, serves rs_group_schedule_tti_at), rs_group_specialize_queued
 * (rs_group_queued_kernel_jit, serves rs_group_schedule_tti_queued), rs_group_specialize_counted (rs_group_counted_kernel_jit, serves
 * rs_group_schedule_tti_counted) and rs_group_specialize_flows (rs_group_flows_kernel_jit, serves rs_group_schedule_tti_flows); a sixth,
 * rs_group_specialize_run (rs_group_run_kernel_jit), serves the runs of the resident form (rs_group_run_at).  Between
 * calls at any time: slice state, CQI images, per-PRB stores, resident stores, bearer stores and counters are not touched. */
namespace {
/* kind: a row of kGroupForms -- the call the pair serves */
int group_specialize_pair(rs_group* g, int kind) {
  if (!g) return fail(RS_ERR_INVALID, "null group");
  rs_batch* b = g->b;
  const GroupForm& f = kGroupForms[kind];
  JitPair& p = g->pair[f.pair];
  if (p.jit[0]) return RS_OK;
  if (p.dropped) return fail(RS_ERR_STATE, "%s", p.msg);
  if (f.lacks && !rs_group_form_serves(kind, b->sched)) return fail(RS_ERR_INVALID, "scheduler %d %s: nothing for %s to build", b->sched, f.lacks, f.entry);
  if (kind == kGroupRun && b->any_alpha)
    return fail(RS_ERR_INVALID, "a config with a customised slice (algo_alpha != 0) %s: nothing for %s to build", f.lacks, f.entry);
  HIP_TRY(hipSetDevice(b->cfg.cell.device));
  p.wanted = true; /* (from here on a failure is the pair's: status -1) */
  if (!g->d_out2) {
    const size_t out_bytes = g->out_stride * g->out_slots, chk_bytes = 2 * TwinState{g->b, nullptr, g->n_cells}.half(); /* (as many slots as d_out holds: the largest run so far) */
    if (hipMalloc(&g->d_out2, out_bytes) != hipSuccess || hipMalloc(&g->d_chk, chk_bytes) != hipSuccess) {
      (void)hipGetLastError();
      if (g->d_out2) (void)hipFree(g->d_out2);
      g->d_out2 = g->d_chk = nullptr;
      snprintf(p.msg, sizeof p.msg, "allocation of the self-check's twin blocks failed (%zu + %zu bytes)", out_bytes, chk_bytes);
      return fail(RS_ERR_HIP, "%s", p.msg);
    }
    g->h_out2.assign(out_bytes, 0);
  }
  const size_t stores = 2 * group_stores(g, f).half;
  if (stores && !g->d_stores_chk[f.pair] && hipMalloc(&g->d_stores_chk[f.pair], stores) != hipSuccess) {
    (void)hipGetLastError();
    g->d_stores_chk[f.pair] = nullptr;
    snprintf(p.msg, sizeof p.msg, "allocation of the self-check's copies of the %s failed (%zu bytes)", f.stores, stores);
    return fail(RS_ERR_HIP, "%s", p.msg);
  }
  return jit_pair_build(&p, b, 1 | rs_group_form(kind).jit_flags); /* (1: the one-TTI form, as every group build is) */
}

int group_jit_pair_status(rs_group* g, int kind, char* msg, size_t msglen) {
  if (!g) return fail(RS_ERR_INVALID, "null group");
  const GroupForm& f = kGroupForms[kind];
  return jit_pair_status(g->pair[f.pair], f.ref, msg, msglen);
}
}  // namespace

/* the entry points: one pair each */
int rs_group_specialize(rs_group* g) { return group_specialize_pair(g, kGroupPlain); }
int rs_group_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupPlain, msg, msglen); }
int rs_group_specialize_resident(rs_group* g) { return group_specialize_pair(g, kGroupResident); }
int rs_group_resident_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupResident, msg, msglen); }
int rs_group_specialize_queued(rs_group* g) { return group_specialize_pair(g, kGroupQueued); }
int rs_group_queued_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupQueued, msg, msglen); }
int rs_group_specialize_counted(rs_group* g) { return group_specialize_pair(g, kGroupCounted); }
int rs_group_counted_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupCounted, msg, msglen); }
int rs_group_specialize_flows(rs_group* g) { return group_specialize_pair(g, kGroupFlows); }
int rs_group_flows_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupFlows, msg, msglen); }
int rs_group_specialize_run(rs_group* g) { return group_specialize_pair(g, kGroupRun); }
int rs_group_run_jit_status(rs_group* g, char* msg, size_t msglen) { return group_jit_pair_status(g, kGroupRun, msg, msglen); }

/* ---- the reference's CQI trace files (include/radiosaber_hip.h) ---- */

int rs_trace_read_mapping(const char* path, int32_t* trace_of_entry, int32_t max_entries) {
  if (!path || (!trace_of_entry && max_entries > 0)) return fail(RS_ERR_INVALID, "null argument");
  std::ifstream ifs(path);
  if (!ifs) return fail(RS_ERR_INVALID, "cannot open %s", path);
  /* ref: enb-mac-entity.cc:50-53 -- `while (ifs >> uid >> tid) push_back(tid)`: the user id column is not used */
  long long uid, tid;
  int n = 0;
  while (ifs >> uid >> tid) {
    if (tid < 0 || tid > 0x7fffffff) return fail(RS_ERR_RANGE, "%s: trace id %lld out of range", path, tid);
    if (n < max_entries) trace_of_entry[n] = (int32_t)tid;
    n++;
  }
  if (n == 0) return fail(RS_ERR_INVALID, "%s: no \"<user> <trace>\" pairs", path);
  return n;
}

int rs_trace_read_ue_log(const char* path, int32_t n_rows, int32_t nb_rbs, int32_t rbg_size, uint8_t* out_rbg,
                         uint8_t* out_prb) {
  if (!path) return fail(RS_ERR_INVALID, "null argument");
  if (n_rows < 1 || nb_rbs < 1 || rbg_size < 1 || nb_rbs % rbg_size)
    return fail(RS_ERR_INVALID, "n_rows=%d nb_rbs=%d rbg_size=%d", n_rows, nb_rbs, rbg_size);
  std::ifstream ifs(path);
  if (!ifs) return fail(RS_ERR_INVALID, "cannot open %s", path);
  const int R = nb_rbs / rbg_size;
  int mixed = 0;
  int cqi = 0; /* ref: enb-mac-entity.cc:175 -- declared outside both loops: a failed extraction keeps the last value */
  std::vector<int> row(nb_rbs);
  for (int i = 0; i < n_rows; i++) {
    std::string line;
    std::getline(ifs, line);
    const char* q = line.c_str();
    bool failed = false; /* the istringstream's failbit: once set, every later `>>` leaves cqi alone */
    for (int j = 0; j < nb_rbs; j++) {
      if (!failed) {
        while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n' || *q == '\v' || *q == '\f') q++;
        if (!*q) {
          failed = true; /* end of line while skipping blanks: value untouched */
        } else {
          char* end = nullptr;
          errno = 0;
          long v = strtol(q, &end, 10);
          if (end == q) { cqi = 0; failed = true; } /* not a number: C++11 num_get stores 0 and fails */
          else {
            if (errno == ERANGE || v < 0 || v > 255)
              return fail(RS_ERR_RANGE, "%s: line %d value %d = %ld does not fit a CQI byte", path, i + 1, j + 1, v);
            cqi = (int)v;
            q = end;
          }
        }
      }
      row[j] = cqi;
    }
    for (int r = 0; r < R; r++) {
      for (int k = 1; k < rbg_size; k++)
        if (row[r * rbg_size + k] != row[r * rbg_size]) { mixed++; break; }
      if (out_rbg) out_rbg[(size_t)i * R + r] = (uint8_t)row[r * rbg_size];
    }
    if (out_prb)
      for (int j = 0; j < nb_rbs; j++) out_prb[(size_t)i * nb_rbs + j] = (uint8_t)row[j];
  }
  return mixed;
}

int rs_trace_load_dir(const char* dir, int32_t n_traces, int32_t n_rows, int32_t nb_rbs, int32_t rbg_size,
                      uint8_t* out_rbg) {
  if (!dir || !out_rbg) return fail(RS_ERR_INVALID, "null argument");
  if (n_traces < 1 || rbg_size < 1 || nb_rbs < 1 || nb_rbs % rbg_size) return fail(RS_ERR_INVALID, "bad trace shape");
  const size_t per = (size_t)n_rows * (nb_rbs / rbg_size);
  long long mixed = 0;
  for (int t = 0; t < n_traces; t++) {
    std::string f = std::string(dir) + "/ue" + std::to_string(t) + ".log"; /* ref: enb-mac-entity.cc:172 */
    int rc = rs_trace_read_ue_log(f.c_str(), n_rows, nb_rbs, rbg_size, out_rbg + (size_t)t * per, nullptr);
    if (rc < 0) return rc;
    mixed += rc;
  }
  return mixed > 0x7fffffff ? 0x7fffffff : (int)mixed;
}

int rs_lds_bytes_per_cell(int n_slices, int n_users, int n_rbgs, int sched, int threads) {
  if (n_slices < 1 || n_slices > RS_MAX_SLICES || n_users < 1 || n_users > RS_MAX_USERS || n_rbgs < 1 || n_rbgs > RS_MAX_RBGS ||
      threads < 64 || threads > 1024 || threads % 64)
    return fail(RS_ERR_INVALID, "bad shape");
  return rs_carve(n_slices, n_users, n_rbgs, sched, threads).lds_bytes;
}

/* ---- measurement helper ---- */
int rs_hbm_copy_probe(int device, uint64_t bytes, int iters, double* copy_gbs) {
  if (!copy_gbs || iters < 1 || bytes < (1u << 20) || (bytes & 15)) return fail(RS_ERR_INVALID, "bad probe arguments");
  HIP_TRY(hipSetDevice(device));
  void *src = nullptr, *dst = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = RS_OK;
  float ms = 0;
#define PROBE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { rc = fail(RS_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); goto done; } } while (0)
  PROBE_TRY(hipMalloc(&src, bytes));
  PROBE_TRY(hipMalloc(&dst, bytes));
  PROBE_TRY(hipMemset(src, 1, bytes));
  PROBE_TRY(hipEventCreate(&e0));
  PROBE_TRY(hipEventCreate(&e1));
  PROBE_TRY(rs_launch_copy_probe(src, dst, bytes, nullptr)); /* warm-up */
  *copy_gbs = 0;
  for (int trial = 0; trial < 3; trial++) { /* best of three: the rate wanders by 10-15 % between trials */
    PROBE_TRY(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; i++) PROBE_TRY(rs_launch_copy_probe(src, dst, bytes, nullptr));
    PROBE_TRY(hipEventRecord(e1, nullptr));
    PROBE_TRY(hipEventSynchronize(e1));
    PROBE_TRY(hipEventElapsedTime(&ms, e0, e1));
    const double g = 2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9; /* bytes read + bytes written */
    if (g > *copy_gbs) *copy_gbs = g;
  }
done:
#undef PROBE_TRY
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (src) (void)hipFree(src);
  if (dst) (void)hipFree(dst);
  return rc;
}

}  // extern "C"
