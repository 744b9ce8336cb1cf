/*
 * radiosaber_hip.h -- C ABI of the MI355X-native RadioSaber downlink RBG allocation path.
 *
 * Plain C, caller-owned flat buffers, int status returns, no exceptions, no torch types.
 * One context per host thread / HIP stream.  Implemented by libradiosaber_hip.so
 * (radiosaber_amd/csrc/, hand-written HIP for gfx950; there is NO CPU fallback: every entry point
 * that computes returns RS_ERR_NO_DEVICE / RS_ERR_HIP when no MI355X is usable).
 *
 * The reference (elvinlife/RadioSaber, an LTE-Sim fork) has no C ABI or plug-in loader: its
 * boundary is the C++ virtual seam
 *     PacketScheduler::Schedule() -> virtual DoSchedule() -> virtual RBsAllocation()
 *     (src/protocolStack/mac/packet-scheduler/packet-scheduler.cpp:72-90, packet-scheduler.h:133-137)
 * installed by ENodeB::SetDLScheduler (src/device/ENodeB.cpp:303-391).  Each entry point below
 * names the reference function(s) it replaces; INTEGRATION.md shows the C++ adapter class a
 * maintainer adds to the LTE-Sim tree to call them.  `ref:` paths are relative to the reference's
 * src/protocolStack/mac/packet-scheduler/ unless they start with src/.
 */
#ifndef RADIOSABER_HIP_H_
#define RADIOSABER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 11 /* 11: (additions, no layout changed) rs_batch_flow_record (flow completion times of the queue model),
                               rs_batch_bearer_log + rs_batch_run_logged_bearers (per-bearer DoStopSchedule rows),
                               rs_bearer_record / rs_batch_record_bound / rs_batch_run_records (the same lines from unlogged launches: one 32-byte record per credited bearer),
                               rs_batch_grant_record / rs_batch_grant_bound / rs_batch_run_grant_records / rs_jit_selfcheck_grant_records (a backlogged batch's app: lines from unlogged launches: one 32-byte record per grant),
                               rs_batch_set_cell_configs / rs_batch_get_cell_config / rs_batch_slice_totals / rs_jit_selfcheck_cell_configs (per-cell weights, exponents and slice sizes in one batch),
                               RS_USER_ABSENT / rs_batch_cell_users / rs_jit_selfcheck_ragged_cells (cells of different user counts in one batch: an absent-user suffix in a cell's row),
                               rs_batch_set_cell_configs_n / rs_batch_cell_slices / rs_jit_selfcheck_ragged_slices (cells of different slice counts in one batch: an absent-slice suffix),
                               rs_batch_set_cqi_epochs_device / rs_batch_write_cqi_epochs_device / rs_batch_cqi_write_status / rs_batch_debug_cqi_image (a batch's epoch grids from device memory, packed by a kernel on its stream; epochs rewritten in place: a ring),
                               rs_group_* (one TTI of several drop-in cells in one launch), rs_group_image_stats (cqi_epoch per cell of a group),
                               rs_group_specialize / rs_group_jit_status / rs_jit_selfcheck_group (a group's own self-checked builds of the one-TTI kernel),
                               rs_group_set_avg / rs_group_get_avg / rs_group_set_pending / rs_group_schedule_tti_at (a group cell's PF averages resident on the device),
                               rs_group_specialize_resident / rs_group_resident_jit_status / rs_jit_selfcheck_group_resident (a group's own builds of the resident kernel, self-checked on state),
                               rs_group_set_bearers / rs_group_get_bearers / rs_group_schedule_tti_queued (a group cell's two bearers per user resident on the device: finite queues credited there),
                               rs_group_specialize_queued / rs_group_queued_jit_status / rs_jit_selfcheck_group_queued (a group's own builds of the queued kernel, self-checked on the bearer stores),
                               rs_group_specialize_counted / rs_group_counted_jit_status / rs_jit_selfcheck_group_counted and rs_group_specialize_flows / rs_group_flows_jit_status / rs_jit_selfcheck_group_flows
                               (a group's own builds of the counted and of the flows kernel, self-checked on bearer stores, counters and sent rows),
                               rs_group_set_counters / rs_group_get_counters / rs_group_schedule_tti_counted (a bearer-resident group cell's m_cumulateBytes / m_cumulateRBs on the device, the bytes sent per bearer returned per call),
                               rs_group_set_flows / rs_group_get_flows / rs_group_schedule_tti_flows (scheduler 1's flows of a group cell resident on the device: averages, pending bytes and counters per bearer, the whole block credited to the flow),
                               rs_group_run_at + RS_GROUP_MAX_RUN (T consecutive TTIs of average-resident group cells in one launch),
                               rs_group_specialize_run / rs_group_run_jit_status / rs_jit_selfcheck_group_run (a group's own builds of the run kernel, self-checked per run on every TTI's outputs and on state),
                               rs_group_set_avg_counters / rs_group_get_avg_counters / rs_group_run_counted_at (an average-resident group cell's m_cumulateBytes / m_cumulateRBs per user on the device, advanced by runs that may return no per-TTI outputs at all),
                               rs_grant_record / rs_group_grant_bound / rs_group_run_records_at (the counted run with one compact record per grant and TTI: the reference's app: lines from a run without per-TTI outputs);
                               rs_config.link_tables (RS_LINK_*) + rs_link_tables_pinned / rs_link_tables_compare, rs_tti_in.cqi_epoch (the context keeps the
                               CQI image of an unchanged report set on the device), rs_ctx_jit_status (a specialised context checks its run-time build against the
                               built-in kernel during its first calls), rs_batch_config.selfcheck -1 / 0 / 1 with run-time builds verified by default and the
                               self-check mark in the cache file, rs_jit_compiler_identity (the compiler's full identity in the cache key);
                            10: rs_batch_debug_heap_sorts / rs_ctx_debug_heap_sorts (the sort emulation's heap-sort fallback counted per device site),
                               rs_jit_cache_stats / _file / _warm (code objects cached on disk), rs_batch_config.autotune + rs_batch_autotune_report, rs_batch_config.selfcheck, rs_batch_debug_clocks, rs_batch_checkpoint_bytes / _save / _load;
                            9: rs_create_checked / rs_batch_create_checked (RS_CREATE / RS_BATCH_CREATE: the caller's ABI version and struct size are
                            checked), rs_batch_config.cqi_epoch_wrap / queue_state_lds, threads_per_cell up to 1024 with jit, rs_jit_selfcheck_untuned, rs_batch_write_state, rs_ctx_specialize, rs_jit_selfcheck_dropin;
                            8: rs_jit_selfcheck_queue, rs_config.synthetic_exp, any integer algo_epsilon / algo_psi in drop-in contexts; 7: rs_device_source_hash; rs_schedule_tti accepts any double as avg_rate / hol_delay (exact scan outside the FP32 filter's range);
                            6: rs_tti_in.required_rbs / data_to_transmit (the gates of schedulers 7 and 1 in the drop-in mode);
                            5: per-PRB batch sources (rs_batch_upload_cqi_epochs_prb, rs_batch_set_trace_prb);
                            4: finite queues in batches (rs_batch_set_bearers, rs_batch_set_arrivals, rs_batch_read_bearer_state, rs_internet_flow_arrivals);
                            2: rs_tti_in.rand_draws, schedulers 10 / 11 / 101 / 103, rs_trace_*, rs_hbm_copy_probe, rs_lds_bytes_per_cell;
                            3: rs_get_rbg_size, rs_dl_prbs_for_bandwidth, rs_batch_read_clock, rs_batch_jit_status,
                               rs_batch_synthesize_cqi_at, rs_batch_run_logged_ex */

/* status codes */
enum {
  RS_OK = 0,
  RS_ERR_INVALID = -1,    /* bad argument / unsupported configuration (message: rs_last_error) */
  RS_ERR_NO_DEVICE = -2,  /* no usable HIP device */
  RS_ERR_HIP = -3,        /* a HIP runtime call failed */
  RS_ERR_STATE = -4,      /* call order (e.g. run before a CQI source is set) */
  RS_ERR_RANGE = -5       /* device-side check failed (trace row out of range, ...) */
};

/* scheduler selection, numbered like the reference CLI `sched` argument
 * (ref: src/scenarios/single-cell-with-interference.h:94-123, src/device/ENodeB.h:66-81) */
enum {
  RS_SCHED_PF = 1,         /* DL_PF_PacketScheduler -> DownlinkPacketScheduler::RBsAllocation
                              (ref: downlink-packet-scheduler.cpp:179-331, dl-pf-packet-scheduler.cpp:128-140) */
  RS_SCHED_NVS = 7,        /* DownlinkNVSScheduler (ref: downlink-nvs-scheduler.cpp:94-142,275-358) */
  RS_SCHED_SEQUENTIAL = 8, /* DownlinkTransportScheduler + GreedyByRow (ref: downlink-transport-scheduler.cpp:249-272) */
  RS_SCHED_MAXCELL = 9,    /* DownlinkTransportScheduler + MaximizeCell = RadioSaber (ref: :351-376) */
  RS_SCHED_NVS_NONGREEDY = 11, /* DownlinkNVSScheduler with is_nongreedy_ (the CLI's scheduler 11): RBsAllocationNonGreedyPF +
                              AssignRBsGivenMCS (ref: downlink-nvs-scheduler.cpp:405-528), 300 sampled CQI-index vectors per TTI */
  RS_SCHED_UPPERBOUND = 10, /* DownlinkTransportScheduler + UpperBound (ref: :223-246, apply step :603-616): every slice takes
                              its own best quota RBGs whatever the others take -- an upper bound, not an allocation: several
                              UEs may hold one RBG.  rbg_to_user then reports the UE of the lowest-numbered slice holding
                              the RBG; user_nprb / user_tbs_bits / ... are complete and rs_tti_out.upper_rbg / upper_user list
                              every slice's RBGs in push order.  Needs n_rbgs*n_slices <= 2048. */
  RS_SCHED_SUBOPT = 101,   /* DownlinkTransportScheduler + SubOpt (ref: :274-349; inter_sched_ = 1, which no CLI number selects):
                            * best slice per RBG, then least-loss moves from slices above to slices below their quota, ties
                            * in the order libstdc++'s unordered_map yields the slices */
  RS_SCHED_VOGEL = 103     /* DownlinkTransportScheduler + VogelApproximate (ref: :378-451; inter_sched_ = 3, which no CLI
                              scheduler number of the reference selects -- ENodeB::DLScheduler_VOGEL exists, ENodeB.cpp:375) */
};

#define RS_MAX_SLICES 64
#define RS_MAX_RBGS 64
#define RS_MAX_USERS 1024

/* What the reference scheduler constructors parse out of the JSON config
 * (ref: downlink-transport-scheduler.cpp:55-97, downlink-nvs-scheduler.cpp:44-86,
 *  dl-pf-packet-scheduler.cpp:40-58) plus the cell's PRB grid
 * (ref: RBsAllocation :457-461 nb_rbs/rbg_size; src/utility/eesm-effective-sinr.h:82-103). */
typedef struct rs_config {
  int32_t n_slices;             /* S = ues_per_slice.size()                      (1..64)   */
  int32_t n_users;              /* U = sum(ues_per_slice); user ids are 0..U-1   (1..1024) */
  int32_t n_rbgs;               /* R = nb_rbs / rbg_size                         (1..64)   */
  int32_t rbg_size;             /* PRBs per RBG = get_rbg_size(nb_rbs)           (1..8)    */
  int32_t sched;                /* RS_SCHED_*                                               */
  int32_t device;               /* HIP device ordinal                                       */
  const double* slice_weight;   /* [S] "weight"                                             */
  const int32_t* algo_alpha;    /* [S] 0, or 1 = customised slice (ref: :694-711): the queue state comes in through
                                   rs_tti_in.hol_delay / prio_has_data (drop-in mode) or from the batch's own queue model
                                   (rs_batch_set_bearers / rs_batch_set_arrivals)                       */
  const int32_t* algo_beta;     /* [S] 0 or 1: with alpha = 1, multiply the metric by the HoL delay  */
  const int32_t* algo_epsilon;  /* [S] exponent of the rate in pow(se_kbps, epsilon) / pow(avg_kbps, psi) (ref: downlink-transport-
                                 * scheduler.cpp:690-693).  rs_create (drop-in): any integer in -64..64 -- the host's libm raises
                                 * the powers (16 numerators per slice once, every user's denominator per call), the device divides
                                 * and compares exactly.  rs_batch_create: 0 or 1 only (pow(x,0)=1, pow(x,1)=x are exact; the PF
                                 * averages live on the device, which has no pow())                                        */
  const int32_t* algo_psi;      /* [S] exponent of the average, same rule                                                  */
  const int32_t* user_to_slice; /* [U] non-decreasing (run-length expansion of ues_per_slice) */
  void* stream;                 /* hipStream_t to launch on, NULL = a stream owned by the context */
  int32_t synthetic_exp;        /* 0 (as shipped), or 1 = the reference built with FIRST_SYNTHETIC_EXP / SECOND_SYNTHETIC_EXP
                                 * (CONFIG/global_config:57-58): schedulers 7, 8, 9, 10, 101, 103 size a transport block PRB by
                                 * PRB, each with the MCS of its own CQI (downlink-transport-scheduler.cpp:653-659,
                                 * downlink-nvs-scheduler.cpp:336-342; the PDCCH record keeps the EESM MCS); schedulers 1 and 11 have
                                 * no such branch and ignore it.  (ABI 8)                                                      */
  int32_t link_tables;          /* RS_LINK_*: where the EESM constants E[c] / X[k] come from (see rs_link_tables).  (ABI 11)    */
} rs_config;

/* The EESM constants are transcendental: the reference evaluates exp / pow / log / log10 with the libm of the machine it was built on
 * (src/utility/eesm-effective-sinr.h:33-46, src/protocolStack/mac/AMCModule.cpp:253-261), and a final CQI can differ by one between two
 * libms that round one of them differently.
 *   RS_LINK_PINNED_GLIBC_2_35  the values glibc 2.35 (x86-64) gives -- the libm behind every fixture of this repository (SURVEY.md
 *                              Appendix A, tests/golden/appendix_a.json) -- compiled into the library as data: results do not depend
 *                              on the machine that runs the GPU
 *   RS_LINK_HOST_LIBM          this host's libm, evaluated at create time exactly as the reference evaluates them: what a drop-in needs
 *                              beside a reference built on the same machine
 *   RS_LINK_DEFAULT (0)        batches: pinned; drop-in contexts (rs_create): host libm -- and when the two sets differ on this host,
 *                              rs_create still succeeds and rs_last_error() carries one line that says where (empty otherwise) */
enum { RS_LINK_DEFAULT = 0, RS_LINK_HOST_LIBM = 1, RS_LINK_PINNED_GLIBC_2_35 = 2 };

const char* rs_last_error(void);   /* thread-local message of the last failing call */
/* The structs of this header grow at their ends from one ABI version to the next, and the plain create functions below read them
 * with THIS library's layout.  A caller that may meet a library of another version either compares rs_abi_version() with the
 * RS_ABI_VERSION it was compiled with before creating anything, or creates through RS_CREATE / RS_BATCH_CREATE
 * (rs_create_checked / rs_batch_create_checked), which pass the caller's version and struct size and are refused with
 * RS_ERR_INVALID on any mismatch -- nothing is inferred from field values. */
int rs_abi_version(void);
int rs_device_count(void);         /* number of HIP devices (0 when none)           */

/* Link-adaptation constants the device uses, computed by the HOST libm exactly as the reference
 * evaluates them (ref: src/utility/eesm-effective-sinr.h:33-46, src/protocolStack/mac/AMCModule.cpp:253-261,320-327):
 *   eff[c]  = (TBS(1 PRB, mcs(c)) / 0.001) / 180000.            c = 1..15  (eff[0] = 0)
 *   kbps[c] = eff[c] * 180000 / 1000
 *   E[c]    = exp(-pow(10, SINRForCQIIndex[c-1] / 10))
 *   X[k]    = max{ x : 10*log10(-1*log(x)) >= SINRForCQIIndex[k] }   k = 1..13
 * final CQI of an allocation = 1 + #{k : x <= X[k]}, x = (sum of E over its PRBs) / nPRB; x == 0 -> 15.
 * Needs no GPU.  Returns RS_ERR_INVALID if the host libm is not monotone around a threshold. */
int rs_link_tables(double eff[16], double kbps[16], double eesm_e[16], double eesm_x[16]);
/* the same with E[c] / X[k] from the pinned glibc-2.35 set (eff / kbps are IEEE divisions of table integers: the same on any host) */
int rs_link_tables_pinned(double eff[16], double kbps[16], double eesm_e[16], double eesm_x[16]);
/* this host's libm against the pinned set: the number of E / X entries that differ (0: they agree), msg receives "E[c] host ... pinned
 * ..." for each; RS_ERR_INVALID when the host's libm is not monotone around a threshold.  Needs no GPU. */
int rs_link_tables_compare(char* msg, size_t msglen);

/* replaces get_rbg_size() (ref: src/utility/eesm-effective-sinr.h:82-103): PRBs per RBG of a cell with nb_rbs PRBs
 * (<= 10: 1, <= 26: 2, <= 63: 3, <= 110: 4, <= 512: 8).  Above 512 the reference throws std::runtime_error: RS_ERR_INVALID. */
int rs_get_rbg_size(int nb_rbs);
/* replaces BandwidthManager's GetDlSubChannels().size() (ref: src/core/spectrum/bandwidth-manager.cpp:30-38, 52-108):
 * 1.4 -> 6, 3 -> 15, 5 -> 25, 10 -> 50, 15 -> 75, 20 -> 100, 100 -> 512 PRBs, anything else 25 as the reference's else-branch. */
int rs_dl_prbs_for_bandwidth(double bw_mhz);

/* ------------------------------------------------------------------------------------------
 * Drop-in mode: one RBsAllocation() call.
 * ------------------------------------------------------------------------------------------ */
typedef struct rs_ctx rs_ctx;

/* replaces the scheduler constructor + ENodeB::SetDLScheduler (ref: src/device/ENodeB.cpp:303-391) */
rs_ctx* rs_create(const rs_config* cfg);
rs_ctx* rs_create_checked(const rs_config* cfg, int abi_version, size_t cfg_size);
#define RS_CREATE(cfg) rs_create_checked((cfg), RS_ABI_VERSION, sizeof(rs_config))
void rs_destroy(rs_ctx* ctx);

/* What RBsAllocation() sees on entry (ref: GetUsersToSchedule(): packet-scheduler.h:88-123):
 * the users with queued data, in first-seen (= ascending user id) order. */
typedef struct rs_tti_in {
  int32_t n_users;          /* users to schedule this TTI (<= cfg.n_users)                          */
  const int32_t* user_id;   /* [n] ascending user ids; NULL = 0..n-1                                */
  const uint8_t* cqi;       /* [n][R] CQI (1..15) of PRB rbg*rbg_size = GetCqiFeedbacks().at(rbg*rbg_size);
                               the whole RBG carries that CQI (true for every shipped trace);
                               see cqi_prb for the general case                                     */
  const double* avg_rate;   /* [n] GetAverageTransmissionRate() of the user's bearer; the kernel forms the reference's
                             *     `averageRate = 1 + avg` (:681-686).  A user holding two bearers (MAX_BEARERS = 2): pass
                             *     ((1 + a0) + a1) - 1, which is exact for averages >= 1 and reproduces the reference's
                             *     summation order bit for bit (the C++ adapter does this) */
  int32_t rand0, rand1;     /* the two rand() values RBsAllocation draws (ref: :490, :511);
                               ignored by RS_SCHED_PF / RS_SCHED_NVS                                */
  const uint8_t* cqi_prb;   /* optional [n][R*rbg_size]: the full per-PRB GetCqiFeedbacks() vectors.  When
                               non-NULL `cqi` is ignored (the metric reads PRB rbg*rbg_size, ref: :536) and link
                               adaptation reads every allocated PRB (ref: :643-646), so CQIs may differ inside
                               an RBG as the simulated channel's reports do                           */
  /* customised slices (algo_alpha = 1), ref: downlink-transport-scheduler.cpp:694-711,
   * downlink-nvs-scheduler.cpp:375-387; both may be NULL when every slice has algo_alpha = 0 */
  const double* hol_delay;       /* [n] GetHeadOfLinePacketDelay() of the user's slice-priority bearer     */
  const uint8_t* prio_has_data;  /* [n] m_dataToTransmit[slice_priority_[slice]] != 0; NULL = all 1        */
  const int32_t* rand_draws;     /* RS_SCHED_NVS_NONGREEDY only: the 300 * n values rand() returns to
                                    RBsAllocationNonGreedyPF, in draw order (sample-major, user-minor;
                                    downlink-nvs-scheduler.cpp:431-441); NULL for every other scheduler     */
  /* finite queues: the two gates that never bind for InfiniteBuffer flows.  NULL = backlogged (no gate). */
  const int32_t* required_rbs;     /* RS_SCHED_NVS, [n]: UserToSchedule::m_requiredRBs in PRBs; a user competes for an RBG
                                      only while its allocated PRBs are below it (downlink-nvs-scheduler.cpp:299-300)       */
  const int32_t* data_to_transmit; /* RS_SCHED_PF, [n] bytes: FlowToSchedule::GetDataToTransmit(); a flow leaves the TTI's
                                      competition once the transport block of its PRBs so far carries data * 8 bits
                                      (downlink-packet-scheduler.cpp:253-265)                                               */
  uint64_t cqi_epoch;       /* 0: no promise -- the CQI block is validated, copied and read on every call.  Non-zero: the caller's
                               version number of `cqi` (or `cqi_prb`): it changes the number whenever ANY report changed.  The reference
                               refreshes a UE's CQI every 40 TTIs (src/protocolStack/mac/enb-mac-entity.cc:38 CQI_INTERVAL,
                               src/device/CqiManager/cqi-manager.cpp:115), so 39 calls of 40 see the grid of the call before.  A call
                               whose cqi_epoch, n_users and user_id list equal the previous call's does not touch the caller's block:
                               the kernel reads the image the context -- or, in a group call, the CELL -- kept on the device (the grid in the
                               layout of its LDS, HBM-resident) instead of n * R bytes over the host link, and the host skips the range
                               check and the copy.  (ABI 11) */
} rs_tti_in;

/* What RBsAllocation() leaves behind (ref: :589-620 allocation lists + slice_rbs_offset_,
 * :630-674 UpdateAllocatedBits / PDCCH records). All arrays caller-allocated. */
typedef struct rs_tti_out {
  int32_t* target_rbs;      /* [S] slice_target_rbs   (0 for PF/NVS)                      */
  int32_t* quota_rbgs;      /* [S] slice_quota_rbgs   (0 for PF/NVS)                      */
  int32_t* rbg_to_user;     /* [R] user id owning RBG r (its PRBs r*rbg_size..+rbg_size-1), -1 = none */
  int32_t* user_nprb;       /* [n] GetListOfAllocatedRBs()->size()                        */
  int32_t* user_final_cqi;  /* [n] GetCQIFromSinr(GetEesmEffectiveSinr(..)), 0 = not scheduled */
  int32_t* user_mcs;        /* [n] mcs of the PDCCH records                               */
  int32_t* user_tbs_bits;   /* [n] UpdateAllocatedBits() argument                         */
  /* RS_SCHED_UPPERBOUND only, both optional (NULL = not wanted): what the apply step :603-616 walks -- per slice the RBGs it
   * took in push order and the user id each one went to (user_index[rbg][slice]); [S][n_rbgs], -1 padded */
  int32_t* upper_rbg;
  int32_t* upper_user;
} rs_tti_out;

/* replaces DownlinkTransportScheduler::RBsAllocation (ref: downlink-transport-scheduler.cpp:453-675),
 * DownlinkPacketScheduler::RBsAllocation (ref: downlink-packet-scheduler.cpp:179-331) and
 * DownlinkNVSScheduler::RBsAllocation (ref: downlink-nvs-scheduler.cpp:275-358; pass the users of the
 * slice SelectSliceToServe chose).  The context carries slice_rbs_offset_ between calls -- and nothing else of the simulator's state:
 * PF averages, pending grants, cumulative counters, the clock and the rand() stream stay the caller's (DoSchedule / DoStopSchedule keep
 * them in the reference too); with rs_tti_in.cqi_epoch it also keeps an image of the last CQI grid on the device.
 * One context per host thread.  Many contexts in one process: export GPU_MAX_HW_QUEUES >= their number (up to 16) before the process
 * starts -- the HIP runtime maps a process's streams onto 4 hardware queues by default, and one-TTI kernels of contexts that share a
 * queue run one after the other; rs_create says so through rs_last_error() when it happens (profiles/r06_dropin_concurrency.md). */
int rs_schedule_tti(rs_ctx* ctx, const rs_tti_in* in, rs_tti_out* out);
/* Optional, once after rs_create: compile this context's own build of the one-TTI kernel (hiprtc, ~2 s per shape and process,
 * cached) -- slices, RBGs, PRBs per RBG, scheduler and the user capacity as compile-time constants, the users of a call still a
 * launch argument.  Results are identical; a call gets shorter.  Two builds (~2 s each): the general one and a lean
 * one that serves the plain call -- per-RBG CQI, no customised slices, no gates, exponents in {0, 1}, every input an ordinary
 * FP32 number -- with those per-call options as constants (RS_JIT_LEAN=0: the general one only).  RS_OK, or RS_ERR_HIP with the
 * context left on the kernels built into the library.  The C++ adapter calls it from its constructor.  (ABI 9) */
int rs_ctx_specialize(rs_ctx* ctx);
/* A specialised context does not trust its run-time build blindly (round 6): unless the code object came from the disk cache with the
 * self-check mark of an earlier process, the first RS_DROPIN_SELFCHECK_CALLS (default 8) calls each of its two builds serves run on the
 * kernel built into the library AS WELL, from the same slice state, and every field of rs_tti_out plus the slice state left behind is
 * compared.  Agreement for all of them leaves the mark in the cache file; one difference drops the build for good -- that call and all
 * later ones are served by the built-in kernel, the call still returns RS_OK with the built-in kernel's (correct) results, and
 * rs_last_error() / rs_ctx_jit_status say which field of which user differed.  RS_JIT_SELFCHECK=0 switches the check off, =2 checks
 * marked builds too.
 * rs_ctx_jit_status: 1 = the specialised kernels serve the calls (msg: empty, or how many checked calls agreed), 0 = rs_ctx_specialize
 * was not called, -1 = it failed to build, -2 = a build was dropped by the check (msg says what differed). */
int rs_ctx_jit_status(rs_ctx* ctx, char* msg, size_t msglen);
/* build check without a GPU: does that kernel compile for a context of this shape? (code size or a negative value) */
int rs_jit_selfcheck_dropin(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);
/* slice_rbs_offset_ accessors (ref: downlink-transport-scheduler.h:38)
 * THE DOMAIN OF SLICE STATE SET FROM OUTSIDE (rs_set_slice_offset, rs_group_set_slice_offset, the slice_state of
 * rs_batch_write_state).  A value outside it is RS_ERR_INVALID with a message, and the state stays as it was:
 *   - every scheduler: finite values;
 *   - RS_SCHED_SEQUENTIAL / MAXCELL / SUBOPT / VOGEL / UPPERBOUND (slice_rbs_offset_): per cell, with nb_rbs = n_rbgs * rbg_size,
 *       5 * nb_rbs * (1 + sum |slice_weight|) + sum |offset|  <  2^15 = 32768.
 *     Two limits stand behind it.  Every surface hands target_rbs and quota_rbgs out as int16 (rs_tti_out of a context or a group
 *     as well as rs_batch_log), so a target of magnitude 2^15 would come back wrong; under the rule the targets stay inside +-2^15 in
 *     the call that reads the offsets and in the one after it, and from there the offsets move toward the weights' shares.  And the
 *     quota step divides extra_rbs, the targets and extra_rbgs by a float division with a fix-up, which equals C's '/' for
 *     numerators of magnitude below 2^25 + 2 (33554432 + 2; 1 <= divisor <= 64; measured in tests/test_quota_edge_inputs.py) and
 *     not beyond: a single offset is thus a factor of a thousand inside that bound minus nb_rbs.
 *   - RS_SCHED_NVS / NVS_NONGREEDY (slice_ewma_time_): values >= 0.  The reference's scan never picks a slice with a negative score,
 *     the kernel orders scores as integer pairs, which is the order of the doubles for non-negative ones only. */
int rs_get_slice_offset(rs_ctx* ctx, double* offset /* [S] */);
int rs_set_slice_offset(rs_ctx* ctx, const double* offset /* [S] */);

/* ------------------------------------------------------------------------------------------
 * Drop-in mode for a host that owns several cells: one TTI of up to n_cells cells in ONE kernel launch
 * (one workgroup per cell) instead of one launch, one wait and one unpack per cell.  (ABI 11 addition, no layout changed.)
 *
 * Cell k of a group behaves exactly like an rs_ctx of its own, created from the same rs_config and fed the same sequence of
 * rs_tti_in: every rs_tti_out field, the upper_* lists of RS_SCHED_UPPERBOUND and the slice state it carries to its next call are
 * identical.  Cells are independent of each other; in one call they may differ in n_users / user_id, rand0 / rand1 and every input
 * value.  A call that names a subset of the cells leaves the others' state untouched.
 *
 * Rules (each one is RS_ERR_INVALID with a message in rs_last_error(); a rejected call launches nothing and moves no cell's state):
 *   - 1 <= n_cells <= RS_GROUP_MAX_CELLS (a sanity bound, not a tuned number); 1 <= n <= n_cells per call.
 *   - cell_ids are distinct and in 0..n_cells-1 (NULL: cells 0..n-1).
 *   - The PRESENCE of optional inputs is the same for every cell of one call: all cells give cqi_prb or none does (then all give cqi);
 *     all or none give hol_delay; all or none give prio_has_data; all or none give the scheduler's gate (required_rbs for
 *     RS_SCHED_NVS, data_to_transmit for RS_SCHED_PF); all or none ask for the upper_* outputs.  These are per-launch switches of
 *     the kernel.
 *   - The exact FP64 scan that rs_schedule_tti uses when an average or a HoL delay lies outside the FP32 filter's safe range is
 *     decided per call: if any cell of the call needs it, every cell of the call uses it (same results: DESIGN.md 2.6).
 *   - cqi_epoch is honoured per CELL and per call, as by an rs_ctx of the cell's own: every cell keeps the CQI image of its last call
 *     under a non-zero number on the device (and a device copy of the per-PRB block when that call gave cqi_prb).  A cell whose call
 *     carries the number, n_users, user_id list (or both NULL) and kind of report (cqi / cqi_prb) of its image is served from it: the
 *     caller's block is neither range-checked, copied nor read.  Any other non-zero number: the block is read and the image replaced.
 *     0: the block is read and the cell's image ends.  The image belongs to the cell, not to the call slot: cell_ids may
 *     map cells to other slots on every call, cells that a call does not name keep theirs, and the cells of one call may differ in
 *     what they do.  A rejected call leaves every image as it was; a call that fails with RS_ERR_HIP ends the images of the cells it
 *     named.  RS_GROUP_IMAGE=0 in the environment of rs_group_create: every cqi_epoch counts as 0 (every block read on every call).
 *     If the per-PRB store cannot be allocated (first cqi_prb call under a number), that call still returns RS_OK, says so once
 *     through rs_last_error(), and the group serves cqi_prb calls as if cqi_epoch were 0 from then on.
 *   - Every scheduler rs_create accepts except RS_SCHED_NVS_NONGREEDY; general integer exponents and synthetic_exp are supported
 *     (they belong to the config, so they are the same for the whole group).
 *   - A group starts on the kernels built into the library and may get builds of its own (rs_group_specialize below).  The built-in
 *     kernels also run beside those builds' checked calls, so a shape they cannot run (more than 512 threads per cell) is rejected
 *     by rs_group_create either way.
 * One host thread per group at a time; different groups may run on different threads.
 * ------------------------------------------------------------------------------------------ */
#define RS_GROUP_MAX_CELLS 1024
typedef struct rs_group rs_group;
rs_group* rs_group_create(const rs_config* cfg, int32_t n_cells);
rs_group* rs_group_create_checked(const rs_config* cfg, int32_t n_cells, int abi_version, size_t cfg_size);
#define RS_GROUP_CREATE(cfg, n_cells) rs_group_create_checked((cfg), (n_cells), RS_ABI_VERSION, sizeof(rs_config))
void rs_group_destroy(rs_group* g);
/* in[k] / out[k] belong to cell cell_ids[k] (NULL: cell k), k = 0..n-1; every cell is validated before anything is launched */
int rs_group_schedule_tti(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, rs_tti_out* out /* [n] */);
/* slice_rbs_offset_ of one cell (RS_SCHED_NVS: its slice EWMAs), as rs_get_slice_offset / rs_set_slice_offset; the setter
 * accepts the domain stated at rs_set_slice_offset and nothing else */
int rs_group_get_slice_offset(rs_group* g, int32_t cell, double* offset /* [S] */);
int rs_group_set_slice_offset(rs_group* g, int32_t cell, const double* offset /* [S] */);
/* scheduling kernels launched so far: one per successful rs_group_schedule_tti, none for a rejected one (tests, tools) */
int64_t rs_group_launch_count(const rs_group* g);
/* cell-TTIs of the successful calls so far: out[0] served from the cell's image (the caller's block not read), out[1] that read the
 * block and stored an image (non-zero cqi_epoch, no match), out[2] without a promise (cqi_epoch 0, or RS_GROUP_IMAGE=0) */
int rs_group_image_stats(const rs_group* g, int64_t out[3]);
/* "rs_group_kernel_jit" while the group's own builds serve its calls; the built-in instantiation's name before rs_group_specialize and
 * after a build was dropped.  While the last call was a resident one: "rs_group_resident_kernel_jit" if the group's resident builds
 * served it (rs_group_specialize_resident), else the built-in "rs_group_resident_kernel<sched, ept>".  While it was a queued one:
 * "rs_group_queued_kernel_jit" if the group's queued builds served it (rs_group_specialize_queued), else the built-in
 * "rs_group_queued_kernel<sched, ept>".  While it was a counted one (rs_group_schedule_tti_counted): "rs_group_counted_kernel_jit" if
 * the group's counted builds served it (rs_group_specialize_counted), else the built-in "rs_group_counted_kernel<sched, ept>".  While
 * it was a flows one (rs_group_schedule_tti_flows): "rs_group_flows_kernel_jit" if the group's flows builds served it
 * (rs_group_specialize_flows), else the built-in "rs_group_flows_kernel<1, 0>".  While it was a run (rs_group_run_at):
 * "rs_group_run_kernel_jit" if the group's run builds served it (rs_group_specialize_run), else the built-in
 * "rs_group_run_kernel<sched, ept>". */
const char* rs_group_kernel_name(rs_group* g);
/* Optional, at any time between two calls: rs_ctx_specialize for a group -- the one-TTI kernel compiled for the config's slices, RBGs,
 * PRBs per RBG, scheduler, workgroup size and user capacity (hiprtc, ~2 s per build and process, cached on disk apart from the
 * contexts' builds), one workgroup per call slot.  Two builds: the general one, and a lean one that rs_group_schedule_tti picks when
 * the call is plain for EVERY cell (per-RBG CQI, no customised slices, no gate, exponents in {0, 1}, every input an ordinary FP32
 * number, no upper_* lists; RS_JIT_LEAN=0: the general one only).  Results are identical.  Slice state, CQI images and per-PRB stores
 * are not touched: a call right after it is served from the images the built-in kernels stored.  RS_OK; RS_ERR_HIP with the group left
 * on the built-in kernels; a second call is a no-op; RS_ERR_STATE (with the reason) once a build was dropped.
 * The builds are checked as a context's are (rs_ctx_jit_status above, same switches): a build without the self-check mark serves its
 * first RS_DROPIN_SELFCHECK_CALLS (default 8) calls beside the built-in group kernel -- same slots, same slice state, completion by
 * the stream -- and every named cell's rs_tti_out fields, upper_* lists and slice state are compared bit for bit.  Agreement on all of
 * them leaves the mark in the cache file.  One difference drops BOTH builds and unlinks their cache files: that call returns the
 * built-in kernel's results and state with RS_OK, later calls run the built-in kernels, and rs_last_error() / rs_group_jit_status name
 * the cell, the field and the index ("cell 3: user_tbs_bits[3] = 2224, the built-in kernel's 2216").  rs_group_launch_count counts a
 * checked call once.  RS_JIT_SELFCHECK=0 never checks, =2 checks marked builds too. */
int rs_group_specialize(rs_group* g);
/* 1 = the group's own builds serve the calls (msg: per build, how it earned its trust), 0 = rs_group_specialize was not called,
 * -1 = it failed to build, -2 = the builds were dropped by the check (msg says what differed) */
int rs_group_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean build of a group of this shape compile?  (the larger code size, or a
 * negative value with the compiler's log in err) */
int rs_jit_selfcheck_group(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* Resident averages (ABI 11 addition, no layout changed): a cell of a group may keep what RadioBearer keeps for the PF metric on the
 * device -- every user's average rate (m_averageTransmissionRate), the bytes granted since the last update (m_transmittedData) and
 * the time of that update (m_lastUpdate) -- next to its slice state.  A call through rs_group_schedule_tti_at then does
 * DoSchedule()'s first line, UpdateAverageTransmissionRate() (ref: src/flows/radio-bearer.cpp:139-164), on the device, schedules the
 * TTI on the result and records the TTI's grants for the next update; once cqi_epoch matches, such a call sends only the slot header
 * and the slice ids of the cell.  Per resident slot, in this order:
 *   1. now == last_update: nothing is updated (the reference's early return).  Otherwise, for EVERY user id u of the config, named by
 *      the call or not:  rate = (double)(pending[u] * 8) / (now - last_update);  a = ((1 - 0.02) * a) + (0.02 * rate);
 *      if (a < 1) a = 1;  pending[u] = 0;  -- then last_update = now.  (The batch kernels' operations, in their order, unfused.)
 *   2. The call's users (user_id[i], or 0..n-1) are scheduled as by rs_group_schedule_tti with avg_rate[i] = avg[user_id[i]].
 *   3. Each served user's grant, min(tbs_bits / 8, 100000000) bytes (the InfiniteBuffer's dataToTransmit), is added to pending[user_id[i]].
 * A cell of this form is one InfiniteBuffer bearer per user.  Users that hold two bearers, and bearers with finite queues -- where
 * DoStopSchedule credits min(grant, dataToTransmit) (downlink-transport-scheduler.cpp:177-188) and not the transport block -- are
 * served by the second resident form, resident bearers (rs_group_set_bearers / rs_group_schedule_tti_queued below).
 * (rs_group_set_pending overwrites the pending bytes of this form: a synchronising copy, outside the fast path.)
 * rs_group_schedule_tti is unchanged: it still needs avg_rate, and on a resident cell it uses the caller's averages and neither reads
 * nor writes the resident state.
 * Resident calls run the resident kernel built into the library ("rs_group_resident_kernel<sched, ept>" in rs_group_kernel_name while
 * a resident call is the last one served), after rs_group_specialize too: that call specialises the plain call only.  Run-time builds of
 * the resident form are an option of their own, rs_group_specialize_resident below. */
/* Makes `cell` resident (again, at any time between two calls): avg[cfg.n_users] by user id, zero pending bytes, last_update =
 * m_lastUpdate.  RS_ERR_INVALID for an average that is not in 1..2^52 (an updated average is never below 1; the upper bound keeps
 * the metric scan's FP32 filter in its range without the host seeing the values -- DESIGN.md 7d) or a last_update that is not finite. */
int rs_group_set_avg(rs_group* g, int32_t cell, const double* avg /* [cfg.n_users], by user id */, double last_update);
/* The resident state as it is after the last call (a synchronising copy for tests, checkpoints and logs; not part of a TTI).  Each
 * output may be NULL.  RS_ERR_STATE: the cell is not resident. */
int rs_group_get_avg(rs_group* g, int32_t cell, double* avg /* [U] or NULL */, int32_t* pending_bytes /* [U] or NULL */, double* last_update /* or NULL */);
/* Overwrites the bytes that wait for the next update (0 <= bytes < 2^28: times 8 an int32); a synchronising copy, outside the fast path */
int rs_group_set_pending(rs_group* g, int32_t cell, const int32_t* pending_bytes /* [U] */);
/* rs_group_schedule_tti for resident cells; now[k] is the simulator clock of cell cell_ids[k]'s TTI.  Every rule of a group call
 * holds (uniform presence of optional inputs, cqi_epoch per cell, subsets and permutations through cell_ids; a rejected call
 * launches nothing and moves nothing; rs_group_launch_count and rs_group_image_stats count these calls like any others), and
 *   - in[k].avg_rate is NULL for every k (RS_ERR_INVALID);
 *   - every named cell is resident (RS_ERR_STATE, the message names the cell);
 *   - now[k] is finite, not before the cell's last_update, and now[k] - last_update is 0 or at least 2^-20 s (RS_ERR_INVALID); a
 *     shorter interval is accepted only while no byte can be pending (no resident call since rs_group_set_avg or an all-zero
 *     rs_group_set_pending), as for a first TTI at 0.1 + 7e-17 s behind an m_lastUpdate of 0.1;
 *   - the config's exponents are in {0, 1} (RS_ERR_INVALID: the general exponents' pow() of the averages is taken on the host).
 * hol_delay outside the FP32 filter's range still switches the call to the exact scan.  A call that fails with RS_ERR_HIP leaves the
 * cells it named not resident. */
int rs_group_schedule_tti_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, rs_tti_out* out /* [n] */, const double* now /* [n] */);
/* Optional, at any time between two calls, with or without rs_group_specialize: rs_group_specialize for the RESIDENT call -- the resident
 * kernel compiled for the group's shape (entry point rs_group_resident_kernel_jit, cache files of its own), a general and a lean build;
 * rs_group_schedule_tti_at picks the lean one under the plain call's per-launch condition (no per-PRB reports, no customised slices, no
 * gate, no exact scan, no upper_* lists, no synthetic-experiment blocks; RS_JIT_LEAN=0: the general build only).  rs_group_schedule_tti
 * is not affected.  Cell state, CQI images and the resident stores are not touched.  RS_OK; a second call is a no-op; RS_ERR_HIP if a
 * build fails, the group left on the built-in resident kernel; RS_ERR_STATE (with the reason) once the resident builds were dropped.
 * The check follows rs_group_specialize's policy and switches (RS_DROPIN_SELFCHECK_CALLS, RS_JIT_SELFCHECK, the mark in the cache file)
 * and compares STATE as well: before a checked call the slice state, the cell scalars and the resident stores are kept; the built-in
 * resident kernel runs into twin output slots; what it left is kept and the earlier state put back; then the group's build runs, with
 * completion by the stream.  For every named cell the rs_tti_out fields (upper_* lists if asked), the slice state, the averages of
 * EVERY user id of the config, the pending bytes and last_update must agree bit for bit.  One difference drops the resident pair and
 * unlinks its cache files -- the plain pair of rs_group_specialize is independent and stays, and the reverse holds too --; that call
 * returns the built-in kernel's outputs and leaves its state, resident stores included; later resident calls run the built-in resident
 * kernel; the message names cell, field and index ("cell 2: pending_bytes[5] = 1391, the built-in kernel's 1390").
 * rs_group_launch_count counts a checked call once. */
int rs_group_specialize_resident(rs_group* g);
/* rs_group_jit_status for the resident pair: 1 = the group's resident builds serve the resident calls, 0 = rs_group_specialize_resident
 * was not called, -1 = it failed to build, -2 = the builds were dropped by the check.  rs_group_jit_status reports the plain pair only. */
int rs_group_resident_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean resident build of a group of this shape compile?  (the larger code size, or a
 * negative value with the compiler's log in err; RS_SCHED_NVS_NONGREEDY has no group builds) */
int rs_jit_selfcheck_group_resident(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* A run of resident calls (ABI 11 addition, no layout changed): n_ttis consecutive TTIs of every named cell in ONE kernel launch, for the
 * host whose cells are backlogged -- one InfiniteBuffer bearer per user -- and which between two CQI reports (CQI_INTERVAL = 40 TTIs)
 * contributes nothing per TTI but the clock and the rand() pair.  The call is, to the bit, this loop:
 *     for (t = 0; t < n_ttis; t++) rs_group_schedule_tti_at(g, n, cell_ids, in_t, out_t, now_t);
 * with in_t[k] = in[k] but rand0 / rand1 = rands[k][t][0 .. 1] (in[k].rand0 / rand1 themselves are not read), now_t[k] = now[k][t] and
 * out_t[k] = out[k][t].  in[k].cqi_epoch is used as given for every t: a non-zero number makes TTIs 1 .. n_ttis-1 image hits, 0 stays 0
 * -- the block is read each TTI and the cell's image ends.  Everything observable afterwards is what the loop leaves: every field of
 * every rs_tti_out (upper_* lists if asked), slice state, every user's average, pending bytes and last_update, named by the call or
 * not, the cells' image records and the three counters of rs_group_image_stats, and the state of the cells that were not named.  Two
 * things differ on purpose: rs_group_launch_count grows by 1, and rs_group_kernel_name returns "rs_group_run_kernel<sched, ept>" (or
 * "rs_group_run_kernel_jit", rs_group_specialize_run below) while a run was the last call served.  Per workgroup the device repeats
 * steps 1 - 3 of rs_group_schedule_tti_at n_ttis times, in their order and arithmetic, a workgroup barrier behind a device-scope fence
 * between two TTIs, and completes once behind the last.
 * Rules, each RS_ERR_INVALID unless stated, each checked before anything is launched (a rejected call launches nothing and moves nothing):
 *   - every rule of rs_group_schedule_tti_at: cell_ids, uniform presence of cqi_prb and of the upper_* outputs (over every TTI of every
 *     cell), avg_rate NULL, every named cell average-resident (RS_ERR_STATE, the message names the cell; a bearer- or flow-resident
 *     cell too), exponents in {0, 1};
 *   - 1 <= n_ttis <= RS_GROUP_MAX_RUN;
 *   - the users of a cell (n_users, user_id) are the slot's, given once, the same for the whole run;
 *   - hol_delay, prio_has_data, required_rbs and data_to_transmit are NULL: they change per TTI and belong to the host -- so a config
 *     with a customised slice (algo_alpha != 0) is refused;
 *   - RS_SCHED_NVS is refused (the host picks the served slice, and with it the user list, per TTI); the served schedulers are
 *     RS_SCHED_PF, RS_SCHED_GREEDY, RS_SCHED_MAXCELL, RS_SCHED_UPPERBOUND, RS_SCHED_SUBOPT and RS_SCHED_VOGEL;
 *   - rands == NULL only for RS_SCHED_PF, which draws no rand();
 *   - now[k][0] obeys the at-call's clock rule against the cell's last_update; each step now[k][t] - now[k][t-1] is 0 (the
 *     reference's early return: nothing is updated) or at least 2^-20 s.
 * RS_ERR_HIP -- a failed allocation of the larger output blocks included: they grow to slots x n_ttis of the largest run so far -- leaves
 * the named cells not resident and ends their images, as the at-call does.  A run executes the run kernel built into the library
 * unless the group has opted in to run-time builds of it with rs_group_specialize_run below; no other rs_group_specialize* reaches
 * runs.  Bearer-, counted- and flow-resident cells have no runs (their data_to_transmit is the host's per TTI). */
#define RS_GROUP_MAX_RUN 64 /* a sanity bound (>= CQI_INTERVAL = 40), not a tuned number */
int rs_group_run_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, int32_t n_ttis,
                    const double* now /* [n][n_ttis] */, const int32_t* rands /* [n][n_ttis][2]: rand0, rand1 of each TTI; NULL only for RS_SCHED_PF */,
                    rs_tti_out* out /* [n][n_ttis] */);
/* Optional, at any time between two calls, with or without any other rs_group_specialize*: rs_group_specialize_resident for the RUN --
 * the run kernel compiled for the group's shape (entry point rs_group_run_kernel_jit, cache files of its own), a general and a lean
 * build; rs_group_run_at picks the lean one when the run has no per-PRB reports, no upper_* outputs and no synthetic-experiment
 * blocks (and no exact scan; RS_JIT_LEAN=0: the general build only), the general one in every other case.  rs_group_schedule_tti_at
 * and every other call are not affected, and no other rs_group_specialize* reaches runs: the six pairs are independent in both
 * directions.  Cell state, CQI images and the resident stores are not touched.  RS_OK; a second call is a no-op; RS_ERR_HIP if a build
 * fails, the group left on the built-in run kernel; RS_ERR_STATE (with the reason) once the run builds were dropped; RS_ERR_INVALID
 * for RS_SCHED_NVS, RS_SCHED_NVS_NONGREEDY and a config with a customised slice, which no run serves.
 * The check follows rs_group_specialize_resident's policy and switches (RS_DROPIN_SELFCHECK_CALLS, RS_JIT_SELFCHECK, the mark in the
 * cache file); one checked call is one RUN: the slice state, the cell scalars and the resident stores are kept; the built-in run kernel
 * serves the whole run into twin output blocks of slots x n_ttis; what it left is kept and the earlier state put back; then the
 * group's build serves the run, with completion by the stream.  Every rs_tti_out field of every (cell, TTI) (upper_* lists if asked),
 * the slice state, the averages and pending bytes of EVERY user id of the config and last_update must agree bit for bit.  (The image
 * and the per-PRB copy that TTI 0 stores are the same bytes in both executions.)  One difference drops the run pair and unlinks its
 * cache files; that call returns the built-in kernel's outputs and leaves its state, resident stores included; later runs execute
 * the built-in run kernel; the message names cell, TTI, field and index ("cell 2, TTI 6: user_tbs_bits[1] = ...", "cell 2:
 * pending_bytes[5] = 1391, the built-in kernel's 1390").  rs_group_launch_count and rs_group_image_stats count a checked run once. */
int rs_group_specialize_run(rs_group* g);
/* rs_group_jit_status for the run pair: 1 = the group's run builds serve the runs, 0 = rs_group_specialize_run was not called,
 * -1 = it failed to build, -2 = the builds were dropped by the check.  The other status functions report their own pairs only. */
int rs_group_run_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean run build of a group of this shape compile?  (the larger code size, or a
 * negative value with the compiler's log in err; negative with a message for RS_SCHED_NVS and RS_SCHED_NVS_NONGREEDY, which have no run) */
int rs_jit_selfcheck_group_run(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* Counted runs (ABI 11 addition, no layout changed): per-user byte and RB counters for average-resident cells, and runs that advance
 * them.  A backlogged cell holds one InfiniteBuffer bearer per user, so RadioBearer::m_cumulateBytes / m_cumulateRBs -- the numbers
 * behind every "app:" line and every per-slice throughput figure -- are one pair per user id of the config.  AVG-COUNTED is a state on
 * top of average-resident, as counted is on top of bearer-resident:
 * rs_group_set_avg_counters makes an average-resident cell avg-counted and sets its counters ([U] each, by user id; NULL = zeros).  A
 *   synchronising copy outside the fast path.  RS_ERR_STATE when the cell is not average-resident (the message names the cell),
 *   RS_ERR_INVALID for a negative value.  rs_group_set_avg on an avg-counted cell keeps the state and the counters (as
 *   rs_group_set_bearers keeps a counted cell's); rs_group_set_bearers and rs_group_set_flows end it; a call that fails with RS_ERR_HIP
 *   ends it for the cells it named.  rs_group_get_counters and rs_group_set_counters stay bearer-only: their answers on such a cell are
 *   what they were.
 * rs_group_get_avg_counters returns the counters as they are after the last call; RS_ERR_STATE when the cell is not avg-counted.
 * rs_group_run_counted_at is rs_group_run_at with a credit added.  Every rule and every check of rs_group_run_at holds, each before
 *   anything is launched, and every named cell must be avg-counted (RS_ERR_STATE, the message names the cell).  Order of operations and
 *   every result are rs_group_run_at's: every rs_tti_out field, averages, pending bytes, last_update, slice state, image records,
 *   rs_group_image_stats; rs_group_launch_count grows by 1.  In addition, in step 3 of every TTI, every call position i with a grant
 *   (bytes != 0, bytes being what step 3 adds to the pending bytes: min(user_tbs_bits / 8, 100000000)) is credited as DoStopSchedule
 *   credits one bearer per user (ref: downlink-transport-scheduler.cpp:177-190; RS_SCHED_PF: dl-pf-packet-scheduler.cpp:84-85):
 *       cum_bytes[user_id[i]] += bytes;   cum_rbs[user_id[i]] += user_nprb[i];
 *   A position without a grant moves no counter, a user the call does not name moves none; a TTI whose clock step is 0 still credits
 *   (only the update is skipped).
 *   out == NULL is the output-free run, for the whole call: the device writes no rs_tti_out row, the host unpacks none, the output
 *   blocks do not grow; state, counters, image records and statistics are what the same run with outputs leaves.  (The upper_*
 *   uniformity rule then has nothing to check.)
 * rs_group_run_at, rs_group_schedule_tti_at and rs_group_schedule_tti serve an avg-counted cell as before and leave its counters alone
 * (as the queued calls leave a counted cell's).  rs_group_kernel_name returns "rs_group_run_counted_kernel<sched, ept>" while a counted
 * run was the last call served.  Counted runs execute the kernel built into the library, before and after every rs_group_specialize*:
 * rs_group_specialize_run in particular does not reach them; a seventh self-checked pair is left to a later change, as it was for
 * every other form. */
int rs_group_set_avg_counters(rs_group* g, int32_t cell, const int64_t* cum_bytes /* [U] or NULL = zeros */, const int64_t* cum_rbs /* [U] or NULL */);
int rs_group_get_avg_counters(rs_group* g, int32_t cell, int64_t* cum_bytes /* [U] or NULL */, int64_t* cum_rbs /* [U] or NULL */);
int rs_group_run_counted_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, int32_t n_ttis,
                            const double* now /* [n][n_ttis] */, const int32_t* rands /* [n][n_ttis][2]; NULL only for RS_SCHED_PF */,
                            rs_tti_out* out /* [n][n_ttis], or NULL: no per-TTI outputs */);

/* Grant records (ABI 11 addition, no layout changed): what DoStopSchedule logs, from a counted run with or without per-TTI outputs.
 * A TTI serves a handful of users -- every scheduler but UpperBound gives an RBG to one -- so the reference's log of a TTI, its
 * "app:" lines (scheduler 1: "flow:" lines), is a few dozen (position, user, bytes, PRBs, counters) tuples and not U output rows.
 * The thread that credits a grant in step 3 of a counted run writes one rs_grant_record for it.
 * rs_group_grant_bound is the most grants one cell of the group can have in one TTI (> 0): min(n_users, n_rbgs) of the config for
 *   RS_SCHED_PF, _SEQUENTIAL, _MAXCELL, _SUBOPT and _VOGEL, which give an RBG to one user; for RS_SCHED_UPPERBOUND, where an RBG
 *   taken by several slices is a grant for each of them, the sum over the config's slices of min(the slice's users, n_rbgs) -- n_users
 *   when no slice has more users than there are RBGs.
 * rs_group_run_records_at IS rs_group_run_counted_at with the same `out` -- every rule, every check, the order of operations and every
 *   result: outputs if asked, averages, pending bytes, last_update, slice state, counters, image records, rs_group_image_stats;
 *   rs_group_launch_count grows by 1, rs_group_kernel_name says "rs_group_run_counted_kernel<sched, ept>".  In addition, for every
 *   slot k and TTI t, n_recs[k * n_ttis + t] is the number of call positions with a grant (bytes != 0) and
 *   recs[(k * n_ttis + t) * rec_cap + 0 .. n_recs - 1] holds one record per such position, ASCENDING in pos: the order in which
 *   DoStopSchedule walks its users (ref: downlink-transport-scheduler.cpp:177-190; scheduler 1: dl-pf-packet-scheduler.cpp:84-85).
 *   Entries behind the count are not written.  A TTI whose clock step is 0 has its records like any other.
 *   Two more rules, checked with the others before anything is launched (a rejected call launches nothing and moves nothing):
 *   recs and n_recs are both given, and rec_cap >= rs_group_grant_bound(g); RS_ERR_INVALID otherwise.  A larger rec_cap is fine.
 *   Should the device ever count more grants in a TTI than the list holds, nothing is written behind the capacity, n_recs carries the
 *   count as counted, and the call returns RS_ERR_STATE naming cell and TTI -- state and counters are complete then, that TTI's
 *   records are not.  It would mean that rs_group_grant_bound is wrong.
 * rs_group_run_counted_at itself is what it was, with and without outputs. */
typedef struct rs_grant_record { /* 32 bytes */
  int32_t pos;       /* call position i of the served user */
  int32_t user_id;   /* user_id[i], or i when the call names no ids */
  int32_t bytes;     /* what step 3 credits: min(user_tbs_bits[i] / 8, 100000000); never 0 */
  int32_t nprb;      /* rs_tti_out.user_nprb[i] */
  int64_t cum_bytes; /* the user's counters AFTER this TTI's credit */
  int64_t cum_rbs;
} rs_grant_record;
int rs_group_grant_bound(const rs_group* g);
int rs_group_run_records_at(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, int32_t n_ttis,
                            const double* now /* [n][n_ttis] */, const int32_t* rands /* [n][n_ttis][2]; NULL only for RS_SCHED_PF */,
                            rs_tti_out* out /* [n][n_ttis], or NULL: no per-TTI outputs */, int32_t rec_cap,
                            rs_grant_record* recs /* [n][n_ttis][rec_cap] */, int32_t* n_recs /* [n][n_ttis] */);

/* Resident bearers (ABI 11 addition, no layout changed): the second resident form of a group's cell.  The cell keeps, per user id of the
 * config and per bearer (MAX_BEARERS = 2, index = the bearer's priority), RadioBearer's average rate and the bytes DoStopSchedule
 * credited since the last update, and whether the bearer exists; one last_update per cell (the reference's bearers all share it from
 * their first DoSchedule() on).  The caller passes what SelectFlowsToSchedule formed: data_to_transmit[k][i][b] is
 * UserToSchedule::m_dataToTransmit[b] of the call's i-th user -- 100000000 for an InfiniteBuffer bearer, the queue size with MAC
 * overhead for a finite one, 0 for a bearer without packets or without existence.  Per slot of rs_group_schedule_tti_queued, in this order:
 *   1. now == last_update: nothing.  Otherwise, for every EXISTING bearer of every user id of the config, named or not:
 *      rate = (double)(pending * 8) / (now - last_update);  a = ((1 - 0.02) * a) + (0.02 * rate);  if (a < 1) a = 1;  pending = 0;
 *      -- then last_update = now.  Step 1 of rs_group_schedule_tti_at per bearer: same operations, same wrapping int product, unfused.
 *      A bearer that does not exist is neither read nor written.
 *   2. Position i's average is the sum over the bearers WITH DATA (the reference sums the bearers it inserted, ComputeSchedulingMetric
 *      downlink-transport-scheduler.cpp:681-687), in the form whose 1 + x the kernel takes: a[b] when only bearer b has data,
 *      ((1 + a0) + a1) - 1 when both have -- exact while the sum stays below 2^53, hence the bound on the averages.
 *   3. The TTI is scheduled as by rs_group_schedule_tti on those averages; hol_delay, prio_has_data, required_rbs, cqi / cqi_prb,
 *      cqi_epoch, user_id, rand0 / rand1 stay the caller's.
 *   4. DoStopSchedule's loop (:170-221) per position: available = tbs_bits / 8; for b = 1, 0: stop when available <= 0; if
 *      data[b] > 0: sent = min(available, data[b]); available -= sent; pending[user][b] += sent.
 * Update-only slots: in[k].n_users == 0 is accepted by this call alone -- a finite-queue cell often has nobody to schedule, and the
 * reference then skips RBsAllocation (:163-165) but has run the update.  Such a slot does step 1 alone: no rand() pair is consumed
 * (rand0 / rand1 are not read), slice state and CQI image are untouched, nothing else of in[k] is read, and out[k] reads "nothing
 * scheduled" (rbg_to_user -1, target_rbs / quota_rbgs 0; out[k]'s arrays may be NULL).  A call whose slots are all update-only
 * still launches once.  RS_SCHED_NVS: the caller chooses the served slice, and an update-only slot moves no slice state.
 * Queued calls run the built-in "rs_group_queued_kernel<sched, ept>" (rs_group_kernel_name while a queued call is the last one
 * served); rs_group_specialize and rs_group_specialize_resident do not reach them: same results before and after either.  A group
 * that wants run-time builds of this form opts in with rs_group_specialize_queued below. */
/* Makes `cell` bearer-resident (again, at any time between two calls; a cell is average-resident or bearer-resident, the later of
 * rs_group_set_avg / rs_group_set_bearers wins): has_bearer[U][2] and avg[U][2] by user id and bearer priority, zero pending bytes.
 * A user may have no bearer at all; avg of a bearer that does not exist is not read.  RS_ERR_INVALID: RS_SCHED_PF (it races flows
 * and credits the whole block to the flow), RS_SCHED_UPPERBOUND and RS_SCHED_NVS_NONGREEDY (no restatement with queues to check
 * against); exponents outside {0, 1}; an existing bearer's average outside 1..2^51 (so that (1 + a0) + a1 < 2^53); a
 * last_update that is not finite. */
int rs_group_set_bearers(rs_group* g, int32_t cell, const uint8_t* has_bearer /* [U][2], index = bearer priority */,
                         const double* avg /* [U][2] */, double last_update);
/* The bearer state as it is after the last call (a synchronising copy; not part of a TTI); 0 for a bearer that does not exist.  Each
 * output may be NULL.  RS_ERR_STATE: the cell is not bearer-resident. */
int rs_group_get_bearers(rs_group* g, int32_t cell, double* avg /* [U][2] or NULL */, int32_t* pending_bytes /* [U][2] or NULL */,
                         double* last_update /* or NULL */);
/* rs_group_schedule_tti for bearer-resident cells.  Every rule of a group call holds (uniform presence of optional inputs among the
 * slots that have users, cqi_epoch per cell, subsets and permutations through cell_ids; a rejected call launches nothing and moves
 * nothing; rs_group_launch_count and rs_group_image_stats count these calls like any others -- an update-only slot counts in no
 * image statistic), and
 *   - in[k].avg_rate is NULL for every k (RS_ERR_INVALID);
 *   - every named cell is bearer-resident (RS_ERR_STATE); rs_group_schedule_tti_at on such a cell is RS_ERR_STATE too, while
 *     rs_group_schedule_tti works on it and touches none of its resident state;
 *   - the clock rules of rs_group_schedule_tti_at, unchanged;
 *   - data_to_transmit[k] may be NULL only when in[k].n_users == 0; every data word is >= 0, a named user has data in at least one
 *     bearer, and data > 0 only where the bearer exists (RS_ERR_INVALID; the library keeps a mirror of has_bearer on the host).
 * A call that fails with RS_ERR_HIP leaves the cells it named not resident. */
int rs_group_schedule_tti_queued(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, rs_tti_out* out /* [n] */,
                                 const double* now /* [n] */, const int32_t* const* data_to_transmit /* [n]: [in[k].n_users][2] */);
/* Optional, at any time between two calls, with or without rs_group_specialize and rs_group_specialize_resident: rs_group_specialize for
 * the QUEUED call -- the queued kernel compiled for the group's shape (entry point rs_group_queued_kernel_jit, cache files of its own), a
 * general and a lean build; rs_group_schedule_tti_queued picks the lean one under the plain call's per-launch condition, taken among the
 * slots that have users (no per-PRB reports, no customised slices, no gate, no exact scan, no synthetic-experiment blocks;
 * RS_JIT_LEAN=0: the general build only).  A call made of update-only slots only has no such inputs: it runs the lean build, unless the
 * config itself rules that build out (customised slices, synthetic-experiment blocks); either build does the same update.  The other
 * two call forms are not affected.  Cell state, CQI images and the bearer stores are not touched.  RS_OK; a second call is a no-op;
 * RS_ERR_HIP if a build fails, the group left on the built-in queued kernel; RS_ERR_STATE (with the reason) once the queued builds were
 * dropped; RS_ERR_INVALID for a scheduler without a queued form (RS_SCHED_PF, RS_SCHED_UPPERBOUND).
 * The check follows rs_group_specialize_resident's policy and switches (RS_DROPIN_SELFCHECK_CALLS, RS_JIT_SELFCHECK, the mark in the
 * cache file): before a checked call the slice state, the cell scalars and the bearer stores (averages, pending bytes, last_update) are
 * kept; the built-in queued kernel runs into twin output slots; what it left is kept and the earlier state put back; then the group's
 * build runs, with completion by the stream.  For every named cell the rs_tti_out fields, the slice state, avg[U][2] and
 * pending_bytes[U][2] of EVERY user id of the config and last_update must agree bit for bit; an update-only slot is compared on state
 * alone, and a call made only of such slots is a checked call like any other.  One difference drops the queued pair and unlinks its
 * cache files -- the plain and the resident pair are independent and stay, and the reverse holds too --; that call returns the built-in
 * kernel's outputs and leaves its state, bearer stores included; later queued calls run the built-in queued kernel; the message names
 * cell, field and index ("cell 1: pending_bytes[7][0] = 301, the built-in kernel's 300").  rs_group_launch_count counts a checked call
 * once. */
int rs_group_specialize_queued(rs_group* g);
/* rs_group_jit_status for the queued pair: 1 = the group's queued builds serve the queued calls, 0 = rs_group_specialize_queued was not
 * called, -1 = it failed to build, -2 = the builds were dropped by the check.  rs_group_jit_status and rs_group_resident_jit_status keep
 * reporting their own pair only. */
int rs_group_queued_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean queued build of a group of this shape compile?  (the larger code size, or a
 * negative value with the compiler's log in err; negative for the schedulers without a queued form: RS_SCHED_PF, RS_SCHED_UPPERBOUND,
 * RS_SCHED_NVS_NONGREEDY) */
int rs_jit_selfcheck_group_queued(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* Counted bearers (ABI 11 addition, no layout changed): a bearer-resident cell may also keep RadioBearer's m_cumulateBytes and
 * m_cumulateRBs of both bearers of every user id on the device -- the numbers of the reference's "app:" log lines and per-slice
 * throughput figures -- and a call through rs_group_schedule_tti_counted returns dataTransmitted per bearer, what a binding passes to
 * UpdateTransmittedBytes and rlc->TransmissionProcedure (ref: downlink-transport-scheduler.cpp:170-221, downlink-nvs-scheduler.cpp:221-273).
 * Such a call is rs_group_schedule_tti_queued in every rule, order of operations and result; in its step 4, for call position i, user
 * id u and every bearer b that is credited (data[b] > 0 reached with available > 0):
 *      cum_bytes[u][b] += sent;  cum_rbs[u][b] += the position's allocated PRBs (rs_tti_out.user_nprb[i]: the reference's
 *      GetListOfAllocatedRBs()->size(), the same count for both bearers of a split grant);  sent[k][i][b] = sent,
 * and sent[k][i][b] = 0 for a bearer that is not credited.  Update-only slots and positions without a grant move no counter.
 * Counted calls run the built-in "rs_group_counted_kernel<sched, ept>", after rs_group_specialize_queued too; a host that wants
 * run-time builds of this form opts in with rs_group_specialize_counted below. */
/* Makes a bearer-resident `cell` counted (again, at any time between two calls) and sets its counters: [U][2] by user id and bearer
 * priority, NULL = zeros.  A synchronising copy outside the fast path.  RS_ERR_STATE: the cell is not bearer-resident; RS_ERR_INVALID:
 * a negative value.  rs_group_set_bearers leaves the counters and the counted state as they are (a bearer that does not exist is
 * never written by a call); rs_group_set_avg ends the counted state, and so does a call that fails with RS_ERR_HIP for the cells it
 * named.  rs_group_schedule_tti_queued and rs_group_schedule_tti serve a counted cell as before and leave its counters alone. */
int rs_group_set_counters(rs_group* g, int32_t cell, const int64_t* cum_bytes /* [U][2] or NULL = zeros */, const int64_t* cum_rbs /* [U][2] or NULL */);
/* The counters as they are after the last call (a synchronising copy; not part of a TTI).  Each output may be NULL.  RS_ERR_STATE: the
 * cell is not counted. */
int rs_group_get_counters(rs_group* g, int32_t cell, int64_t* cum_bytes /* [U][2] or NULL */, int64_t* cum_rbs /* [U][2] or NULL */);
/* rs_group_schedule_tti_queued for counted cells: its rules (update-only slots, the clock rules, cqi_epoch, subsets and permutations,
 * a rejected call launches nothing and moves nothing, launch and image statistics), and every named cell is counted (RS_ERR_STATE, the
 * message names the cell).  sent may be NULL (the counters alone are kept); sent[k] may be NULL for an update-only slot, and for any
 * slot whose rows the caller does not want. */
int rs_group_schedule_tti_counted(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, rs_tti_out* out /* [n] */,
                                  const double* now /* [n] */, const int32_t* const* data_to_transmit /* [n]: [in[k].n_users][2] */,
                                  int32_t* const* sent /* [n]: [in[k].n_users][2]; NULL, or NULL per update-only slot */);
/* rs_group_specialize_queued for the COUNTED call (ABI 11 addition), to the letter: the counted kernel compiled for the group's shape
 * (entry point rs_group_counted_kernel_jit, cache files of its own), a general and a lean build picked by the queued call's per-launch
 * condition (a call made of update-only slots only takes the lean build, unless the config rules it out); at any time between two
 * calls, a second call is a no-op; RS_ERR_HIP if a build fails, the group left on the built-in counted kernel; RS_ERR_STATE (with the
 * reason) once the counted builds were dropped; RS_ERR_INVALID for a scheduler without the form.  The six pairs (the run pair of rs_group_specialize_run included) are independent in
 * both directions: rs_group_specialize_queued does not reach counted calls, this one does not reach queued calls.
 * The check is the queued pair's (policy, switches, the mark in the cache file) on more stores: for every user id of the config and
 * both bearers avg, pending_bytes, last_update, cum_bytes[U][2] and cum_rbs[U][2] (int64, bit for bit) are kept, put back and compared,
 * and so is sent[k][i][b] of every named slot that has users -- the built-in kernel writes a twin sent block, allocated by the first
 * checked call, whether or not the caller passes `sent` or a slot's row.  One difference drops the counted pair alone and unlinks its two
 * cache files; that call returns the built-in kernel's outputs, sent rows and state with RS_OK; later counted calls run the built-in
 * kernel; the message names cell, field and index ("cell 1: cum_rbs[7][0] = 5, the built-in kernel's 4", "cell 0: sent[3][1] = 301, the
 * built-in kernel's 300").  rs_group_launch_count counts a checked call once. */
int rs_group_specialize_counted(rs_group* g);
/* rs_group_jit_status for the counted pair: 1 / 0 / -1 / -2 as rs_group_queued_jit_status; every status reports its own pair only. */
int rs_group_counted_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean counted build of a group of this shape compile?  (the larger code size, or a
 * negative value with a message for the schedulers without the form, rs_jit_selfcheck_group_queued's) */
int rs_jit_selfcheck_group_counted(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* Resident flows (ABI 11 addition, no layout changed): RS_SCHED_PF alone.  DL_PF_PacketScheduler races FLOWS -- bearers with data, in
 * RRC-container order --, divides by the flow's own average and credits the whole transport block to the flow (ref:
 * downlink-packet-scheduler.cpp:179-331, dl-pf-packet-scheduler.cpp:64-140), so its resident form is one of its own: a cell of a
 * scheduler-1 group may keep, for both bearers of every user id, the average, the bytes credited since the last update, the existence
 * byte, m_cumulateBytes and m_cumulateRBs on the device.  A slot of a flows call, in this order:
 *   1. UpdateAverageTransmissionRate for every existing bearer of every user id (rs_group_schedule_tti_queued's step 1, and its clock
 *      rules: now == last_update is the early return);
 *   2. call position i is bearer flow_bearer[k][i] of user user_id[i], and its average is that bearer's;
 *   3. RBsAllocation on the positions with the data_to_transmit gate, as rs_group_schedule_tti serves it for RS_SCHED_PF;
 *   4. for every position with a grant: bytes = user_tbs_bits[i] / 8;  pending[u][b] += bytes;  cum_bytes[u][b] += bytes;
 *      cum_rbs[u][b] += user_nprb[i] -- no min with the data: the reference hands the whole block to the RLC.
 * rs_group_set_bearers stays refused on a scheduler-1 group, and the queued, counted and resident-average calls refuse a flow-resident
 * cell (RS_ERR_STATE); rs_group_schedule_tti serves it as before and touches none of this state.  Flows calls run the built-in
 * "rs_group_flows_kernel<1, 0>"; a host that wants run-time builds of this form opts in with rs_group_specialize_flows below. */
/* Makes `cell` flow-resident (again, at any time between two calls): has_bearer and avg [U][2] by user id and bearer index, zero
 * pending bytes, last_update, and the counters (NULL = zeros).  A cell is resident in one form at a time: the later of
 * rs_group_set_avg / rs_group_set_flows wins.  RS_ERR_INVALID: the scheduler is not RS_SCHED_PF (not served); exponents outside
 * {0, 1}; an existing bearer's average outside 1..2^51; a last_update that is not finite; a negative counter. */
int rs_group_set_flows(rs_group* g, int32_t cell, const uint8_t* has_bearer /* [U][2] */, const double* avg /* [U][2] */, double last_update,
                       const int64_t* cum_bytes /* [U][2] or NULL = zeros */, const int64_t* cum_rbs /* [U][2] or NULL */);
/* The flows' state as it is after the last call (a synchronising copy; not part of a TTI): zeros for a bearer that does not exist.
 * Each output may be NULL.  RS_ERR_STATE: the cell is not flow-resident. */
int rs_group_get_flows(rs_group* g, int32_t cell, double* avg /* [U][2] */, int32_t* pending_bytes /* [U][2] */, double* last_update,
                       int64_t* cum_bytes /* [U][2] */, int64_t* cum_rbs /* [U][2] */);
/* One TTI of n flow-resident cells: every rule of a group call (subsets and permutations through cell_ids, uniform presence of cqi_prb,
 * cqi_epoch per cell, one launch) and the clock rules of rs_group_schedule_tti_at.  in[k].n_users counts the call's FLOWS (<= the
 * config's n_users: a host with N users x 2 bearers creates the group with n_users = its largest flow count); user ids are below the
 * config's n_users, user_id == NULL means user i; the pairs (user_id[i], flow_bearer[k][i]) ascend strictly in lexicographic order, so
 * a user may hold two adjacent positions and no flow is named twice.  avg_rate, hol_delay, prio_has_data and required_rbs must be
 * NULL; data_to_transmit is required, every word > 0, and the bearer must exist; cqi / cqi_prb hold one row per position.
 * n_users == 0 is an update-only slot (flow_bearer[k] may be NULL; its outputs read "nothing scheduled").  Outputs are per position;
 * rbg_to_user[r] holds the flow id 2 * user + bearer.  A rejected call launches nothing and moves nothing (RS_ERR_STATE names the
 * cell that is not flow-resident); RS_ERR_HIP ends the flow-resident state of the cells the call named. */
int rs_group_schedule_tti_flows(rs_group* g, int32_t n, const int32_t* cell_ids, const rs_tti_in* in /* [n] */, rs_tti_out* out /* [n] */,
                                const double* now /* [n] */, const uint8_t* const* flow_bearer /* [n]: [in[k].n_users], 0 or 1 */);
/* rs_group_specialize_queued for the FLOWS call (ABI 11 addition): the flows kernel compiled for the group's shape (entry point
 * rs_group_flows_kernel_jit, cache files of its own), a general and a lean build.  A flows call always carries the data_to_transmit gate,
 * so its lean build keeps the gate and is picked when no slot brings per-PRB reports, the exact scan or synthetic-experiment blocks (and
 * the config has no customised slices).  When, errors, independence of the pairs and the check are rs_group_specialize_counted's;
 * RS_ERR_INVALID for every scheduler but RS_SCHED_PF.  The check keeps, puts back and compares avg, pending_bytes, last_update,
 * cum_bytes[U][2] and cum_rbs[U][2] of every user id and both bearers; the message names cell, field and index ("cell 2:
 * cum_bytes[4][1] = 1201, the built-in kernel's 1200"). */
int rs_group_specialize_flows(rs_group* g);
/* rs_group_jit_status for the flows pair: 1 / 0 / -1 / -2 as rs_group_queued_jit_status; every status reports its own pair only. */
int rs_group_flows_jit_status(rs_group* g, char* msg, size_t msglen);
/* build check without a GPU: do the general and the lean flows build of a group of this shape compile?  (the larger code size, or a
 * negative value with a message for every scheduler but RS_SCHED_PF) */
int rs_jit_selfcheck_group_flows(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err, size_t errlen);

/* ------------------------------------------------------------------------------------------
 * Batched mode: many independent cells resident on the device, whole DoSchedule() loops
 * (EWMA update -> RBsAllocation -> DoStopSchedule accounting) run in one launch.
 * Replaces, per cell and per TTI: RadioBearer::UpdateAverageTransmissionRate
 * (ref: src/flows/radio-bearer.cpp:139-164), SelectSliceToServe (NVS), RBsAllocation,
 * DoStopSchedule's counters (ref: downlink-transport-scheduler.cpp:170-221), the CQI refresh
 * (ref: src/protocolStack/mac/enb-mac-entity.cc:160-193, src/device/CqiManager/cqi-manager.cpp:94-123)
 * and the simulator clock t_k = fl(t_{k-1} + 0.001) (ref: src/core/eventScheduler/simulator.cc:117-126).
 * ------------------------------------------------------------------------------------------ */
typedef struct rs_batch rs_batch;

typedef struct rs_batch_config {
  rs_config cell;            /* every cell of the batch shares this configuration -- but for the four
                              * per-slice / per-user arrays once rs_batch_set_cell_configs gave the cells rows of their own */
  int32_t n_cells;
  int32_t first_tti;         /* TTI index of the first scheduled TTI (reference: 100 = 0.1 s)   */
  int32_t cqi_refresh;       /* synthetic/epoch source: new grid every this many TTIs (40)      */
  int32_t phy_error_draws;   /* 1: consume one rand() per UE served in the previous TTI, as the
                                reference's PHY error model does on the shared libc stream
                                (ref: src/phy/wideband-cqi-eesm-error-model.cpp:69)              */
  int32_t threads_per_cell;  /* workgroup size, multiple of 64 in [64,512] ([64,1024] with jit = 1: the built-in kernels
                                are bounded at 512); 0 = default: 512, or 256 once the batch puts 4 or more cells on
                                every CU.  More than 512 threads work with jit = 1 but are never chosen automatically
                                (640 on the 64-RBG grid: 8.55 against 13.58 M TTIs/s, profiles/r04_r64.md)          */
  int32_t jit;               /* 1: compile the cell kernel for this batch's exact shape at create time
                                (hiprtc, ~2 s, cached per process); results are identical, the built-in
                                kernels are used if the compilation fails (rs_batch_jit_status tells).  0: built-in kernels.
                                The environment variable RS_JIT=0|1 overrides.  Unlogged launches of at least 256 TTIs
                                (RS_JIT_LEAN_MIN_TTIS) on epoch grids without per-PRB twins, error-model draws or synthetic-experiment
                                blocks run the LEAN build of that kernel (those launch options as compile-time constants; compiled at
                                the first such launch, ~2 s; identical results; RS_JIT_LEAN=0 keeps the general build).  A batch with
                                cqi_refresh <= 4 gets kernels that fetch the next grid during the serial end of the TTI.        */
  int32_t cqi_epoch_wrap;    /* epoch sources (upload / synthesize): 0 = running past the last epoch is RS_ERR_RANGE;
                                1 = the epochs cycle (epoch index modulo n_epochs) -- a bounded set of grids serves a
                                run of any length, e.g. the streamed-CQI measurement with cqi_refresh = 1 (ABI 9)  */
  int32_t queue_state_lds;   /* queue model: where the bearers' hot words (156 B per user) live during a launch.
                                0 = automatic: LDS when the cell still fits the CU's 160 KB, except when that is what
                                takes the cell over 80 KB (one cell per CU instead of two) in a batch of more cells
                                than CUs; 1 = LDS whenever it fits; -1 = HBM (ABI 9)                              */
  int32_t autotune;          /* 1 (with jit = 1; schedulers 8, 9, 101, 103 without the queue model): before the batch's first long
                                unlogged launch (or in rs_batch_prepare_launch) the lean kernel is built in two or three variants
                                the library's rule table chooses between -- LLVM scheduler strategy, speculative next-TTI scan /
                                held winners on or off, users per stage-1 block --, each is timed on the batch's next
                                min(n_ttis, 512) TTIs from a snapshot of the whole cell state that is put back afterwards, and the
                                fastest serves the batch.  Every variant is exact, so results do not depend on the choice; cost
                                ~2 s of hiprtc per variant once per shape and machine (the code objects are cached on disk).
                                rs_batch_autotune_report tells what was measured.  0 = the rule table alone.  Every trial's final
                                state is compared with the rule table's build: a variant that disagrees is never kept.  (ABI 10) */
  int32_t selfcheck;         /* The self-check of a batch's run-time builds (jit = 1, up to 512 threads per cell): before the batch's first
                                launch (or in rs_batch_prepare_launch) its next min(n_ttis, 256) TTIs run on the kernels built into the
                                library and on its run-time compiled ones (general build; the lean build before the first launch that
                                uses it), each from the same snapshot of the whole cell state -- bearers' queues included --, which is put
                                back; the final states must agree bit for bit.  The built-in kernels are one binary -- the one the GPU
                                parity suite checks against the oracle --, a run-time build is a fresh compilation for this shape.  A
                                general build that disagrees is dropped: the batch runs on the built-in kernels and rs_batch_jit_status
                                returns -2 with the reason; a lean build that disagrees alone is dropped alone.
                                0 (default, ABI 11): every build that does not carry the self-check mark -- compiled by this process, or
                                loaded from a cache file no process has checked yet; a build that passes gets the mark in its cache file,
                                so only the first process of a campaign pays (RS_JIT_SELFCHECK=0 switches this default off).
                                1: every build, marked or not.  -1: never.  (ABI 10; default on and -1 since ABI 11)            */
} rs_batch_config;

rs_batch* rs_batch_create(const rs_batch_config* cfg);
rs_batch* rs_batch_create_checked(const rs_batch_config* cfg, int abi_version, size_t cfg_size);
#define RS_BATCH_CREATE(cfg) rs_batch_create_checked((cfg), RS_ABI_VERSION, sizeof(rs_batch_config))
void rs_batch_destroy(rs_batch* b);

/* per-cell libc-compatible rand() streams: srand(seed[c]) then rand_skip[c] values discarded
 * (ref: src/scenarios/single-cell-with-interference.h:84-89, src/utility/seed.h:25-35) */
int rs_batch_seed(rs_batch* b, const uint32_t* seed /* [n_cells] */, const int64_t* rand_skip /* [n_cells] or NULL */);
/* Per-cell slice configurations (ABI 11 addition): what the reference's run scripts vary between the processes they start besides the
 * seed and the trace mapping -- the configuration file -- varied between the cells of one batch.  Each array holds one row per cell; a
 * NULL array leaves every cell the shared rs_config's values of that field.  Cell c then behaves, to the bit, like cell 0 of a one-cell
 * batch created from an rs_config that holds row c (logged rows, PF averages, counters, slice state, clock, rand() ring).  Shared as
 * before: n_slices, n_users, n_rbgs, rbg_size, sched, algo_alpha, algo_beta, synthetic_exp, link_tables.  Before the first TTI only
 * (RS_ERR_STATE afterwards, as for rs_batch_seed); a second call replaces the first.  Every row is validated as a configuration is --
 * slice ids in range and non-decreasing (empty slices allowed), algo_epsilon / algo_psi 0 or 1, finite weights -- and each cell's
 * slice state against its own weights by rs_batch_write_state's domain rule: RS_ERR_INVALID naming the cell and the index, nothing
 * stored.  RS_SCHED_NVS_NONGREEDY: RS_ERR_INVALID (its kernel is another one).  A batch with the queue model: RS_ERR_STATE, and
 * rs_batch_set_bearers after this call likewise (slice priorities and customised slices stay uniform).  With jit = 1 the run-time
 * builds are compiled again, for the longest slice window of any cell, and self-checked as any build is; a checkpoint loads only into
 * a batch that was given the same rows; rs_batch_grant_bound for RS_SCHED_UPPERBOUND is the largest cell's; rs_batch_slice_bytes reads
 * each cell's own map.
 * Cells of different user counts (ragged batches): a row of user_to_slice may END in RS_USER_ABSENT entries -- n_c >= 1 entries valid as
 * above, then U - n_c times RS_USER_ABSENT.  Cell c then behaves, to the bit, like cell 0 of a one-cell batch created with n_users = n_c
 * from the row's first n_c entries, in everything that batch returns about users 0 .. n_c - 1; its grids, trace mapping and state rows
 * are the first n_c rows of the cell's.  The absent users u >= n_c are never scanned and never granted: they are in no record and in no
 * rbg_to_user entry, their logged rows read as an unserved user's, and their cum_bytes / cum_rbs / avg_rate words keep, bit for bit,
 * what they held (no decay, no write); their CQI rows, h_user_trace entries and rs_batch_write_state words are accepted, stored and
 * ignored.  RS_ERR_INVALID naming cell and user: a slice id behind an RS_USER_ABSENT, a row of nothing else, any other negative value.
 * The shared rs_config takes no RS_USER_ABSENT.  rs_batch_grant_bound counts each cell's own users (min(n_c, R); UpperBound: per slice)
 * and returns the largest cell's; the slice window is taken over the present users; rs_batch_slice_bytes / rs_batch_slice_totals skip
 * the absent ones; the checkpoint hash covers the suffixes, so a checkpoint loads only into a batch of the same counts; run-time builds
 * of a batch with an absent user carry -DRS_JIT_CELL_CONFIGS=2 (any other batch's builds are what they were).
 * Cells of different slice counts: rs_batch_set_cell_configs_n below.  Still uniform: R, algo_alpha / algo_beta. */
#define RS_USER_ABSENT (-1)
int rs_batch_set_cell_configs(rs_batch* b,
        const double*  slice_weight  /* [n_cells][S] or NULL */,
        const int32_t* algo_epsilon  /* [n_cells][S] or NULL */,
        const int32_t* algo_psi      /* [n_cells][S] or NULL */,
        const int32_t* user_to_slice /* [n_cells][U] or NULL */);
/* one cell's row of the four (the shared configuration's where no rows were given); any output may be NULL */
int rs_batch_get_cell_config(rs_batch* b, int32_t cell, double* slice_weight /* [S] or NULL */,
        int32_t* algo_epsilon, int32_t* algo_psi, int32_t* user_to_slice /* [U] or NULL */);
/* per cell and slice, the sums of the users' cumulative bytes and RBs by the cell's own map, reduced on the device (exact integer sums):
 * the two panels of the reference's plot_throughput.py:26-56, per cell */
int rs_batch_slice_totals(rs_batch* b, int64_t* cum_bytes /* [n_cells][S] or NULL */, int64_t* cum_rbs /* [n_cells][S] or NULL */);
/* every cell's user count n_c: the entries of its row before the RS_USER_ABSENT suffix; U for every cell of a batch without rows */
int rs_batch_cell_users(rs_batch* b, int32_t* n_users /* [n_cells] */);
/* rs_batch_set_cell_configs with a slice count per cell: 1 <= cell_slices[c] <= S (the batch's n_slices); cell_slices == NULL: exactly
 * rs_batch_set_cell_configs.  The reference's run scripts sweep the slice count too (5, 10, 15 and 20 slices as separate processes), and a
 * smaller count cannot be had by padding with empty zero-weight slices: both quota rotations are (i + rand()) % num_slices_ and
 * MaximizeCell's std::sort runs over nb_rbgs * nb_slices records, whose order among equal keys depends on the length.
 * Cell c behaves, to the bit, like cell 0 of a one-cell batch created with n_slices = S_c (and n_users = n_c) from the heads of its rows,
 * in everything the batch returns about slices 0 .. S_c - 1 and users 0 .. n_c - 1: logged rows, grant records, PF averages, counters,
 * slice state, clock, rand() ring, heap-sort counters.  The absent slices s >= S_c take part in nothing: their quota, target and
 * slice_keys log entries are 0; their slice_state words keep, bit for bit, what they held (rs_batch_write_state accepts and stores values
 * for them outside its domain rule, the kernel never writes them); their entries in the three per-slice rows are stored, returned by
 * rs_batch_get_cell_config as given, not validated and ignored; rs_batch_slice_totals returns 0 for them and rs_batch_slice_bytes adds
 * nothing for them (no user is theirs).  RS_ERR_INVALID naming cell and index, nothing stored: a count outside 1..S, a user_to_slice id
 * >= S_c in front of the absent-user suffix, and everything rs_batch_set_cell_configs checks, applied to the heads.  A row may combine
 * fewer slices with an absent-user suffix, or have fewer slices with all U users.  Refusals as for rs_batch_set_cell_configs; a later
 * call of either function replaces the earlier one.  rs_batch_grant_bound for RS_SCHED_UPPERBOUND sums over each cell's own slices; the
 * checkpoint hash covers the counts where one is below S; run-time builds of a batch with such a cell carry RS_JIT_CELL_CONFIGS | 4
 * (-DRS_JIT_CELL_CONFIGS=5 or 6; any other batch's builds, option lists and cache keys are what they were). */
int rs_batch_set_cell_configs_n(rs_batch* b, const int32_t* cell_slices /* [n_cells] or NULL */,
        const double* slice_weight, const int32_t* algo_epsilon, const int32_t* algo_psi, const int32_t* user_to_slice);
/* every cell's slice count S_c; S for every cell of a batch without counts */
int rs_batch_cell_slices(rs_batch* b, int32_t* n_slices /* [n_cells] */);

/* CQI source A: explicit grids. h_cqi = [n_cells][n_epochs][U][R] (host); epoch e serves scheduled
 * TTIs [e*cqi_refresh, (e+1)*cqi_refresh).  Copied to HBM once. */
int rs_batch_upload_cqi_epochs(rs_batch* b, const uint8_t* h_cqi, int32_t n_epochs);
/* CQI source A, per PRB: h_cqi_prb = [n_cells][n_epochs][U][R*rbg_size], reports that may differ inside an RBG (what
 * enb-mac-entity.cc:173-186 stores: all PRBs).  The metric reads PRB rbg*rbg_size (ref: downlink-transport-scheduler.cpp:536), link
 * adaptation every allocated PRB (ref: :643-646). */
int rs_batch_upload_cqi_epochs_prb(rs_batch* b, const uint8_t* h_cqi_prb, int32_t n_epochs);
/* CQI source B: i.i.d. grids drawn on the device from a CQI histogram (weights of CQI 1..15),
 * counter-based generator keyed by (seed, cell, epoch, user, rbg).  Stays in HBM. */
int rs_batch_synthesize_cqi(rs_batch* b, uint64_t seed, const double* cqi_weights /* [15] */, int32_t n_epochs);
/* same with the batch's cells numbered first_cell .. first_cell + n_cells - 1: the generator is keyed by the GLOBAL cell id,
 * so a cell's grids do not depend on how a job's cells are sharded over ranks (rs_batch_synthesize_cqi: first_cell = 0) */
int rs_batch_synthesize_cqi_at(rs_batch* b, uint64_t seed, const double* cqi_weights /* [15] */, int32_t n_epochs,
                               int64_t first_cell);
/* read back the grids of one cell (either source) for the parity tests: [n_epochs][U][R] */
int rs_batch_download_cqi_epochs(rs_batch* b, int32_t cell, uint8_t* h_cqi);
/* CQI source A from device memory: d_cqi = [n_cells][n_epochs][U][R] bytes ON THE BATCH'S DEVICE, values 1..15, at any byte
 * alignment (a view of a larger buffer will do).  What rs_batch_upload_cqi_epochs does with the same bytes, with the packing into
 * the kernels' image done by a kernel on the batch's stream; the call waits for it.  d_bytes must be the byte count the shape
 * implies and d_cqi device memory of the batch's device (hipPointerGetAttributes; a host or managed pointer is RS_ERR_INVALID):
 * both are checked before anything is enqueued or stored.  The values are checked by the kernel: a byte outside 1..15 is stored
 * as CQI 1, and the call returns RS_ERR_INVALID naming the lowest such byte ("CQI %d at byte %lld outside 1..15") and leaves the
 * batch WITHOUT a CQI source, as if none had been set, until a later call succeeds. */
int rs_batch_set_cqi_epochs_device(rs_batch* b, const uint8_t* d_cqi, size_t d_bytes, int32_t n_epochs);
/* Rewrites epochs [first_epoch, first_epoch + n) of the epoch grids in place: d_cqi = [n_cells][n][U][R] device bytes as above, no
 * allocation, the other epochs untouched.  1 <= n <= n_epochs, 0 <= first_epoch < n_epochs; with cqi_epoch_wrap the epoch indices
 * are taken modulo n_epochs, without it a window that runs past the end is RS_ERR_RANGE.  RS_ERR_STATE for a batch without epoch
 * grids and for one with a per-PRB twin (which would no longer match).  The pack is enqueued on the batch's stream: behind the
 * launches made so far, ahead of the later ones -- a producer may refill the epochs a run has consumed while the batch goes on
 * (the ring: DESIGN.md 2.1).  Without RS_CQI_WRITE_ASYNC the call waits and reports like the setter.  With it the call returns
 * after the enqueue; values outside 1..15 run as CQI 1 and are reported by rs_batch_cqi_write_status.  The caller orders its
 * producer ahead of the batch's stream and keeps d_cqi alive until the stream has passed the pack. */
#define RS_CQI_WRITE_ASYNC 1u
int rs_batch_write_cqi_epochs_device(rs_batch* b, int32_t first_epoch, int32_t n, const uint8_t* d_cqi, size_t d_bytes, uint32_t flags);
/* waits for the batch's stream; RS_OK with *bad_byte = -1 when no pack since the last report met a value outside 1..15, else
 * RS_ERR_INVALID with the lowest such byte's index in its call's d_cqi and its value; the report clears the record and leaves the
 * batch without a CQI source, like a failing synchronous call */
int rs_batch_cqi_write_status(rs_batch* b, int64_t* bad_byte, int32_t* bad_value);
/* one grid exactly as stored, for the tests: `bytes` must be the image's round_up(Upad * R, 16), Upad = 8 * odd >= U; [R][Upad],
 * zeros in the padding and the tail */
int rs_batch_debug_cqi_image(rs_batch* b, int32_t cell, int32_t epoch, uint8_t* h_image, size_t bytes);
/* CQI source C: the reference's trace replay.  h_trace = [n_traces][n_rows][R]; user u of cell c
 * replays trace h_user_trace[c*U+u]; refresh rule and row index exactly as
 * cqi-manager.cpp:105-123 / enb-mac-entity.cc:189-191 ((int)(Now*1000/40) % row_modulus). */
int rs_batch_set_trace(rs_batch* b, const uint8_t* h_trace, int32_t n_traces, int32_t n_rows,
                       int32_t row_modulus, const int32_t* h_user_trace /* [n_cells][U] */);

/* CQI source C, per PRB: h_trace_prb = [n_traces][n_rows][R*rbg_size] (rs_trace_read_ue_log's out_prb rows); same replay rule */
int rs_batch_set_trace_prb(rs_batch* b, const uint8_t* h_trace_prb, int32_t n_traces, int32_t n_rows, int32_t row_modulus,
                           const int32_t* h_user_trace /* [n_cells][U] */);

/* ---- the reference's CQI trace files (host side of source C; no GPU involved) ----------------------
 * mapping<i>.config: lines "<user id> <trace id>"; user u replays trace map[u % n_entries]
 *   (ref: src/protocolStack/mac/enb-mac-entity.cc:47-53 and :171).  Returns the number of entries read
 *   (at most max_entries are stored), or a negative RS_ERR_*.
 * ue<trace id>.log: one text line per 40-TTI report, nb_rbs space-separated CQI values per line taken from the
 *   start of the line (ref: :173-186, MAX_TTI_TRACE = 475 lines).  rs_trace_read_ue_log parses the first n_rows
 *   lines; out_prb (optional) = [n_rows][nb_rbs]; out_rbg (optional) = [n_rows][nb_rbs/rbg_size], the value of the
 *   first PRB of every RBG -- what the metric reads (downlink-transport-scheduler.cpp:536).  Returns the number of
 *   RBGs whose PRBs do NOT all carry the same value (0 for the shipped traces: then the RBG-granular replay of
 *   rs_batch_set_trace is exact, otherwise use the per-PRB drop-in path), or a negative RS_ERR_*.
 *   A line with fewer than nb_rbs values repeats the last value read, like the reference's extraction loop.
 * rs_trace_load_dir reads ue0.log .. ue<n_traces-1>.log of one directory into out_rbg =
 *   [n_traces][n_rows][nb_rbs/rbg_size] (the h_trace argument of rs_batch_set_trace); same return value. */
/* LDS bytes one cell occupies (the kernel's carve for this shape; no GPU needed).  160 KB per CU: <= 40 960 B keeps four
 * cells on a CU, <= 81 920 B two. */
int rs_lds_bytes_per_cell(int n_slices, int n_users, int n_rbgs, int sched, int threads);

/* measurement helper: streaming copy of `bytes` (16 B per lane), `iters` launches timed with HIP events;
 * *copy_gbs = (bytes read + bytes written) / time.  Quoted by bench.py next to the 8 TB/s HBM3E spec. */
int rs_hbm_copy_probe(int device, uint64_t bytes, int iters, double* copy_gbs);

int rs_trace_read_mapping(const char* path, int32_t* trace_of_entry, int32_t max_entries);
int rs_trace_read_ue_log(const char* path, int32_t n_rows, int32_t nb_rbs, int32_t rbg_size, uint8_t* out_rbg,
                         uint8_t* out_prb);
int rs_trace_load_dir(const char* dir, int32_t n_traces, int32_t n_rows, int32_t nb_rbs, int32_t rbg_size,
                      uint8_t* out_rbg);

/* ------------------------------------------------------------------------------------------
 * Finite queues in a batch: what customised slices (algo_alpha = 1) and rate-limited traffic need.
 * Replaces, per cell: the bearers' MAC queues and RLC dequeue (ref: src/flows/MacQueue.cpp:86-200,
 * src/protocolStack/rlc/um-rlc-entity.cpp:126-196), HasPackets / GetQueueSize / GetHeadOfLinePacketDelay
 * (src/flows/radio-bearer.cpp:263-367), SelectFlowsToSchedule + InsertFlowToUser (downlink-transport-scheduler.cpp:105-150,
 * packet-scheduler.cpp:305-335: users without queued data are not scheduled, slice_priority_, dataToTransmit) and
 * DoStopSchedule's split of a grant over the user's bearers from the highest priority down (:170-221).
 * Schedulers 8, 9, 101, 103 and, RBG by RBG on one wave because their gates bind with finite queues, 7 (a user leaves the race
 * once its PRBs reach m_requiredRBs, downlink-nvs-scheduler.cpp:299-300 with packet-scheduler.cpp:319-334) and 1 (every bearer
 * with packets is a flow with its own PF average; a flow leaves once the transport block of its PRBs so far carries its queue,
 * downlink-packet-scheduler.cpp:221-265; rbg_to_user then holds flow ids 2 * user + bearer and DoStopSchedule credits whole
 * transport blocks, dl-pf-packet-scheduler.cpp:60-125).  The applications themselves stay outside: the caller hands in every
 * bearer's arrival bursts.
 * Restriction: a batch's band is exactly n_rbgs * rbg_size PRBs.  The reference's wideband CQI behind m_requiredRBs
 * (packet-scheduler.cpp:321-327) runs over cqiFeedbacks.size() = every PRB of the band, including the nb_rbs % rbg_size
 * trailing PRBs that are never allocated (25 PRBs with RBGs of 2, 50 with 3, 75 with 4); a batch has no such PRBs, so scheduler 7
 * with queues matches the reference on bands whose PRB count is a multiple of the RBG size -- every shipped configuration
 * (100 MHz: 512 PRBs in RBGs of 8; the trace grid).
 * Round 3: a launch keeps the bearers' hot words in LDS (156 B per user) when the cell still fits the CU's 160 KB, else in HBM.
 * ------------------------------------------------------------------------------------------ */
/* bearer_kind [U][2], index = bearer priority (RadioBearer::GetPriority, radio-bearer.cpp:88-97): 0 none, 1 InfiniteBuffer
 * (always has packets, dataToTransmit 1e8), 2 finite MAC queue.  Every user needs at least one bearer.  Before the first run. */
int rs_batch_set_bearers(rs_batch* b, const uint8_t* bearer_kind);
/* arrival bursts of every finite-queue bearer: bearer (cell c, user u, priority k) owns bursts offsets[(c*U+u)*2+k] ..
 * offsets[(c*U+u)*2+k+1] of the three arrays (ascending in time).  At time[i] the application enqueues n_full[i] packets of
 * 1495 bytes (MAXMTUSIZE 1490 + UDP 8 + IP 20, ROHC 28 -> 3, + PDCP 2) and then, if last_bytes[i] > 0, one of last_bytes[i]
 * bytes; a burst is visible to the TTI whose time stamp is >= time[i]. */
int rs_batch_set_arrivals(rs_batch* b, const int64_t* offsets, const double* time, const int32_t* n_full, const int32_t* last_bytes);
/* per bearer, [n_cells][U][2]: PF average, cumulative bytes / RBs (the `cumu_bytes:` / `cumu_rbs:` of the bearer's log lines),
 * MAC queue bytes and packets; any pointer may be NULL */
int rs_batch_read_bearer_state(rs_batch* b, double* avg_rate, int64_t* cum_bytes, int64_t* cum_rbs, int32_t* queue_bytes,
                               int32_t* queue_packets);
/* host-side generator (no GPU): the arrival bursts of one InternetFlow application (ref: src/flows/application/
 * InternetFlow.cpp: exponential inter-arrival times rounded up to ms, heavy-tailed flow sizes, 1490-byte packets) between
 * start_time and stop_time; flow sizes from a libc-compatible rand() stream seeded with size_seed.  Returns the number of
 * bursts written (<= max_bursts) or a negative RS_ERR_*. */
int rs_internet_flow_arrivals(double rate_mbps, double start_time, double stop_time, uint32_t size_seed, int32_t max_bursts,
                              double* time, int32_t* n_full, int32_t* last_bytes);
/* The flow completion record (ABI 11 addition): one entry per arrival burst, in the order of rs_batch_set_arrivals' arrays (a burst is
 * one InternetFlow flow, InternetFlow::Send).  done_tti = the scheduled TTI, counted from the batch's first, whose DoStopSchedule sent
 * the burst's last packet (whole or as its last fragment: um-rlc-entity.cpp:143-160, "ipflow end"); done_time = that TTI's clock value
 * (the flow's completion time is done_time - time[i]); -1 in both while the flow is not complete.  rs_batch_set_arrivals resets it;
 * every launch of the queue model writes it (one store per completed flow).  It is output, not state: a checkpoint does not carry it
 * (rs_batch_checkpoint_bytes is unchanged), so a resumed batch records the flows that complete after the resume.  The self-check's
 * trial launches leave it as it was.  Either pointer may be NULL; RS_ERR_STATE without the queue model's arrivals. */
int rs_batch_flow_record(rs_batch* b, int32_t* done_tti, double* done_time);

/* run n_ttis scheduled TTIs of every cell in ONE kernel launch on the batch's stream and wait */
int rs_batch_run(rs_batch* b, int32_t n_ttis);
/* same, not waiting (for overlap and hipEvent timing by the caller) */
int rs_batch_run_async(rs_batch* b, int32_t n_ttis);
int rs_batch_sync(rs_batch* b);
/* same as rs_batch_run, also returning the per-TTI decisions of every cell (parity tests, log writer):
 * h_rbg_to_user [n_cells][n_ttis][R] (int16, -1 = none), h_tbs_bits [n_cells][n_ttis][U] (int32),
 * h_quota / h_target [n_cells][n_ttis][S] (int16), h_uinfo [n_cells][n_ttis][U] (int32:
 * nPRB | final_cqi << 16 | mcs << 24, 0 = not scheduled); any may be NULL */
int rs_batch_run_logged(rs_batch* b, int32_t n_ttis, int16_t* h_rbg_to_user, int32_t* h_tbs_bits,
                        int16_t* h_quota, int16_t* h_target, int32_t* h_uinfo);
/* the same with every log optional in one struct, plus what the inter-slice step reads (parity tests pin
 * GreedyByRow / MaximizeCell / Vogel on the device's own per-TTI inputs with it) */
typedef struct rs_batch_log {
  int16_t* rbg_to_user;  /* [n_cells][n_ttis][R] */
  int32_t* tbs_bits;     /* [n_cells][n_ttis][U] */
  int16_t* quota;        /* [n_cells][n_ttis][S] */
  int16_t* target;       /* [n_cells][n_ttis][S] */
  int32_t* uinfo;        /* [n_cells][n_ttis][U] */
  uint32_t* slice_keys;  /* [n_cells][n_ttis][R][S], RS_SCHED_SEQUENTIAL / MAXCELL / UPPERBOUND / SUBOPT / VOGEL only:
                            CQI of the slice's best user on the RBG (0: the slice has no user) | (user id + 1) << 8, i.e.
                            flow_spectraleff / user_index of ref :545-567 */
} rs_batch_log;
int rs_batch_run_logged_ex(rs_batch* b, int32_t n_ttis, const rs_batch_log* log);
/* The same with the queue model's per-bearer rows (ABI 11 addition; RS_ERR_STATE without rs_batch_set_bearers).  Both arrays are
 * [n_cells][n_ttis][U][2] (index = bearer priority), row = the TTI whose DoStopSchedule credited the bytes
 * (downlink-transport-scheduler.cpp:179-199, dl-pf-packet-scheduler.cpp:77-96): bytes = what UpdateTransmittedBytes added (0: the
 * bearer sent nothing, no log line), hol_delay = RadioBearer::GetHeadOfLinePacketDelay at that moment, before the RLC dequeue: 0 for
 * an empty MAC queue or an InfiniteBuffer bearer, else the TTI's clock - the head packet's time stamp, at least 1e-5 (the value the
 * customised slice's metric used in that TTI).  Either pointer may be NULL; `bearers` may be NULL (= rs_batch_run_logged_ex). */
typedef struct rs_batch_bearer_log {
  int32_t* bytes;        /* [n_cells][n_ttis][U][2] */
  double* hol_delay;     /* [n_cells][n_ttis][U][2] */
} rs_batch_bearer_log;
int rs_batch_run_logged_bearers(rs_batch* b, int32_t n_ttis, const rs_batch_log* log, const rs_batch_bearer_log* bearers);
/* Bearer records (ABI 11 addition): the same per-bearer lines from an UNLOGGED launch.  The thread that credits a bearer in
 * DoStopSchedule writes one 32-byte record for it; nothing dense is written, no other log row is needed, and the launch takes the
 * kernel rs_batch_run would take (the lean build included).
 *
 * rs_batch_record_bound is the most records one cell can get in one TTI (> 0): a credit needs a grant and a grant an RBG, so
 * min(2 n_users, n_rbgs) for RS_SCHED_PF (an RBG goes to one flow) and 2 * min(n_users, n_rbgs) for the transport schedulers and NVS
 * (an RBG goes to one user, a user has two bearers).  RS_ERR_STATE without the queue model.
 *
 * rs_batch_run_records IS rs_batch_run(b, n_ttis) -- same kernel choice, and the same state, bearer state, clock, flow record,
 * checkpoint and jit status afterwards -- and in addition n_recs[c] = the bearers credited in cell c during these n_ttis, and
 * recs[c * cap + 0 .. n_recs[c]-1] one record each, ascending in tti, then in user, then in the reference's loop order over the user's
 * bearers (1 before 0 for the transport schedulers and NVS, 0 before 1 for RS_SCHED_PF): the order of the log's counter lines.
 * Records are output, not state: no checkpoint carries them, the self-check's trial launches write none, and no other run call does.
 * Refused before anything is launched, the batch does not move: RS_ERR_INVALID for a null argument, cap < 1, n_ttis < 1 or
 * n_ttis > 32768 (as for logged runs); RS_ERR_STATE without rs_batch_set_bearers / rs_batch_set_arrivals; RS_ERR_HIP when the device
 * block cannot be allocated.  Overflow -- a cell counts more than cap: nothing is written at or behind the capacity, n_recs[c] carries
 * the count as counted, the launch completes (state, flow record and the other cells' lists are complete) and the call returns
 * RS_ERR_RANGE naming the first such cell.  cap = n_ttis * rs_batch_record_bound(b) can never overflow.
 * The device block holds min(cap, n_ttis * bound) places per cell, grows with the largest call so far and is freed with the batch; after
 * an RS_ERR_HIP refusal the batch has none, and the next call allocates again.  RS_RECORDS_MAX_BYTES in the environment caps the
 * block's size: a call that needs more is refused the same way. */
typedef struct rs_bearer_record { /* 32 bytes */
  int32_t tti;       /* the scheduled TTI whose DoStopSchedule credited the bearer, counted from the batch's first
                        (the numbering of rs_batch_flow_record's done_tti): launches concatenate */
  int32_t user;      /* user id 0..U-1 */
  int32_t bearer;    /* bearer priority, 0 or 1 */
  int32_t bytes;     /* what UpdateTransmittedBytes added; never 0 */
  int32_t nprb;      /* what UpdateCumulateRBs added: the user's PRBs (schedulers 7, 8, 9, 101, 103; the same count for both
                        bearers of a split grant), the flow's own PRBs (scheduler 1) */
  int32_t reserved;  /* 0 */
  double hol_delay;  /* GetHeadOfLinePacketDelay before the dequeue: bit for bit rs_batch_bearer_log.hol_delay's value */
} rs_bearer_record;
int rs_batch_record_bound(rs_batch* b);
int rs_batch_run_records(rs_batch* b, int32_t n_ttis, int64_t cap, rs_bearer_record* recs /* [n_cells][cap] */, int64_t* n_recs /* [n_cells] */);
/* Grant records (ABI 11 addition): the app: lines of a BACKLOGGED batch (no queue model) from an unlogged launch.  The lane that works
 * out a served user's transport block writes one 32-byte record for it; no dense row is written, and the launch takes the build
 * rs_batch_run would take -- general, lean or streamed -- in its records variant (a run-time build of its own, compiled at the first
 * records launch that needs it and self-checked with records on; the general build's variant, then the built-in kernels, are the
 * fallbacks).
 *
 * rs_batch_grant_bound is the most records one cell can get in one TTI: min(n_users, n_rbgs) for schedulers 1, 7, 8, 9, 101 and 103; for
 * RS_SCHED_UPPERBOUND, whose slices take their RBGs whatever the other slices take, the sum over the config's slices of
 * min(the slice's users, n_rbgs), as rs_group_grant_bound has it.  RS_ERR_STATE on a batch with the queue model (rs_batch_record_bound
 * is its bound), RS_ERR_INVALID for RS_SCHED_NVS_NONGREEDY.
 *
 * rs_batch_run_grant_records IS rs_batch_run(b, n_ttis) -- the same state, clock, checkpoint bytes and jit status afterwards -- and in
 * addition n_recs[c] = the (TTI, user) pairs of cell c that DoStopSchedule credits bytes > 0 in these n_ttis, and
 * recs[c * cap + 0 .. n_recs[c]-1] one record each, ascending in tti, then in user: DoStopSchedule's walk, the order of the log's lines.
 * Records are output, not state: no checkpoint carries them, and the self-check's and the autotune's trial launches write none into the
 * caller's lists.  RS_SCHED_UPPERBOUND: rbg_mask holds the RBGs of the user's slice's list that went to it; two records of one TTI may
 * share a bit.
 * Refused before anything is launched, the batch does not move: RS_ERR_INVALID for a null argument, cap < 1, n_ttis < 1 or
 * n_ttis > 32768, and for RS_SCHED_NVS_NONGREEDY (its kernel is another one); RS_ERR_STATE on a batch with the queue model
 * (rs_batch_run_records is its call); RS_ERR_HIP when the device block cannot be had (RS_RECORDS_MAX_BYTES caps it, as above).
 * Overflow -- a cell counts more than cap: nothing is written at or behind the capacity, n_recs[c] carries the count as counted, the
 * launch completes and the call returns RS_ERR_RANGE naming the first such cell.  cap = n_ttis * rs_batch_grant_bound(b) never
 * overflows.  The device block holds min(cap, n_ttis * bound) places per cell; it is the block rs_batch_run_records uses (a batch is
 * queue-model or not, and both records are 32 bytes).
 * rs_batch_jit_status: -2 also once the general build's records variant disagreed with the built-in kernels in its self-check (the
 * message names cell, record index and field); the built-in kernels then serve the records launches, every other launch keeps its build. */
typedef struct rs_batch_grant_record { /* 32 bytes, two 16-byte halves */
  int32_t  tti;       /* scheduled TTI, counted from the batch's first (rs_batch_ttis_done's numbering): launches concatenate */
  int32_t  user;      /* user id 0..U-1 */
  int32_t  tbs_bits;  /* what rs_batch_log.tbs_bits holds for (tti, user) */
  int32_t  bytes;     /* min(tbs_bits / 8, 100000000): what DoStopSchedule credits; never 0 */
  uint64_t rbg_mask;  /* bit r: RBG r is among the user's allocated RBGs of this TTI */
  int32_t  nprb;      /* uinfo & 0xffff */
  uint8_t  final_cqi, mcs; /* uinfo >> 16 & 0xff, uinfo >> 24 */
  uint16_t reserved;  /* 0 */
} rs_batch_grant_record;
int rs_batch_grant_bound(rs_batch* b);
int rs_batch_run_grant_records(rs_batch* b, int32_t n_ttis, int64_t cap, rs_batch_grant_record* recs /* [n_cells][cap] */, int64_t* n_recs /* [n_cells] */);
/* `launches` back-to-back launches of n_ttis each, timed with HIP events on the batch's stream;
 * ms_per_launch[launches] receives each launch's duration */
int rs_batch_run_timed(rs_batch* b, int32_t n_ttis, int32_t launches, float* ms_per_launch);

/* per-bearer state after the runs so far; any pointer may be NULL.
 * avg_rate [n_cells][U], cum_bytes/cum_rbs [n_cells][U] (RadioBearer::GetCumulateBytes/RBs),
 * slice_state [n_cells][S] (slice_rbs_offset_, or slice_ewma_time_ for NVS) */
int rs_batch_read_state(rs_batch* b, double* avg_rate, int64_t* cum_bytes, int64_t* cum_rbs,
                        double* slice_state);
/* An initialisation / test hook, NOT a checkpoint: sets avg_rate [n_cells][U] (every value >= 1, the EWMA's clamp) and
 * slice_state [n_cells][S]; either may be NULL = left alone.  It does not touch the rest of a cell's state -- the grant of the last
 * TTI that the next EWMA update consumes, the clock, the rand() ring, the cumulative counters -- so it is exact before the first
 * launch (or on a batch whose last grant was zero); after a launch the pending grant is applied on top of the new averages.  Not
 * with the queue model (one average per bearer there).  slice_state: every cell's values lie in the domain stated at
 * rs_set_slice_offset, else RS_ERR_INVALID and nothing is written.  (ABI 9) */
int rs_batch_write_state(rs_batch* b, const double* avg_rate, const double* slice_state);
/* Checkpoint / resume (ABI 10).  A checkpoint is everything a batch carries from one launch to the next -- PF averages, the grants
 * the next EWMA update consumes, cumulative counters, slice state, every cell's clock, rand() ring and CQI-report state, the number of
 * TTIs done, and with the queue model the bearers' queues, averages and counters -- as one host block of rs_batch_checkpoint_bytes
 * bytes.  rs_batch_checkpoint_load puts it into a batch of the same shape (slices, UEs, RBGs, PRBs per RBG, scheduler, cells, queue
 * model or not; jit, threads_per_cell, device and process may differ), which then continues bit for bit like the batch that saved
 * it: run 300 TTIs, save, run 300 more == load into a new batch, run 300.  The CQI source (epoch grids, trace tables, arrival bursts) is
 * configuration, not state: set it on the resuming batch as on the first one (rs_batch_seed need not be called: the ring is in the
 * block).  Between launches only.  rs_batch_read_state / rs_batch_write_state remain the partial accessors they were. */
int64_t rs_batch_checkpoint_bytes(rs_batch* b);
int rs_batch_checkpoint_save(rs_batch* b, void* buf, size_t buflen);
int rs_batch_checkpoint_load(rs_batch* b, const void* buf, size_t buflen);
/* the simulated clock of every cell (ref: src/core/eventScheduler/simulator.cc:117-126): t [n_cells] = time stamp of the next
 * TTI, last_update [n_cells] = RadioBearer::m_lastUpdate; either may be NULL */
int rs_batch_read_clock(rs_batch* b, double* t, double* last_update);
/* 1: the shape-specialised (hiprtc) kernel is in use (msg is empty, says that the untuned variant had to be built, or reports a
 * passed rs_batch_config.selfcheck); 0: it was not asked for; -1: it was asked for and could not be built -- the built-in kernels
 * run instead and msg receives the reason; -2: it was built and rs_batch_config.selfcheck found its results different from the
 * built-in kernels': dropped, the built-in kernels run */
int rs_batch_jit_status(rs_batch* b, char* msg, size_t msglen);
/* what rs_batch_config.autotune measured: one line "variant: ms" per candidate and the one kept; empty before the tuning ran or
 * when it does not apply.  Returns the number of candidates timed (0: none). */
int rs_batch_autotune_report(rs_batch* b, char* msg, size_t msglen);
/* Optional: build now whatever kernel an unlogged rs_batch_run of n_ttis TTIs would otherwise build at its first launch (the lean
 * build of the shape-specialised kernel, see rs_batch_config.jit), so that no timed launch carries a hiprtc run.  Call it once the
 * CQI source is set.  RS_OK also when there is nothing to build. */
int rs_batch_prepare_launch(rs_batch* b, int32_t n_ttis);
/* per-slice cumulative bytes summed over the batch's cells, reduced on the device into
 * d_out[S] (device pointer, uint64) on the batch's stream -- the vector the multi-GPU run
 * all-reduces over RCCL (the reference's plot_throughput.py:26-56 sums it per slice post hoc) */
int rs_batch_slice_bytes_device(rs_batch* b, uint64_t* d_out);
int rs_batch_slice_bytes(rs_batch* b, uint64_t* h_out /* [S] */);
/* build check (needs no GPU): compile the shape-specialised kernel for one shape with hiprtc; returns the
 * code object size or a negative value with the compiler log in err */
int rs_jit_selfcheck(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err,
                     size_t errlen);
/* the same without the internal -mllvm tuning options: the build the library falls back to (and reports through
 * rs_batch_jit_status: return value 1 with a non-empty message) when hiprtc refuses them */
int rs_jit_selfcheck_untuned(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err,
                             size_t errlen);
/* the same for the queue-model kernel (the code object rs_batch_set_bearers switches a batch to; schedulers 1, 7, 8, 9, 101, 103) */
int rs_jit_selfcheck_queue(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, char* err,
                           size_t errlen);
/* the records variant (rs_batch_run_grant_records) of the batch kernel of this shape: lean = 0 the general build, 1 the lean build.
 * A negative value with the reason in err for RS_SCHED_NVS_NONGREEDY. */
int rs_jit_selfcheck_grant_records(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int lean,
                                   char* err, size_t errlen);
/* the batch kernel of this shape with per-cell configuration rows (what rs_batch_set_cell_configs compiles for a batch with jit = 1):
 * lean = 0 the general build, 1 the lean build.  A negative value with the reason in err for RS_SCHED_NVS_NONGREEDY. */
int rs_jit_selfcheck_cell_configs(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int lean, char* err, size_t errlen);
/* the same with rows that end in absent users (what a ragged batch compiles: -DRS_JIT_CELL_CONFIGS=2) */
int rs_jit_selfcheck_ragged_cells(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int lean, char* err, size_t errlen);
/* the same for a batch with a cell of fewer slices than n_slices, absent users included (-DRS_JIT_CELL_CONFIGS=6) */
int rs_jit_selfcheck_ragged_slices(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int lean, char* err, size_t errlen);
/* ---- the run-time compiled kernels' cache on disk (ABI 10) ----
 * Every code object hiprtc produces (rs_batch_create with jit = 1, the lean / streamed variants, rs_ctx_specialize) is kept in
 * $RS_JIT_CACHE_DIR (default $XDG_CACHE_HOME/radiosaber_amd, else ~/.cache/radiosaber_amd; created with mode 0700), one file per (device
 * source hash, compiler identity -- see rs_jit_compiler_identity --, full hiprtc option list); a later process loads it instead of
 * compiling (~2 s per variant -> a few ms).  Files are written under a temporary name and renamed; a file that does not check out
 * (magic, key text, length, checksum), is not a regular file of the caller's own, or is writable by anybody else is compiled again and
 * replaced (RS_JIT_CACHE_SHARED=1 accepts another account's read-only cache).  Its last 8 bytes say whether the object has passed a
 * self-check against the built-in kernels ("VERIFIED"); a build that a self-check rejects is unlinked.  RS_JIT_CACHE=0 switches the
 * cache off.
 * rs_jit_cache_stats: this process's hits, misses (= hiprtc runs), files written, files rejected.
 * rs_jit_cache_file: the file the batch kernel of a shape lives in (flags: 2 = streamed-CQI variant, 4 = lean build); returns its
 *   length, 0 when no cache directory can be named.
 * rs_jit_cache_warm: that kernel THROUGH the cache (compiles and stores on a miss); needs no GPU; code size or -1 with the log. */
void rs_jit_cache_stats(long long out[4]);
/* the compiler identity that is part of every cache key (ABI 11): hiprtc and HIP runtime versions down to the patch level, the clang
 * version string of the compiler inside hiprtc with its LLVM commit (read from a two-line probe compilation), comgr's version.
 * RS_JIT_COMPILER_ID replaces it (deployments that pin the toolchain themselves).  Needs no GPU. */
const char* rs_jit_compiler_identity(void);
int rs_jit_cache_file(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int flags, char* out, size_t outlen);
int rs_jit_cache_warm(int n_slices, int n_users, int n_rbgs, int rbg_size, int threads, int sched, int flags, char* err, size_t errlen);
/* 16 hex digits: FNV-1a hash of the device sources this library was built from (and compiles at run time); measurement
 * records under profiles/ carry it so that a record taken on other kernel code can be told apart (bench.py: "stale") */
const char* rs_device_source_hash(void);
/* diagnostics: how often the std::sort emulation (MaximizeCell, UpperBound) took libstdc++'s heap-sort fallback -- std::__partial_sort,
 * when std::__introsort_loop's depth limit 2 * floor(log2 n) runs out on a range longer than 16 (bits/stl_algo.h:1937-1957; the
 * reference's call: downlink-transport-scheduler.cpp:354-361) -- since the batch / context was created, per device site:
 * [0] workgroup level of the register form, [1] inside a single wave's finish of the last levels, [2] workgroup level of the LDS
 * form (more than four sort records per thread).  Random CQI grids never get there; tests/golden/sort_killers.npz holds grids that
 * do.  out = [n_cells][3] / [3].  (ABI 10) */
int rs_batch_debug_heap_sorts(rs_batch* b, int64_t* out);
int rs_ctx_debug_heap_sorts(rs_ctx* ctx, int64_t* out);
/* diagnostics: the shader clock the LAST launch really ran at, per cell: (s_memtime cycles) / (s_memrealtime ticks at 100 MHz) between
 * the first and the last instruction of the cell's thread 0 -> shader_mhz [n_cells]; kernel_ms [n_cells] = that span in milliseconds
 * (a cell's own run time: cells that waited for a free CU start later).  Either may be NULL.  (ABI 10) */
int rs_batch_debug_clocks(rs_batch* b, double* shader_mhz, double* kernel_ms);
/* diagnostics: cycles per kernel phase of one cell's first thread, summed over the last launch;
 * only in the separate -DRS_STAMPS build (RS_ERR_STATE in the product library) */
int rs_batch_debug_stamps(rs_batch* b, int32_t cell, uint64_t* out20);
/* scheduled TTIs completed per cell so far */
int64_t rs_batch_ttis_done(rs_batch* b);
/* the hipStream_t the batch launches on */
void* rs_batch_stream(rs_batch* b);
/* name of the dominant kernel (for matching rocprofv3 --kernel-trace rows) */
const char* rs_batch_kernel_name(rs_batch* b);

#ifdef __cplusplus
}
#endif
#endif /* RADIOSABER_HIP_H_ */
