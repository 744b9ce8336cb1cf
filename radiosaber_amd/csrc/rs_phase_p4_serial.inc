/* rs_phase_p4_serial.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: the serial end of the TTI on wave 0, first half: the inter-slice policy (rs_interslice.h) or the per-RBG reduction of schedulers 1 / 7, incl. their RBG-by-RBG races with finite queues and gates; leaves `owner` (lane = RBG) and `got` (lane = slice). */
      /* the only running wave of this cell until the end-of-TTI barrier: ask the SIMD's arbiter to prefer it
       * over the co-resident cell's waves (measured +3 % with two cells per CU) */
      RS_SETPRIO(RS_SERIAL_PRIO);
      int owner = -1;
      int got = 0; /* lane s: RBGs granted to slice s */
      int my_target = 0, my_quota = 0; /* lane s: this TTI's values (the quota wave may overwrite the LDS copies for TTI t+1) */
      if (kHoldSched) {
        hold_served[lane] = 0u; /* (m->hist is free: this TTI's lists are consumed, the counting sort is over) */
      }
      if (kEarly17) {
        if (lane == 0) { fl_prev->ctr_p1 = 0; fl_prev->ctr_p3 = 0; fl_prev->greedy_done = 0; fl_prev->n_fix = 0; }
      }
      if (kSpecSched || kHoldSched) {
        my_target = m->target[lane];
        my_quota = m->quota[lane];
        /* the other flag set belongs to the NEXT serial phase: its last reader (this TTI's fix-up) is behind a barrier */
        if (lane == 0) { fl_prev->ctr_p1 = 0; fl_prev->ctr_p3 = 0; fl_prev->greedy_done = 0; fl_prev->n_fix = 0; }
        if (spec_next && lane < 32) served_bits[lane] = 0u;
      }
      if constexpr (kQSerial) {
        /* Schedulers 1 and 7 with finite queues: RBG by RBG, the first maximum among the candidates still in the race --
         * flows whose transport block does not yet carry their queue (downlink-packet-scheduler.cpp:221-265) / users of the
         * served slice below their m_requiredRBs (downlink-nvs-scheduler.cpp:283-308).  Lanes = candidates, 64 at a time;
         * metrics are >= 0, so their bit patterns order like (high word signed, low word unsigned): two DPP max reductions
         * and the lowest lane among the equals; a later chunk only wins with a strictly larger metric. */
        int c_lo = 0, c_hi = 2 * U; /* sched 1: flow ids 2 * user + bearer */
        int sl_eps = 1, sl_psi = 1, sl_custom = 0;
        if (SCHED == 7) {
          c_lo = m->seg_begin[seg_lo];
          c_hi = m->seg_begin[seg_lo + 1];
          sl_eps = m->eps_psi[seg_lo] & 1;
          sl_psi = (m->eps_psi[seg_lo] >> 1) & 1;
          sl_custom = (m->eps_psi[seg_lo] & 4) != 0;
        }
        /* sched 7, served slice of at most 64 users with its metric table in place: lane = user, the user's remaining
         * m_requiredRBs in a register, per RBG two LDS reads (the next RBG's CQI is fetched a step ahead) and the two reductions */
        const bool table7 = SCHED == 7 && c_hi - c_lo <= 64 && (c_hi - c_lo) * 128 <= o.items - o.elems;
        if (table7) {
          const int u = c_lo + lane;
          const bool mine = u < c_hi && (prio_in[u < c_hi ? u : c_lo] & 2) != 0;
          int need = mine ? q_need[u] : 0;
          const double* const row = (const double*)s_elems + lane * 16;
          int cq_next = mine ? (int)s_cqi[u] : 0;
          for (int r = 0; r < R; ++r) {
            const int cq = cq_next;
            if (r + 1 < R && mine) cq_next = s_cqi[(r + 1) * Upad + u];
            const double metric = mine ? row[cq] : 0.0;
            const bool valid = mine && need > 0;
            const int hi = valid ? __double2hiint(metric) : -1;
            const int lo = (int)((unsigned)__double2loint(metric) ^ 0x80000000u);
            const int mhi = wave_max(hi);
            const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
            const int pick = mhi >= 0 ? __ffsll((long long)__ballot(valid && hi == mhi && lo == mlo)) - 1 : -1;
            if (lane == r) owner = pick >= 0 ? c_lo + pick : -1;
            if (lane == pick) need -= G;
          }
        }
        /* sched 1 in a shape-specialised build: every lane keeps its flows (flow id 64 k + lane, k < kFK) in registers -- the
         * stage-1 reciprocal of the flow's average and an "in the race" bit -- and ranks them per RBG with the FP32 product of
         * DESIGN.md 2.6 (one multiply per flow, one wave reduction per RBG); only flows within 2^-19 of the best product can win
         * or tie, so a single survivor is the winner without any division and several are compared exactly, ascending flow id,
         * strict '>' (the reference's scan order, downlink-packet-scheduler.cpp:221-237). */
        constexpr int kFK = FIXED ? (2 * RS_JIT_U + 63) / 64 : 1;
        constexpr bool kFlowRegs = FIXED && SCHED == 1 && kFK <= 16;
        float flow_rc[kFK];
        unsigned flow_alive = 0u;
        if constexpr (kFlowRegs) {
#pragma unroll
          for (int k = 0; k < kFK; ++k) {
            const int f = 64 * k + lane, u = (f >> 1) < U ? (f >> 1) : U - 1;
            const int data = f < 2 * U ? ((f & 1) ? q_data1[u] : q_data0[u]) : 0;
            const double af = (f & 1) ? s_avgk[u] : s_avg[u];
            flow_rc[k] = __builtin_amdgcn_rcpf((float)af);
            if (data > 0) flow_alive |= 1u << k;
          }
        }
        int tbs_cap8 = 0; /* sched 1: floor(largest transport block of the table / 8): more bytes than that are never carried */
        if (SCHED == 1) {
          for (int i = lane; i < (R + 1) * 16; i += 64) tbs_cap8 = s_tbs[i] > tbs_cap8 ? s_tbs[i] : tbs_cap8;
          tbs_cap8 = wave_max(tbs_cap8) >> 3;
        }
        double run_sum = 0.0; /* sched 1, lane r: EESM sum / PRBs of the flow that holds RBG r, up to and including RBG r */
        int run_nprb = 0;
        for (int r = 0; r < R && !table7; ++r) {
          int bhi = -1, blo = (int)0x80000000, bpick = -1;
          if constexpr (kFlowRegs) {
            const float kTolF = 0x1.ffffcp-1f; /* 1 - 2^-19 */
            int cqv[kFK];
            float av[kFK];
            float best_a = 0.0f;
#pragma unroll
            for (int k = 0; k < kFK; ++k) {
              const int f = 64 * k + lane, u = (f >> 1) < U ? (f >> 1) : U - 1;
              cqv[k] = s_cqi[r * Upad + u];
            }
#pragma unroll
            for (int k = 0; k < kFK; ++k) {
              av[k] = ((flow_alive >> k) & 1u) ? s_num32[cqv[k]] * flow_rc[k] : 0.0f;
              best_a = fmaxf(best_a, av[k]);
            }
            const float mx = __int_as_float(wave_max(__float_as_int(best_a))); /* products are >= 0: they order like their bits */
            if (mx > 0.0f) {
              const float thr = mx * kTolF;
              unsigned cm = 0u;
#pragma unroll
              for (int k = 0; k < kFK; ++k) cm |= av[k] >= thr ? (1u << k) : 0u; /* thr > 0: a survivor is in the race */
              const unsigned long long holders = __ballot(cm != 0u);
              if (__popcll(holders) == 1) {
                const int src = __ffsll((long long)holders) - 1;
                const unsigned cmw = (unsigned)__builtin_amdgcn_readlane((int)cm, src);
                if ((cmw & (cmw - 1u)) == 0u) bpick = 64 * (__ffs((int)cmw) - 1) + src;
              }
              if (bpick < 0) {
                /* several flows within the tolerance (flows that were never served share one average): compared exactly, chunk
                 * by chunk in ascending flow id, strict '>' (three reductions over per-lane bests measured slower: 63.1 against
                 * 60.8 us per TTI) */
#pragma unroll
                for (int k = 0; k < kFK; ++k) {
                  if (__ballot((cm >> k) & 1u) == 0ull) continue;
                  const int f = 64 * k + lane, u = (f >> 1) < U ? (f >> 1) : U - 1;
                  bool valid = ((cm >> k) & 1u) != 0u;
                  const double metric = s_num[cqv[k]] / ((f & 1) ? s_avgk[u] : s_avg[u]); /* (se * 180000.) / the flow's own average */
                  valid = valid && metric > 0; /* the scan starts from 0 with '>' */
                  const int hi = valid ? __double2hiint(metric) : -1;
                  const int lo = (int)((unsigned)__double2loint(metric) ^ 0x80000000u);
                  const int mhi = wave_max(hi);
                  const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
                  if (mhi >= 0 && (mhi > bhi || (mhi == bhi && mlo > blo))) {
                    bhi = mhi;
                    blo = mlo;
                    bpick = 64 * k + __ffsll((long long)__ballot(valid && hi == mhi && lo == mlo)) - 1;
                  }
                }
              }
            }
          }
          for (int c0 = c_lo; c0 < c_hi && !kFlowRegs; c0 += 64) {
            const int cnd = c0 + lane;
            const int u = SCHED == 1 ? cnd >> 1 : cnd;
            bool valid = cnd < c_hi;
            double metric = 0.0;
            if (valid) {
              const int cq = s_cqi[r * Upad + u];
              if (SCHED == 1) {
                const int data = (cnd & 1) ? q_data1[u] : q_data0[u];
                valid = data > 0 && q_done[cnd] == 0;
                metric = s_num[cq] / ((cnd & 1) ? s_avgk[u] : s_avg[u]); /* (se * 180000.) / the flow's own average */
                valid = valid && metric > 0; /* the scan starts from 0 with '>' */
              } else {
                valid = (prio_in[u] & 2) != 0 && q_need[u] > 0;
                const double num = sl_eps ? s_num[cq] : 1.0, den = sl_psi ? s_avgk[u] : 1.0;
                if (!sl_custom) metric = num / den;
                else metric = (prio_in[u] & 1) == 0 ? 0.0 : hol_in[u] * num / den; /* ref: nvs :375-387 */
              }
            }
            const int hi = valid ? __double2hiint(metric) : -1;
            const int lo = (int)((unsigned)__double2loint(metric) ^ 0x80000000u);
            const int mhi = wave_max(hi);
            const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
            if (mhi >= 0 && (mhi > bhi || (mhi == bhi && mlo > blo))) {
              bhi = mhi;
              blo = mlo;
              bpick = c0 + __ffsll((long long)__ballot(valid && hi == mhi && lo == mlo)) - 1;
            }
          }
          if (lane == r) owner = bpick;
          if (bpick >= 0) {
            if (SCHED == 7) {
              if (lane == 0) q_need[bpick] -= G;
            } else {
              /* the flow's transport block so far (its PRBs in RBG order): satisfied once it carries the whole queue.  The new
               * RBG is the flow's last, so the EESM sum continues where the lane of the flow's previous RBG left it (the same
               * additions in the same order as summing all of them again) */
              /* (a flow with more data than the largest transport block of the table -- every InfiniteBuffer flow -- is never
               * satisfied: no sum to keep) */
              const int data_pick = (bpick & 1) ? q_data1[bpick >> 1] : q_data0[bpick >> 1];
              if (data_pick <= tbs_cap8) {
              const unsigned long long before = __ballot(owner == bpick && lane < r);
              const int prev = before != 0ull ? 63 - __clzll((long long)before) : 0;
              const double psum = __shfl(run_sum, prev, 64);
              const int pn = __builtin_amdgcn_readlane(run_nprb, prev);
              if (lane == r) {
                const int u = bpick >> 1;
                double sum = before != 0ull ? psum : 0.0;
                int nprb = before != 0ull ? pn : 0;
                if (per_prb) { /* the flow's per-PRB feedback (ref: downlink-packet-scheduler.cpp:245-264) */
                  const uint8_t* pr = prb_ptr(u, r);
                  for (int k = 0; k < G; ++k) sum += s_e[pr[k]];
                } else {
                  const double ev = s_e[s_cqi[r * Upad + u]];
                  for (int k = 0; k < G; ++k) sum += ev;
                }
                nprb += G;
                run_sum = sum;
                run_nprb = nprb;
                const double x = sum / (double)nprb;
                int fq = 15;
                if (!(x == 0)) {
                  fq = 1;
#pragma unroll
                  for (int k = 1; k <= 13; ++k) fq += (x <= xthr_k[k - 1]) ? 1 : 0;
                }
                if (s_tbs[(nprb / G) * 16 + fq] >= data_pick * 8) q_done[bpick] = 1;
              }
              }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if constexpr (kFlowRegs) { /* a satisfied flow leaves the race: its lane clears the bit */
              if (q_done[bpick] != 0 && lane == (bpick & 63)) flow_alive &= ~(1u << (bpick >> 6));
            }
          }
        }
      } else if (DIRECT && (SCHED == 1 || SCHED == 7) && p.gate != nullptr) {
        /* Drop-in mode with finite queues (rs_tti_in.data_to_transmit / required_rbs): the same RBG-by-RBG race as above on the
         * caller's candidates -- flows (sched 1: every passed "user" is one flow) / the served slice's users (sched 7).  The
         * caller's averages and delays are arbitrary doubles, so sched 7's metrics may be negative, -0.0, infinite or NaN: the race
         * starts from lowest() with a strict '>' (downlink-nvs-scheduler.cpp:294-300: a negative metric wins when nobody better is
         * eligible, a NaN or -inf never does) and the lanes compare through double_order_key. */
        for (int u = lane; u < U; u += 64) {
          q_need[u] = p.gate[u];
          q_done[u] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int sl7 = (int)p.user_slice[0];
        const int sl_eps = SCHED == 7 ? (m->eps_psi[sl7] & 1) : 1, sl_psi = SCHED == 7 ? ((m->eps_psi[sl7] >> 1) & 1) : 1;
        const bool custom7 = SCHED == 7 && queue_mode_in && p.alpha[sl7] != 0;
        for (int r = 0; r < R; ++r) {
          int bhi = (int)0x80000000, blo = (int)0x80000000, bpick = -1;
          for (int c0 = 0; c0 < U; c0 += 64) {
            const int u = c0 + lane;
            bool valid = u < U;
            double metric = 0.0;
            if (valid) {
              const int cq = s_cqi[r * Upad + u];
              if (SCHED == 1) {
                valid = q_done[u] == 0;
                metric = s_num[cq] / s_avg[u];
                valid = valid && metric > 0;
              } else {
                valid = q_need[u] > 0;
                const double num = p.gen_exp ? p.gen_num[sl7 * 16 + cq] : (sl_eps ? s_num[cq] : 1.0);
                const double den = p.gen_exp ? s_avgk[u] : (sl_psi ? s_avgk[u] : 1.0);
                if (!custom7) metric = num / den;
                else metric = (prio_in && (prio_in[u] & 1) == 0) ? 0.0 : hol_in[u] * num / den;
                valid = valid && metric > -1.7976931348623157e308; /* the scan starts from lowest() with '>': false for a NaN */
              }
            }
            int hi, lo;
            double_order_key(metric, hi, lo);
            hi = valid ? hi : (int)0x80000000;
            const int mhi = wave_max(hi);
            const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
            if (mhi != (int)0x80000000 && (mhi > bhi || (mhi == bhi && mlo > blo))) {
              bhi = mhi;
              blo = mlo;
              bpick = c0 + __ffsll((long long)__ballot(valid && hi == mhi && lo == mlo)) - 1;
            }
          }
          if (lane == r) owner = bpick;
          if (bpick >= 0) {
            if (SCHED == 7) {
              if (lane == 0) q_need[bpick] -= G;
            } else {
              const unsigned long long mine = __ballot(owner == bpick && lane <= r);
              if (lane == r) {
                unsigned long long mm = mine;
                double sum = 0;
                int nprb = 0;
                while (mm) {
                  const int r2 = __ffsll((long long)mm) - 1;
                  mm &= mm - 1;
                  if (per_prb) {
                    const uint8_t* pr = prb_ptr(bpick, r2);
                    for (int k = 0; k < G; ++k) sum += s_e[pr[k]];
                  } else {
                    const double ev = s_e[s_cqi[r2 * Upad + bpick]];
                    for (int k = 0; k < G; ++k) sum += ev;
                  }
                  nprb += G;
                }
                const double x = sum / (double)nprb;
                int fq = 15;
                if (!(x == 0)) {
                  fq = 1;
#pragma unroll
                  for (int k = 1; k <= 13; ++k) fq += (x <= xthr_k[k - 1]) ? 1 : 0;
                }
                if (s_tbs[(nprb / G) * 16 + fq] >= q_need[bpick] * 8) q_done[bpick] = 1;
              }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        }
      } else if constexpr (SCHED == 8 || SCHED == 9 || SCHED == 101 || SCHED == 103) {
        /* DownlinkTransportScheduler's inter-slice policies (rs_interslice.h): lane r learns the slice of RBG r */
        int my_slice;
        /* (a build for cells of fewer slices: the slice count is the cell's run-time Sn, the mask widths stay the batch's) */
        constexpr int kS = (FIXED && !kRaggedS) ? RS_JIT_S : 0, kR = FIXED ? RS_JIT_R : 0;
        constexpr bool kK32 = (FIXED ? RS_JIT_S : 0) <= 32 && kR <= 32;
        if constexpr (SCHED == 8) my_slice = interslice_greedy_by_row<kS, kR>(cur_rec, m, Sn, R, got);
        else if constexpr (SCHED == 101) my_slice = interslice_subopt<kS, kR>(cur_rec, m, (uint8_t*)(lds + o.sortx), Sn, R, got);
        else if constexpr (SCHED == 103) my_slice = interslice_vogel<kS, kR>(cur_rec, m, Sn, R, got);
        else {
#ifdef RS_STAMPS
#define RS_SCAN_ARGS s_sorted, m, Sn, R, got, stamp_acc
#else
#define RS_SCAN_ARGS s_sorted, m, Sn, R, got
#endif
          if constexpr (kSegScan) {
#ifdef RS_STAMPS
            my_slice = interslice_maximize_cell_segments<kS, kR, kK32>(s_elems, s_sorted, m, Sn, R, got, stamp_acc);
#else
            my_slice = interslice_maximize_cell_segments<kS, kR, kK32>(s_elems, s_sorted, m, Sn, R, got);
#endif
          } else if constexpr (kVecScan) {
            if constexpr (FIXED) {
              my_slice = interslice_maximize_cell_vector<kS, kR, kK32>(RS_SCAN_ARGS);
            } else {
              if (vec_scan && R <= 32 && S <= 32) my_slice = interslice_maximize_cell_vector<0, 0, true>(RS_SCAN_ARGS);
              else if (vec_scan) my_slice = interslice_maximize_cell_vector<0, 0, false>(RS_SCAN_ARGS);
              else my_slice = interslice_maximize_cell<0, 0>(RS_SCAN_ARGS);
            }
          } else {
            my_slice = interslice_maximize_cell<kS, kR>(RS_SCAN_ARGS);
          }
        }
        if (((kSpecSched && spec_next) || quota_next) && !p.phy_draws) {
          /* slice_rbs_offset_ is final as soon as the RBGs are dealt out (ref: :618-620): the quota wave can start TTI t+1's
           * targets while this wave still looks up the winners and adapts the links */
          if (lane < Sn) s_sstate[lane] = (double)(my_target - got * G);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (lane == 0) atomicExch(&fl_cur->greedy_done, 1);
        }
        if (lane < R && my_slice >= 0) {
          int u = cur_bu[my_slice * R + lane];
          owner = u == 0xFFFF ? -1 : u;
        }
      } else if (SCHED == 1 && kPf1) {
        /* the waves settled every RBG in P3 (one wave per RBG over all users): the winner table is the allocation */
        if (lane < R) {
          const int u = cur_bu[lane];
          owner = u == 0xFFFF ? -1 : u;
        }
      } else if (SCHED == 1) {
        /* ref: downlink-packet-scheduler.cpp:221-237 -- per RBG the first maximum over all flows,
         * here over the segment winners in ascending segment order */
        if (lane < R) {
          double best = 0.0;
          int sg = 0;
          for (; sg + 4 <= o.n_seg; sg += 4) { /* four segments per step: the eight LDS reads first */
            double v[4];
            int u[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] = s_best_metric[(sg + q) * R + lane]; u[q] = s_best_user[(sg + q) * R + lane]; }
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (u[q] != 0xFFFF && v[q] > best) { best = v[q]; owner = u[q]; }
          }
          for (; sg < o.n_seg; ++sg) {
            double v = s_best_metric[sg * R + lane];
            int u = s_best_user[sg * R + lane];
            if (u != 0xFFFF && v > best) { best = v; owner = u; }
          }
        }
      } else if (SCHED == 7 && (FIXED ? kCv.nvs_seg : p.nvs_seg) != 0) {
        /* ref: downlink-nvs-scheduler.cpp:283-297 -- per RBG the first maximum from lowest(), over the run winners in
         * ascending run order */
        if (lane < R) {
          double best = -1.7976931348623157e308;
          bool none = true;
          for (int sg = 0; sg < nvs_runs; ++sg) {
            const double v = s_best_metric[sg * R + lane];
            const int u = s_best_user[sg * R + lane];
            if (u != 0xFFFF && (none || v > best)) { best = v; owner = u; none = false; }
          }
        }
      } else {
        if (lane < R) {
          int u = s_best_user[lane];
          owner = u == 0xFFFF ? -1 : u;
        }
      }
      RS_STAMP(5);
      if (kEarly17 && SCHED == 7 && early17) {
        /* the winner tables are in this wave's registers now: the scanning waves may overwrite them with TTI t+1's */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) atomicExch(&fl_cur->greedy_done, 1);
      }

