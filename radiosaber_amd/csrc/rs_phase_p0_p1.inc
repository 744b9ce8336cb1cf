/* rs_phase_p0_p1.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: P0 CQI refresh (epoch grids / trace rows -> the RBG-major LDS grid) and P1 the PF EWMA of every user (or, queue model, of every bearer + arrivals + the user records); a TTI whose averages were prepared during the previous serial phase only does the owners' byte bookkeeping. */
    /* ---------------- P0: CQI refresh ---------------- */
    bool grid_loaded = false; /* this TTI scans a new CQI grid (held winners: everything is scanned again) */
    if (p.cqi_mode == RS_CQI_EPOCHS) {
      /* a launch that starts inside an epoch loads that epoch's grid first: LDS does not survive between launches */
      if (kDirect || tti == 0 || (epoch_pos == 0 && !grid_ahead)) {
        grid_loaded = true;
        long long e = kDirect ? 0 : epoch;
        if (e >= p.n_epochs) { local_err = RS_CQI_EPOCHS; e = p.n_epochs - 1; }
        const uint4* src = (const uint4*)(p.epochs + ((size_t)cell * p.n_epochs + (size_t)e) * p.grid_stride);
        const int n16 = (int)(p.grid_stride >> 4);
        if (DIRECT && grid_from_image) {
          /* the reports of the call before (rs_tti_in.cqi_epoch): the context's image IS the LDS grid -- 16 bytes per lane, from HBM */
          const int n16i = (R * Upad + 15) >> 4;
          if constexpr (kPrefetch) {
#pragma unroll
            for (int j = 0; j < kPG; ++j)
              if (tid + j * nt < n16i) ((uint4*)s_cqi)[tid + j * nt] = pre_grid[j];
          } else {
            const uint4* img = (const uint4*)p.grid_image;
            for (int i = tid; i < n16i; i += nt) ((uint4*)s_cqi)[i] = img[i];
          }
        } else if constexpr (DIRECT) {
          /* the caller's grid is [U][R] (one row per UE, like the reference's per-UE CQI vectors); LDS keeps it
           * RBG-major [R][Upad] so that the metric scan reads 8 consecutive UEs of one RBG per load */
          const int total = U * R;
          auto scatter16 = [&](int i, const uint4 w) { /* 16 grid bytes [u][r] -> the RBG-major LDS grid */
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
            int idx = i << 4;
            int u = idx / R, r = idx - u * R;
#pragma unroll
            for (int k = 0; k < 16; ++k, ++idx) {
              if (idx < total) s_cqi[r * Upad + u] = (uint8_t)(ww[k >> 2] >> ((k & 3) * 8));
              if (++r == R) { r = 0; ++u; }
            }
          };
          if constexpr (kPrefetch) {
#pragma unroll
            for (int j = 0; j < kPG; ++j)
              if (tid + j * nt < n16) scatter16(tid + j * nt, pre_grid[j]);
          } else {
            for (int i = tid; i < n16; i += nt) scatter16(i, src[i]);
          }
          if (p.image_mode == 1) {
            /* new reports under a cqi_epoch: leave the grid behind for the calls that will see the same reports */
            __syncthreads();
            const int n16i = (R * Upad + 15) >> 4;
            uint4* img = (uint4*)p.grid_image;
            for (int i = tid; i < n16i; i += nt) img[i] = ((const uint4*)s_cqi)[i];
          }
        } else {
          /* a batch's grids live in HBM as the LDS image ([R][Upad], zero padding included; rs_batch_upload_cqi_epochs and the
           * synthesis kernel write them that way): a straight copy, 16 bytes per lane */
          for (int i = tid; i < n16; i += nt) ((uint4*)s_cqi)[i] = src[i];
        }
      } else if (epoch_pos == 0) {
        grid_loaded = true; /* written during the previous TTI's serial phase (kGridAhead) */
      }
    } else if (p.cqi_mode == RS_CQI_TRACE) {
      /* ref: src/device/CqiManager/cqi-manager.cpp:105-123 (interval 40),
       *      src/protocolStack/mac/enb-mac-entity.cc:189-191 */
      bool load = tti == 0 && reported; /* a launch that starts between two reports reloads the last reported row */
      if (!reported || ((int)(t * 1000) - last_sent) >= 40) {
        reported = 1;
        last_sent = (long long)(t * 1000);
        int stamp = (int)(t * 1000 / 40);
        cqi_row = stamp % p.row_mod;
        if (cqi_row >= p.n_rows) { local_err = RS_CQI_TRACE; cqi_row = 0; }
        load = true;
      }
      if (load) {
        grid_loaded = true;
        for (int i = tid; i < U * R; i += nt) {
          int u = i / R, r = i - u * R;
          int tr = p.user_trace[(size_t)cell * U + u];
          s_cqi[r * Upad + u] = p.trace[((size_t)tr * p.n_rows + cqi_row) * R + r];
        }
      }
    }
    /* which buffers this TTI's winners and records live in (see kSpecSched) */
    const int n_items_rt = o.n_items;
    /* (a cell of fewer slices than the batch: the items are slice-major, the absent slices' are a suffix that is never listed or scanned) */
    const int n_items_n = (ragged_s && kTransport) ? Sn * R : n_items_rt;
    uint16_t* const cur_bu = s_best_user + ((kSpecSched && (tti & 1)) ? n_items_rt : 0);
    uint16_t* const nxt_bu = s_best_user + ((kSpecSched && !(tti & 1)) ? n_items_rt : 0);
    /* held winners: pack the items of chunk k0 that this wave has to scan again into its list (item = k * nwaves + wave: the
     * items a served user leads are neighbours -- one slice, many RBGs -- so every wave gets its share); returns their number */
    uint16_t* const hold_wl = hold_list + wave * 64;
    auto hold_pack = [&](int k0, int for_wave) -> int { /* for_wave: whose items (wave 1 also packs wave 0's in the serial phase) */
      const int it_l = (k0 + lane) * nwaves + for_wave;
      const bool in = it_l < n_items_n;
      const int w = in ? (int)cur_bu[it_l] : 0xFFFF;
      const bool held_bit = ((hold_bits[(k0 >> 6) * nwaves + for_wave] >> lane) & 1ull) != 0ull;
      const int sg_l = FIXED ? it_l / RS_JIT_R : idiv_small(in ? it_l : 0, R);
      const bool psi_on = (m->eps_psi[in ? sg_l : 0] & 2) != 0;
      const bool was_served = w != 0xFFFF && ((hold_served[(w & 2047) >> 5] >> (w & 31)) & 1u) != 0u;
      const bool need = in && w != 0xFFFF && (!held_bit || (was_served && psi_on));
      const unsigned long long mk = __ballot(need);
      if (need) hold_list[for_wave * 64 + __popcll(mk & ((1ull << lane) - 1ull))] = (uint16_t)it_l;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      return __popcll(mk);
    };
    /* sched 9 scans s_sorted in the serial phase, so the next TTI's records can go straight to s_elems; the policies that read
     * the records themselves (8, 101, 103) alternate between s_elems and the otherwise unused s_sorted */
    constexpr bool kAltRec = kSpecSched && SCHED != 9;
    uint32_t* const cur_rec = (kAltRec && (tti & 1)) ? s_sorted : s_elems;
    uint32_t* const nxt_rec = (kAltRec && !(tti & 1)) ? s_sorted : s_elems;
    RsSpecFlags* const fl_cur = &m->spec[tti & 1];        /* flags of this TTI's serial phase */
    RsSpecFlags* const fl_prev = &m->spec[(tti & 1) ^ 1]; /* ... of the previous one (read by the fix-up below) */
    uint32_t* const served_bits = (uint32_t*)m->hist;     /* [32] users served in the serial phase (m->hist is free then) */
    uint16_t* const fix_list = m->hist + 64;              /* items to rescan, RS_FIX_CAP entries */
    /* items the scanning waves take in the serial phase: whole rounds of nt - 64 lanes (at least one round) */
    auto spec_items = [&](int n) {
      const int nsp_ = nt > 64 ? nt - 64 : 64; /* (one-wave cells never speculate) */
      /* the serial phase lasts ~330 cycles per RBG, a round of scans ~4 000-5 000: with many RBGs every round fits (64 RBGs:
       * 13.06 instead of 12.92 M TTIs/s), with 25 a second, nearly empty round would outlast the serial wave */
      const int rounds_all = (n + nsp_ - 1) / nsp_;
      if (rounds_all * 16 <= R) return n;
      const int rounds = n / nsp_;
      return rounds == 0 ? n : rounds * nsp_;
    };
    /* averageRate /= 1000.0 (ref: :685-689).  The three-instruction form needs an ordinary operand (no underflow, finite); the
     * drop-in entry point takes any double from its caller, and when one is out of range (p.exact_scan, set by the host) it
     * divides for real -- inf / 1000 is inf, the short form would give NaN. */
    auto div_1000 = [&](double k) -> double {
      if constexpr (DIRECT) {
        if (p.exact_scan) return k / 1000.0;
      }
      return rs_div_1000(k);
    };
    /* PF terms of a user whose average is `a`: exact denominator and stage-1 reciprocal (ref: :685-689) */
    auto pf_terms = [&](int u, double a) {
      double k = 1;
      k += a;
      k = div_1000(k);
      if constexpr (DIRECT) {
        if (p.gen_exp) k = a; /* general exponents: the caller's block already holds pow(avg_kbps, psi) (host libm) */
      }
      s_avgk[u] = k;
      const int uo = s_uoff[u];
      /* stage-1 ranking only, never part of a result; psi == 0 slices rank on the numerator */
      s_rcp32[u + (uo & ~7)] = (uo & 1) ? __builtin_amdgcn_rcpf((float)k) : 1.0f; /* v_rcp_f32, 1 ulp */
    };
    /* ---------------- P1: PF EWMA (ref: src/flows/radio-bearer.cpp:139-164) ---------------- */
    if constexpr (QUEUE) {
      if (tid < 64) { q_slice_prio[tid] = 0; q_slice_act[tid] = 0; }
      __syncthreads();
      const bool do_ewma = !(t == last_update);
      const double dt = t - last_update;
      for (int u = tid; u < U; u += nt) {
        stop_schedule_user(u, tti - 1);
        bool has[2] = {false, false};
        double bavg[2] = {0, 0};
        for (int b = 0; b < 2; ++b) {
          const int kind = kind_of[u * 2 + b];
          if (kind == 0) continue;
          /* RadioBearer::UpdateAverageTransmissionRate: every bearer, scheduled or not */
          double a = qavg_base[b * U + u];
          if (do_ewma) {
            const double rate = (double)(QI(QF_TX, b, u) * 8) / dt;
            const double beta = 0.02;
            a = ((1 - beta) * a) + (beta * rate);
            if (a < 1) a = 1;
            qavg_base[b * U + u] = a;
            QI(QF_TX, b, u) = 0;
          }
          bavg[b] = a;
          if (kind == 2) {
            /* the applications' Send() events with a time stamp up to now (MacQueue::Enqueue per packet).  With the state in LDS
             * the next burst's time stamp is cached: a TTI without arrivals touches no HBM */
            int qp = QI(QF_PKTS, b, u);
            if (!q_lds || qs_next[b * U + u] <= t) {
              const size_t a0 = q_lds ? (size_t)qs_a0[b * U + u] : (size_t)p.arr_off[(size_t)(cell * U + u) * 2 + b];
              const int n_arr = q_lds ? qs_narr[b * U + u] : (int)((size_t)p.arr_off[(size_t)(cell * U + u) * 2 + b + 1] - a0);
              int tail = QI(QF_TAIL, b, u), qb = QI(QF_BYTES, b, u);
              const int tail0 = tail, qp0 = qp;
              while (tail < n_arr && p.arr_time[a0 + tail] <= t) {
                const int nfull = p.arr_nfull[a0 + tail], last = p.arr_last[a0 + tail];
                qb += nfull * RS_FULL_PACKET + last;
                qp += nfull + (last > 0 ? 1 : 0);
                tail += 1;
              }
              if (tail != tail0) { QI(QF_TAIL, b, u) = tail; QI(QF_BYTES, b, u) = qb; QI(QF_PKTS, b, u) = qp; }
              if (q_lds) {
                qs_next[b * U + u] = tail < n_arr ? p.arr_time[a0 + tail] : __builtin_inf();
                /* an empty queue's head is its first new burst */
                if (qp0 == 0 && tail != tail0) {
                  const int head = QI(QF_HEAD, b, u);
                  qs_headt[b * U + u] = p.arr_time[a0 + head];
                  qs_hnf[b * U + u] = p.arr_nfull[a0 + head];
                  qs_hla[b * U + u] = p.arr_last[a0 + head];
                }
              }
            }
            has[b] = qp > 0;
          } else {
            has[b] = true; /* InfiniteBuffer: HasPackets() is always true */
          }
        }
        const bool active = has[0] || has[1];
        if constexpr (kQSerial) {
          q_data0[u] = has[0] ? queue_data(kind_of[u * 2], 0, u) : 0;
          q_data1[u] = has[1] ? queue_data(kind_of[u * 2 + 1], 1, u) : 0;
          q_done[2 * u] = 0;
          q_done[2 * u + 1] = 0;
        }
        if constexpr (SCHED == 1) {
          /* flows, not users: each bearer competes with its own average (dl-pf-packet-scheduler.cpp:128-140) */
          s_avg[u] = bavg[0];
          s_avgk[u] = bavg[1];
          continue;
        }
        double k = 1; /* averageRate = 1; += every bearer of the record, in index order (:681-686) */
        if (has[0]) k += bavg[0];
        if (has[1]) k += bavg[1];
        k = rs_div_1000(k);
        s_avgk[u] = k;
        if (active) {
          const int sl = slice_of[u];
          atomicMax(&q_slice_prio[sl], has[1] ? 1 : 0);
          q_slice_act[sl] = 1;
        }
        q_fl[u] = active ? 2 : 0;
      }
      last_update = t;
      __syncthreads();
      for (int u = tid; u < U && SCHED != 1; u += nt) {
        const int flags = q_fl[u];
        const int sl = slice_of[u];
        const int uo = s_uoff[u];
        float r32 = 0.0f;
        if (flags & 2) {
          r32 = (uo & 1) ? __builtin_amdgcn_rcpf((float)s_avgk[u]) : 1.0f;
          const int sl_bits = m->eps_psi[sl];
          if (sl_bits & 4) {
            /* customised slice (ref: :694-711): the slice's priority = the highest bearer priority with packets in the slice */
            const int pb = q_slice_prio[sl];
            const int kind = kind_of[u * 2 + pb];
            const bool has_data = queue_data(kind, pb, u) != 0;
            double hol = 0.0; /* GetHeadOfLinePacketDelay: 0 with an empty MAC queue (an InfiniteBuffer bearer has none) */
            if (kind == 2 && QI(QF_BYTES, pb, u) != 0) {
              double head_time;
              if (q_lds) {
                head_time = qs_headt[pb * U + u];
              } else {
                const size_t a0 = (size_t)p.arr_off[(size_t)(cell * U + u) * 2 + pb];
                head_time = p.arr_time[a0 + QI(QF_HEAD, pb, u)];
              }
              hol = t - head_time;
              if (hol < 0.00001) hol = 0.00001;
            }
            q_ho[u] = hol;
            q_fl[u] = (uint8_t)(2 | (has_data ? 1 : 0));
            r32 = !has_data ? 0.0f : ((SCHED == 7 || (sl_bits & 8) != 0) ? r32 * (float)hol : r32);
          }
        }
        s_rcp32[u + (uo & ~7)] = r32;
      }
      __syncthreads();
    } else
    if (!have_spec && !have_ewma) {
      const bool do_ewma = !kDirect && !(t == last_update);
      const double dt = t - last_update;
      auto ewma_user = [&](int u, int ku) {
        double a = s_avg[u];
        if ((kSpecSched || kHoldSched || kEarly17) && a < 1) a = 1; /* an update prepared in the serial phase leaves the unclamped product behind */
        if (do_ewma) {
          int txb = s_tx[u];
          if (kCumRegs) {
            cum_r[ku < kKU ? ku : 0] += (txb >> RS_TX_NPRB_SHIFT) & RS_TX_NPRB_MASK;
            txb &= RS_TX_BYTES_MASK;
            cum_b[ku < kKU ? ku : 0] += txb;
          }
          double rate = (double)(txb * 8) / dt;
          const double beta = 0.02;
          a = ((1 - beta) * a) + (beta * rate);
          if (a < 1) a = 1;
          s_avg[u] = a;
          s_tx[u] = 0;
        }
        if (SCHED != 1) {
          if (!queue_mode_in) {
            pf_terms(u, a);
          } else {
            /* ref: :685-689  averageRate = 1 + sum(avg); averageRate /= 1000.0 */
            double k = 1;
            k += a;
            k = div_1000(k);
            if constexpr (DIRECT) {
              if (p.gen_exp) k = a;
            }
            s_avgk[u] = k;
            const int uo = s_uoff[u];
            float r32 = (uo & 1) ? __builtin_amdgcn_rcpf((float)k) : 1.0f;
            /* customised slice (ref: :694-711): metric 0 while the prioritized bearer is empty, times the
             * head-of-line delay when beta (sched 7: always) -- folded into the stage-1 factor */
            const int sl = kPrefetch ? pre_sl[ku < kPU ? ku : 0] : (int)cfg_user_slice[u];
            if (m->eps_psi[sl] & 4) { /* algo_alpha */
              const bool has = prio_in ? (prio_in[u] & 1) != 0 : true;
              const bool use_hol = SCHED == 7 || SCHED == 11 || (m->eps_psi[sl] & 8) != 0; /* algo_beta */
              r32 = !has ? 0.0f : (use_hol ? r32 * (float)hol_in[u] : r32);
            }
            s_rcp32[u + (uo & ~7)] = r32;
          }
        } else {
          s_rcp32[u] = __builtin_amdgcn_rcpf((float)a);
        }
      };
      if constexpr (kCumRegs) {
#pragma unroll
        for (int ku = 0; ku < kKU; ++ku)
          if (tid + ku * nt < Un) ewma_user(tid + ku * nt, ku);
      } else if constexpr (kPrefetch) {
#pragma unroll
        for (int ku = 0; ku < kPU; ++ku)
          if (tid + ku * nt < U) ewma_user(tid + ku * nt, ku);
      } else {
        for (int u = tid, ku = 0; u < Un; u += nt, ++ku) ewma_user(u, ku);
      }
      if (!kDirect) last_update = t;
      __syncthreads();
    } else {
      /* the previous serial phase has already updated every average for this TTI (speculatively, then exactly for the
       * served users); what is left is bookkeeping: the owners count the bytes granted in the previous TTI */
      if constexpr (kCumRegs) {
#pragma unroll
        for (int ku = 0; ku < kKU; ++ku) {
          const int u = tid + ku * nt;
          if (u < Un) {
            int v = s_tx[u];
            if (v != 0) {
              /* (NVS with its winners in place runs this TTI without a barrier before wave 0's next grant: take the word atomically) */
              if (kEarly17 && SCHED == 7) v = atomicExch(&s_tx[u], 0);
              else s_tx[u] = 0;
              cum_r[ku] += (v >> RS_TX_NPRB_SHIFT) & RS_TX_NPRB_MASK;
              cum_b[ku] += v & RS_TX_BYTES_MASK;
            }
          }
        }
      }
      last_update = t;
      /* (the barrier that ends the EWMA phase also separates the CQI refresh from the scans that read the grid: a TTI whose
       * averages were prepared beforehand still needs it when P0 loaded a grid -- round 2's speculation never prepared such a TTI) */
      if (grid_loaded) __syncthreads();
    }
    RS_STAMP(0);

