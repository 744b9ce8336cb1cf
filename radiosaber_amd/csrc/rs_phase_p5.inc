/* rs_phase_p5.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: the serial end of the TTI on wave 0, second half: which lanes hold one user, EESM sum in the reference's order, final CQI, MCS, TBS, DoStopSchedule counters, the served users' exact EWMA for a prepared next TTI, the optional decision log. */
      /* ---------------- P5: link adaptation + DoStopSchedule counters (lanes = RBGs) ---------------- */
      /* lanes holding the same user; the lowest one (leader) handles the user */
      constexpr bool kFlows = kQSerial && SCHED == 1; /* owner = flow id 2 * user + bearer */
#if defined(RS_STAMPS) && defined(RS_STAMPS_P5) /* diagnostic: where P5's cycles go (sub-stamp slots, thread 0) */
      unsigned long long p5_prev = __builtin_readcyclecounter();
#define RS_P5STAMP(i) do { if (tid == 0) { unsigned long long n_ = __builtin_readcyclecounter(); sort_sub[i] += n_ - p5_prev; p5_prev = n_; } } while (0)
#else
#define RS_P5STAMP(i) do { } while (0)
#endif
      /* owner + 1 < 4096 = two base-64 digits: the lanes that share both digits share the owner.  One LDS atomic OR per digit
       * into the sort's two 64-entry mask arrays (idle here), ~15 instructions and one LDS round trip */
      /* (round 6: the E value of every RBG lane's own RBG for its owner -- two dependent LDS reads that need nothing but `owner` -- is
       * asked for here, in front of the atomics and fences below, instead of behind them: the two round trips overlap) */
      const uint8_t* const col = s_cqi + (owner < 0 ? 0 : (kFlows ? owner >> 1 : owner));
      /* (the transport schedulers only: per-flow PF loses a tenth with the early read -- 152.3 against 168.4 M TTIs/s, NVS 0.5 % --, they
       * keep it where it was, behind the owner masks) */
      double ev_mine = 0.0;
      if (kTransport && !per_prb) {
        const double ev = s_e[col[(lane < R ? lane : 0) * Upad]];
        ev_mine = (lane < R && owner >= 0) ? ev : 0.0;
      }
      unsigned long long same = 0ull;
      {
        const bool has = lane < R && owner >= 0;
        const int key = has ? owner + 1 : 0;
        /* (MaximizeCell's vector scan leaves both mask arrays cleared: every vector cleans the entries it set) */
        if constexpr (!(FIXED && kVecScan)) {
          m->maskA[lane] = 0ull;
          m->maskB[lane] = 0ull;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
        if (has) {
          atomicOr(&m->maskA[key & 63], 1ull << lane);
          atomicOr(&m->maskB[key >> 6], 1ull << lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned long long lo = m->maskA[key & 63], hi = m->maskB[key >> 6];
        if (has) same = lo & hi;
      }
      RS_P5STAMP(0);
      const bool leader = owner >= 0 && (same & ((1ull << lane) - 1ull)) == 0;
      const unsigned long long lead_mask = __ballot(leader);
      served_prev = __popcll(lead_mask);
      /* ref: :618-620 slice_rbs_offset_ = target - final_rbgs*rbg_size */
      if (kTransport && lane < Sn && !(QUEUE && *q_any == 0))
        s_sstate[lane] = (double)(((kSpecSched || kHoldSched) ? my_target : m->target[lane]) - got * G);
      if (lane == 0) m->served = served_prev;
      if (kHoldSched) {
        if (leader) atomicOr(&hold_served[(owner & 2047) >> 5], 1u << (owner & 31)); /* next TTI: these users' items are scanned again */
        if (quota_next) { /* slice offsets and the served count are in place: the quota wave may finish TTI t+1's quotas */
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (lane == 0) atomicExch(&fl_cur->greedy_done, 2);
        }
      }
      if (kSpecSched && spec_next) {
        /* the allocation is decided: tell the scanning waves who was served (their speculative winners among these need a
         * second look) and let the quota wave start TTI t+1's quotas (slice offsets and the served count are in place) */
        if (leader) atomicOr(&served_bits[owner >> 5], 1u << (owner & 31));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) atomicExch(&fl_cur->greedy_done, 2); /* 1: slice offsets final, 2: served set published too */
      }
      RS_P5STAMP(1);
      int tbs = 0, nprb = 0, fcqi = 0, mcs = 0;
      int tbs_bytes_next = 0; /* bytes of this TTI's grant, for the served user's next EWMA update (speculated TTIs) */
      int rec_bytes = 0; /* grant records: what DoStopSchedule credits this leader's user (0: no record) */
      {
        /* ref: :638-651 -- PRBs in RBG-ascending order, G identical adds per RBG
         * (src/utility/eesm-effective-sinr.h:33-46 with the exp() values tabulated by the host) */
        unsigned long long mm = leader ? same : 0ull;
        double sum = 0;
        /* every RBG lane has looked up the E value of its own RBG for its owner once (two dependent LDS reads, all lanes side by
         * side: `ev_mine`, above); the leaders collect their lanes' values in RBG order with lane reads instead of two LDS round trips per RBG */
        if (!per_prb) {
          if (!kTransport) ev_mine = (lane < R && owner >= 0) ? s_e[col[lane * Upad]] : 0.0;
          /* Four RBGs of every user per round: the four source lanes first, their lane reads side by side (one crossbar latency
           * instead of four), then the additions in RBG order.  One RBG per round took 1 780 of NVS's 6 500 cycles per TTI (a user
           * of the served slice holds up to six RBGs), ~950 for the transport schedulers (round 4, tools/phase_stamps.py --p5).
           * Up to 32 RBGs the lane sets are 32-bit masks (one v_ffbl each). */
          constexpr bool kM32 = FIXED && RS_JIT_R <= 32;
          uint32_t mm32 = (uint32_t)mm;
          while (__ballot(kM32 ? mm32 != 0u : mm != 0ull) != 0ull) { /* every lane stays in the loop: a lane read from a masked-off lane returns 0 */
            int src[4];
            bool more[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (kM32) {
                more[i] = mm32 != 0u;
                src[i] = more[i] ? __ffs((int)mm32) - 1 : 0;
                mm32 &= mm32 - 1u;
              } else {
                more[i] = mm != 0ull;
                src[i] = more[i] ? __ffsll((long long)mm) - 1 : 0;
                mm &= mm - 1ull;
              }
            }
            /* (round 6: most users hold one or two RBGs -- the second pair of lane reads and its 2 G dependent FP64 additions are
             * skipped, wave-uniformly, in a round where no user has a third) */
            /* (the transport schedulers only: the served slice's users of NVS and the per-flow PF scheduler's hold up to six -- there the
             * test and the split batch of lane reads lose: 265.9 against 267.7 and 166.0 against 169.8 M TTIs/s, same lease) */
#ifdef RS_P5_NO_PAIR_SKIP
            const bool pair2 = true;
#else
            const bool pair2 = !kTransport || __builtin_amdgcn_ballot_w64(more[2]) != 0ull;
#endif
            double ev[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) ev[i] = __shfl(ev_mine, src[i], 64);
            if (pair2) {
#pragma unroll
              for (int i = 2; i < 4; ++i) ev[i] = __shfl(ev_mine, src[i], 64);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
              if (more[i]) {
                for (int k = 0; k < G; ++k) sum += ev[i];
                nprb += G;
              }
            if (pair2) {
#pragma unroll
              for (int i = 2; i < 4; ++i)
                if (more[i]) {
                  for (int k = 0; k < G; ++k) sum += ev[i];
                  nprb += G;
                }
            }
          }
          mm = 0ull;
        }
        while (mm) {
          const int r2 = __ffsll((long long)mm) - 1;
          mm &= mm - 1;
          if (per_prb) {
            /* per-PRB reports (the simulated channel's, or a per-PRB batch source): read the RBG's PRBs from HBM */
            const uint8_t* pr = prb_ptr(kFlows ? owner >> 1 : owner, r2);
            for (int k = 0; k < G; ++k) sum += s_e[pr[k]];
          } else {
            const double ev = s_e[col[r2 * Upad]];
            for (int k = 0; k < G; ++k) sum += ev;
          }
          nprb += G;
        }
        RS_P5STAMP(2);
        /* the synthetic-experiment build (rs_config.synthetic_exp; ref: :653-659, nvs :336-342): the transport block adds up every
         * allocated PRB at the MCS of its own CQI.  Every RBG lane works out its RBG's bits, the leaders add up their lanes
         * (integers: any order). */
        int syn_bits = 0;
        if (p.synthetic && (SCHED == 7 || kTransport)) {
          int t1 = 0;
          if (lane < R && owner >= 0) {
            if (per_prb) {
              const uint8_t* pr = prb_ptr(owner, lane);
              for (int k = 0; k < G; ++k) t1 += m->tbs1_of_cqi[pr[k]];
            } else {
              t1 = G * m->tbs1_of_cqi[col[lane * Upad]];
            }
          }
          unsigned long long ms = leader ? same : 0ull;
          while (__ballot(ms != 0ull) != 0ull) {
            const bool more = ms != 0ull;
            const int r2 = more ? __ffsll((long long)ms) - 1 : 0;
            ms &= ms - 1;
            const int v = __shfl(t1, r2, 64);
            if (more) syn_bits += v;
          }
        }
        RS_P5STAMP(3);
        if (kGridAhead && grid_next) {
          /* this wave has read all it needs of TTI t's CQI grid (the lanes' E values and PRB bits above): the other waves may write
           * TTI t+1's grid over it (LDS serves a wave's instructions in order: the reads above are done when this store lands) */
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (lane == 0) __hip_atomic_store(&m->grid_free, tti + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (leader) {
          const double x = sum / (double)nprb;
          if (x == 0) {
            fcqi = 15;
          } else {
            fcqi = 1;
#pragma unroll
            for (int k = 1; k <= 13; ++k) fcqi += (x <= xthr_k[k - 1]) ? 1 : 0; /* thresholds: wave-uniform, read before the TTI loop */
          }
          RS_P5STAMP(4);
          mcs = m->mcs_of_cqi[fcqi];
          tbs = (p.synthetic && (SCHED == 7 || kTransport)) ? syn_bits : s_tbs[(nprb / G) * 16 + fcqi];
          /* DoStopSchedule, ref: :170-221 (bytes = bits/8, capped by dataToTransmit = 1e8) */
          int bytes = tbs / 8;
          if (bytes > 100000000) bytes = 100000000;
#if defined(RS_FAULT_INJECT_JIT) || (defined(RS_FAULT_INJECT_P3B8) && RS_P3_BLOCK == 8) || (defined(RS_FAULT_INJECT_LEAN) && defined(RS_JIT_LEAN) && RS_JIT_LEAN)
          /* tests only (tests/test_gpu_round5.py): a deliberately wrong run-time build, so that rs_batch_config.selfcheck and the autotune's
           * state comparison have something to catch -- one byte more per grant in shape-specialised kernels */
          if (FIXED && bytes > 0) bytes += 1;
#endif
          if (bytes > 0) {
            if (kFlows) {
              /* this flow's transport block: credited to its own bearer by the owner thread (stop_schedule_user) */
              if (owner & 1) q_grant1[owner >> 1] = bytes | (nprb << RS_TX_NPRB_SHIFT);
              else s_tx[owner >> 1] = bytes | (nprb << RS_TX_NPRB_SHIFT);
            } else if (kCumRegs || QUEUE) {
              /* the owner thread of P1 counts it (registers) / splits it over the user's bearers and dequeues (queue model) */
              atomicAdd(&s_tx[owner], bytes | (nprb << RS_TX_NPRB_SHIFT)); /* one ds_add, nothing to wait for (this lane is the word's only writer) */
            } else {
              /* the next EWMA update consumes the bytes: in a speculated TTI that happens right below, on this lane */
              if (!(kSpecSched && spec_next)) s_tx[owner] += bytes;
              /* RadioBearer::m_cumulativeBytes / m_cumulativeRBs live in HBM: fire-and-forget atomics (batches; a drop-in call's counters
               * are the simulator's own, DoStopSchedule keeps them) */
              if (!DIRECT) {
                atomicAdd((unsigned long long*)&p.cum_bytes[(size_t)cell * U + owner], (unsigned long long)bytes);
                atomicAdd((unsigned long long*)&p.cum_rbs[(size_t)cell * U + owner], (unsigned long long)nprb);
              }
            }
          }
          if ((kSpecSched && spec_next) || (kHoldSched && ewma_next) || early17) tbs_bytes_next = bytes;
          if (rec_on) rec_bytes = bytes;
        }
      }
      if (rec_on) {
        /* Grant records (rs_batch_run_grant_records): the leaders whose users are credited take the TTI's places behind the cell's
         * running count -- one ballot says which lanes -- and store their record as two 16-byte halves.  A lane's place among them is
         * the number of those lanes with a smaller user: DoStopSchedule's order, so the host finds every TTI's stretch sorted (lane
         * order is RBG order, which says nothing about the users'; sorting 50 records per cell-TTI on the host cost three times the
         * launch, profiles/batch_grant_records.md).  The walk over the ballot's bits is wave-uniform: a scalar loop, one lane read and
         * one compare per served user, every lane in it.  A place at or behind the capacity is not written, the count goes on. */
        const bool w = leader && rec_bytes > 0;
        const unsigned long long wm = __ballot(w);
        int rank = 0;
        for (unsigned long long it = wm; it != 0ull; it &= it - 1ull) {
          const int o = __builtin_amdgcn_readlane(owner, __ffsll((long long)it) - 1);
          rank += o < owner ? 1 : 0;
        }
        const int place = rec_count + rank;
        if (w && place < rec_cap) {
#if defined(RS_FAULT_INJECT_RECORDS)
          /* tests only: a run-time build whose RECORD says one byte more than was credited -- the state agrees, only the self-check's
           * comparison of the record lists can catch it */
          if (FIXED) rec_bytes += 1;
#endif
          int4* const dst = (int4*)(rec_list + place);
          dst[0] = make_int4((int)n_done, owner, tbs, rec_bytes);
          dst[1] = make_int4((int)(uint32_t)same, (int)(uint32_t)(same >> 32), nprb, fcqi | (mcs << 8));
        }
        rec_count += __popcll(wm);
      }
      RS_P5STAMP(5);
      if ((kHoldSched && ewma_next) || early17) {
        /* the exact EWMA of the served users for TTI t+1, on top of the decay the other waves applied (all of them first).
         * (Handing these ~900 cycles to wave 1 through an LDS list was measured and lost -- NVS 164 against 184 M TTIs/s, GreedyByRow
         * 97.8 against 98.4: the update is a dependent chain that nothing overlaps with, whoever runs it, and the hand-over adds a
         * polling round trip; profiles/r04_sched17.md) */
        while (rs_lds_load(&fl_cur->ctr_p1) < nwaves - 1) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (leader) {
          const double t_next = t + 0.001;
          const double dt_next = t_next - t; /* Now - m_lastUpdate of the next update: m_lastUpdate is this TTI's time */
          double a = SCHED == 1 ? s_avgk[owner] : s_avg[owner];
          const double rate = (double)(tbs_bytes_next * 8) / dt_next;
          const double beta = 0.02;
          a = a + (beta * rate);
          if (a < 1) a = 1;
          s_avg[owner] = a;
          if (SCHED == 1) s_rcp32[owner] = __builtin_amdgcn_rcpf((float)a);
          else pf_terms(owner, a);
        }
      }
      if (kSpecSched && spec_next) {
        /* Exact EWMA of the served users for TTI t+1 (ref: src/flows/radio-bearer.cpp:139-164): the scanning waves left
         * (1 - beta) * avg, unclamped, in s_avg; adding beta * rate gives the reference's sum of the two rounded products.
         * Not before every speculative scan is over: they must all have seen one state, the speculative one. */
        RS_STAMP(7);
        while (rs_lds_load(&fl_cur->ctr_p3) < nwaves - 1) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        RS_STAMP(6);
        if (leader) {
          const double t_next = t + 0.001;
          const double dt_next = t_next - t; /* Now - m_lastUpdate of the next update: m_lastUpdate is this TTI's time */
          double a = s_avg[owner];
          const double rate = (double)(tbs_bytes_next * 8) / dt_next;
          const double beta = 0.02;
          a = a + (beta * rate);
          if (a < 1) a = 1;
          s_avg[owner] = a;
          pf_terms(owner, a);
        }
      }
      RS_P5STAMP(6);
#if defined(RS_FAULT_INJECT_DIRECT)
      /* tests only (tests/test_gpu_round6.py): a deliberately wrong run-time build of the ONE-TTI kernel -- a byte more in every transport
       * block it reports --, so that the specialised context's check against the built-in kernel has something to catch */
      if (FIXED && DIRECT && leader) tbs += 8;
#endif
      /* optional log */
      if (p.log_map) {
        size_t row = (size_t)cell * p.n_ttis + tti;
        if (lane < R) p.log_map[row * R + lane] = (int16_t)owner;
        if (lane < S) {
          if (p.log_quota) p.log_quota[row * S + lane] = (int16_t)((kSpecSched || kHoldSched) ? my_quota : m->quota[lane]);
          if (p.log_target) p.log_target[row * S + lane] = (int16_t)((kSpecSched || kHoldSched) ? my_target : m->target[lane]);
        }
        if (leader) {
          if (kFlows) { /* two flows of one user may both hold RBGs: the user's row shows their sum */
            if (p.log_tbs) atomicAdd(&p.log_tbs[row * U + (owner >> 1)], tbs);
          } else {
            if (p.log_tbs) p.log_tbs[row * U + owner] = tbs;
            if (p.log_uinfo) p.log_uinfo[row * U + owner] = nprb | (fcqi << 16) | (mcs << 24);
          }
        }
      }
