/* rs_phase_p4.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: P4 on all waves: MaximizeCell's std::sort emulation (rs_sort_device.h) and UpperBound (S segmented sorts + its own apply step). */
    /* ---------------- P4: inter-slice assignment ---------------- */
    if (SCHED == 9) {
      /* (a cell of fewer slices: the vector std::sort sees holds R * Sn records -- depth limit, pivots and the 16-element threshold are
       * that length's; position slots behind it are empty, whole ones included: to the levels they are retired positions.  The ranks'
       * and cuts' LDS offsets stay the carve's, made of R * S) */
      const int N = R * Sn, Ncv = R * S;
      /* std::sort emulation (:361): introsort loop, then the final insertion sort */
      {
        uint16_t* sx = (uint16_t*)(lds + o.sortx);
        uint16_t* pa = (uint16_t*)s_sorted;
        /* EPT = array positions per thread, picked by the host (0: any size, state in LDS) */
        /* Issue priority rises towards the serial end of the TTI: 0 for the throughput phases (EWMA, metric scan), 1 for the
         * barrier-paced sort levels, 2 for the counting sort, 3 for the one wave that runs the greedy scan and the link
         * adaptation.  A phase that meets a barrier every few dozen instructions loses most when the co-resident cell's
         * waves interleave with it (measured with two cells per CU: +5..6 % from the sort's priority alone). */
        RS_SETPRIO(1);
        if constexpr (kHoldSched) {
          if (!hold_full) {
            /* a TTI that scanned only the listed items: every thread rebuilds the records of the positions it owns in the sort
             * (the previous sort permuted the array in place) from the winners and the CQI grid */
            for (int x = tid; x < N; x += nt) {
              const int r = (FIXED && !kRaggedS) ? x / RS_JIT_S : idiv_small(x, Sn), sg = x - r * Sn;
              const int bu = cur_bu[sg * R + r];
              const uint32_t key = bu == 0xFFFF ? 0u : (uint32_t)s_cqi[r * Upad + bu];
              s_elems[x] = (key << 16) | ((uint32_t)r << 8) | (uint32_t)sg;
            }
            if (EPT == 0) __syncthreads(); /* (the LDS form of the sort reads other positions first) */
          }
        }
        if constexpr (EPT > 0) introsort_levels_reg<EPT, FIXED ? RS_JIT_NT : 0, kSegScan>(s_elems, N, s_sorted, (int32_t*)sx, m, sort_sub, 0,
                                                                           rs_sort_ranks_bytes(Ncv) ? (uint16_t*)(lds + o.sortx + rs_sort_cuts_bytes(Ncv)) : m->hist);
        else introsort_loop_levels(s_elems, N, pa, pa + N, sx, sx + N, sx + 2 * N, sx + 3 * N, m);
      }
      RS_STAMP(3);
      RS_SETPRIO(2);
      /* kSegScan: wave 0 reads the loop's array itself -- the tagged loop's closing barrier is all that is left of this phase */
      if constexpr (kSegScan) __syncthreads();
      else if constexpr (EPT > 0) counting_sort_desc_owned<EPT, FIXED ? RS_JIT_NT : 0>(s_elems, s_sorted, N, m);
      else counting_sort_desc(s_elems, s_sorted, N, m);
      RS_SETPRIO(0);
      RS_STAMP(4);
    }
    if constexpr (SCHED == 10) {
      /* ---------------- UpperBound, ref: :223-246 and the inter_sched_ >= 4 branch of :603-616 ----------------
       * Every slice with a positive quota sorts its own R (rbg, eff) pairs (the same unstable std::sort) and takes its
       * first quota RBGs whatever the other slices take.  The S sorts run as ONE level-synchronous pass over the
       * slice-major array (sub-ranges of a level are disjoint anyway); the final insertion sort of each call is a stable
       * rank inside its segment.  Then one thread per taken (slice, k) entry: the first entry of a UE is its leader and
       * sums E[cqi] over the UE's entries in push order (the slice's sorted order, not RBG order). */
      static_assert(EPT > 0, "UpperBound uses the register form of the sort (R*S <= 4 * threads)");
      const int N = R * Sn, Ncv = R * S; /* (a cell of fewer slices: Sn sorts; the LDS offsets stay the carve's) */
      RS_SETPRIO(1);
      introsort_levels_reg<EPT, FIXED ? RS_JIT_NT : 0>(s_elems, N, s_sorted, (int32_t*)(lds + o.sortx), m, sort_sub, R,
                                                       rs_sort_ranks_bytes(Ncv) ? (uint16_t*)(lds + o.sortx + rs_sort_cuts_bytes(Ncv)) : m->hist);
      RS_SETPRIO(0);
      int32_t* low_owner = (int32_t*)m->hist; /* per RBG: (slice << 16 | UE) of the lowest slice holding it */
      if (R > 32) {
        /* (round 5) one segment per wave pass, lane = position inside the segment: the stable rank is (elements of the segment with a
         * larger key) + (equal keys before me) from one same-key mask and a 16-entry count table per wave -- instead of R reads per
         * element (64 RBGs: 800 instructions per thread; the as-shipped grid's UpperBound 21.3 -> M TTIs/s, profiles/r05_notes.md) */
        uint32_t* const cnt = (uint32_t*)m->maskA + wave * 16; /* free behind the sort's workgroup levels (maskA | maskB: 16 waves) */
        const unsigned long long gt_lane = lane == 63 ? 0ull : (~0ull << (lane + 1));
        for (int sl = wave; sl < Sn; sl += nwaves) {
          const int f = sl * R;
          const bool valid = lane < R;
          const uint32_t e = valid ? s_elems[f + lane] : 0u;
          const int k = (int)(e >> 16);
          if (lane < 16) cnt[lane] = 0u;
          uint32_t dl = 0u, dh = 0u;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const uint32_t mine = (uint32_t)(((int)(e << (15 - b))) >> 31);
            const unsigned long long plane = __ballot(mine != 0u);
            dl |= (uint32_t)plane ^ mine;
            dh |= (uint32_t)(plane >> 32) ^ mine;
          }
          const unsigned long long vm = __ballot(valid);
          const uint32_t sl_ = (uint32_t)vm & ~dl, sh_ = (uint32_t)(vm >> 32) & ~dh;
          const int rank_eq = (int)__builtin_amdgcn_mbcnt_hi(sh_, __builtin_amdgcn_mbcnt_lo(sl_, 0u));
          if (valid && ((sl_ & (uint32_t)gt_lane) | (sh_ & (uint32_t)(gt_lane >> 32))) == 0u) cnt[k] = (uint32_t)(rank_eq + 1);
          /* lane q < 16: elements with a key above q (this wave's LDS operations execute in order: no barrier) */
          int inc = lane < 16 ? (int)cnt[lane] : 0;
          {
            int v_ = inc;
            const int identity = 0;
#define RS_ROW_STEP(ctrl, bmask) v_ = v_ + __builtin_amdgcn_update_dpp(identity, v_, ctrl, 0xf, bmask, false)
            RS_ROW_STEP(0x111, 0xf);
            RS_ROW_STEP(0x112, 0xf);
            RS_ROW_STEP(0x114, 0xe);
            RS_ROW_STEP(0x118, 0xc);
#undef RS_ROW_STEP
            inc = v_;
          }
          const int all = __builtin_amdgcn_readlane(inc, 15);
          const int above = __builtin_amdgcn_ds_bpermute(k << 2, all - inc); /* every lane */
          if (valid) s_sorted[f + above + rank_eq] = e;
        }
      } else
      for (int x = tid; x < N; x += nt) {
        const int f = idiv_small(x, R) * R;
        const uint32_t e = s_elems[x];
        const int k = (int)(e >> 16);
        int rank = 0;
        for (int y = f; y < f + R; ++y) {
          const int ky = (int)(s_elems[y] >> 16);
          rank += (ky > k || (ky == k && y < x)) ? 1 : 0;
        }
        s_sorted[f + rank] = e;
      }
      if (tid < R) low_owner[tid] = 0x7fffffff;
      if (tid == 0) {
        m->served = 0;
        if (rec_on) m->rec_tti = 0;
      }
      __syncthreads();
      uint16_t* ent_user = (uint16_t*)s_elems; /* s_elems is dead: UE of entry (slice, k), 0xFFFF = not taken */
      for (int x = tid; x < N; x += nt) {
        const int sl = idiv_small(x, R), k = x - sl * R;
        const int q = m->quota[sl];
        int u = 0xFFFF;
        if (k < q) { /* q <= 0: nothing; q > R cannot index past the segment (the reference would read past its vector) */
          const int rbg = (int)((s_sorted[x] >> 8) & 63u);
          u = s_best_user[sl * R + rbg];
          if (u != 0xFFFF) atomicMin(&low_owner[rbg], (sl << 16) | u);
        }
        ent_user[x] = (uint16_t)u;
        if (p.log_upper) p.log_upper[x] = u == 0xFFFF ? -1 : (int)((s_sorted[x] >> 8) & 63u) | (u << 8);
      }
      __syncthreads();
      for (int x = tid; x < N; x += nt) {
        const int sl = idiv_small(x, R), f = sl * R;
        const int u = ent_user[x];
        int q = m->quota[sl];
        q = q > R ? R : q;
        bool leader = u != 0xFFFF;
        for (int y = f; y < x && leader; ++y) leader = ent_user[y] != u;
        if (!leader) continue;
        double sum = 0;
        int nprb = 0, syn_bits = 0; /* syn_bits: the synthetic-experiment transport block, every PRB at its own CQI (:653-659) */
        unsigned long long rec_mask = 0ull; /* grant records: the RBGs of the slice's list that went to this UE */
        for (int y = x; y < f + q; ++y) {
          if (ent_user[y] != u) continue;
          const int r2 = (int)((s_sorted[y] >> 8) & 63u);
          rec_mask |= 1ull << r2;
          if (per_prb) {
            const uint8_t* pr = prb_ptr(u, r2);
            for (int g = 0; g < G; ++g) { sum += s_e[pr[g]]; syn_bits += m->tbs1_of_cqi[pr[g]]; }
          } else {
            const int cq = s_cqi[r2 * Upad + u];
            const double ev = s_e[cq];
            for (int g = 0; g < G; ++g) sum += ev;
            syn_bits += G * m->tbs1_of_cqi[cq];
          }
          nprb += G;
        }
        const double xm = sum / (double)nprb;
        int fcqi;
        if (xm == 0) {
          fcqi = 15;
        } else {
          fcqi = 1;
          for (int t = 1; t <= 13; ++t) fcqi += (xm <= s_x[t]) ? 1 : 0;
        }
        const int mcs = m->mcs_of_cqi[fcqi];
        const int tbs = p.synthetic ? syn_bits : s_tbs[(nprb / G) * 16 + fcqi];
        int bytes = tbs / 8;
        if (bytes > 100000000) bytes = 100000000;
        if (bytes > 0) {
          if (kCumRegs) {
            s_tx[u] += bytes | (nprb << RS_TX_NPRB_SHIFT);
          } else {
            s_tx[u] += bytes;
            if (!DIRECT) { /* (a drop-in call's counters are the simulator's own) */
              atomicAdd((unsigned long long*)&p.cum_bytes[(size_t)cell * U + u], (unsigned long long)bytes);
              atomicAdd((unsigned long long*)&p.cum_rbs[(size_t)cell * U + u], (unsigned long long)nprb);
            }
          }
        }
        atomicAdd(&m->served, 1);
        if (rec_on && bytes > 0) {
          /* Grant records (rs_batch_run_grant_records): the leaders take their places from one LDS counter, in arrival order, behind
           * the cell's count of the TTIs before (rs_kernels.hip adds the TTI's count behind its closing barrier); the host sorts. */
          const int place = rec_count + atomicAdd(&m->rec_tti, 1);
          if (place < rec_cap) {
            int rb = bytes;
#if defined(RS_FAULT_INJECT_RECORDS)
            if (FIXED) rb += 1; /* tests only, see rs_phase_p5.inc */
#endif
            int4* const dst = (int4*)(rec_list + place);
            dst[0] = make_int4((int)n_done, u, tbs, rb);
            dst[1] = make_int4((int)(uint32_t)rec_mask, (int)(uint32_t)(rec_mask >> 32), nprb, fcqi | (mcs << 8));
          }
        }
        if (p.log_map) {
          const size_t row = (size_t)cell * p.n_ttis + tti;
          if (p.log_tbs) p.log_tbs[row * U + u] = tbs;
          if (p.log_uinfo) p.log_uinfo[row * U + u] = nprb | (fcqi << 16) | (mcs << 24);
        }
      }
      if (tid < Sn) {
        /* ref: :618-620 with slice_final_rbgs = size of the slice's list */
        int q = m->quota[tid];
        q = q < 0 ? 0 : (q > R ? R : q);
        s_sstate[tid] = (double)(m->target[tid] - q * G);
      }
      if (p.log_map) {
        const size_t row = (size_t)cell * p.n_ttis + tti;
        if (tid < R) p.log_map[row * R + tid] = (int16_t)(low_owner[tid] == 0x7fffffff ? -1 : (low_owner[tid] & 0xffff));
        if (tid < S) {
          if (p.log_quota) p.log_quota[row * S + tid] = (int16_t)m->quota[tid];
          if (p.log_target) p.log_target[row * S + tid] = (int16_t)m->target[tid];
        }
      }
    }
