/* rs_phase_p3.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: P3 the metric scan: scan_item (exact two-stage arg-max of one (segment, RBG) item), the queue model's m_requiredRBs / quotient table for NVS, held winners (only the listed items, four lanes per item), the fix-up of a speculated TTI. */
    /* ---------------- P3: best user of every (RBG, segment) ---------------- */
    /* sched 7: the served slice in 8-aligned runs of nvs_seg users, so that a slice of a few dozen users keeps several waves
     * busy instead of R lanes; the run winners meet in P4 */
    const int nvs_seg = FIXED ? kCv.nvs_seg : p.nvs_seg;
    int nvs_lo = 0, nvs_hi = 0, nvs_first = 0;
    const bool nvs_split = SCHED == 7 && nvs_seg != 0;
    if (nvs_split) {
      nvs_lo = kDirect ? 0 : m->seg_begin[seg_lo];
      nvs_hi = kDirect ? U : m->seg_begin[seg_lo + 1];
      nvs_first = nvs_lo & ~7;
      nvs_runs = idiv_small(nvs_hi - nvs_first + nvs_seg - 1, nvs_seg);
    }
    const int n_items = nvs_split ? R * nvs_runs : n_items_n;
    /* one work item = (segment, RBG): winner to bu_out[it], its record (transport schedulers) to rec_out */
    auto scan_item = [&](int it, uint16_t* bu_out, uint32_t* rec_out, auto blk_tag) -> bool {
      bool held = false;
      float top1 = 0.0f, top2 = 0.0f; /* held winners: the two largest stage-1 values of the segment */
      {
        int sg = it / R, r = it - sg * R; /* r fastest: neighbouring lanes read neighbouring CQI bytes */
        int seg = SCHED == 7 ? seg_lo : sg;
        int ub = m->seg_begin[seg], ue = m->seg_begin[seg + 1];
        if (SCHED == 7 && kDirect) { ub = 0; ue = U; }
        if (nvs_split) {
          ub = nvs_first + sg * nvs_seg;
          ue = ub + nvs_seg;
          ub = ub < nvs_lo ? nvs_lo : ub;
          ue = ue > nvs_hi ? nvs_hi : ue;
        }
        double best = SCHED == 1 ? 0.0 : (SCHED == 7 ? -1.7976931348623157e308 : -1.0);
        int bu = -1;
        float run_a = 0.0f; /* stage-1 value of the leader (0: none yet) */
        bool exact = false; /* `best` is the leader's exact metric */
        int sl_eps = 1, sl_psi = 1;
        int sl_custom = 0; /* 1: alpha slice, 2: alpha slice with the HoL factor */
        int sl_id = 0;
        if (SCHED != 1) {
          int sl = SCHED == 7 ? (kDirect ? (int)p.user_slice[0] : seg) : seg;
          sl_id = sl;
          sl_eps = m->eps_psi[sl] & 1;
          sl_psi = (m->eps_psi[sl] >> 1) & 1;
          if (queue_mode_in && (m->eps_psi[sl] & 4)) sl_custom = (SCHED == 7 || (m->eps_psi[sl] & 8) != 0) ? 2 : 1;
        }
        const uint8_t* rowp = s_cqi + r * Upad;
        /* Exact two-stage argmax (DESIGN.md 2.6).  Stage 1 ranks the segment's users by the cheap
         * FP32 product a~ = fl32(num) * rcp32(fl32(den)) (v_rcp_f32, 1 ulp), which is within 2^-21.4 (relative) of the
         * reference's rounded FP64 quotient q = fl(num/den); a user whose a~ is below (1 - 2^-19) of
         * the largest a~ has a strictly smaller q and can neither win nor tie.  Stage 2 evaluates
         * the survivors with the real IEEE FP64 division, ascending user order, strict '>'.
         * Stage 1 reads 8 users per step (one 8-byte CQI load, two 16-byte reciprocal loads), keeps
         * the 32 products of a block in registers, takes their maximum, then marks the survivors. */
        const float kTol = 0x1.ffffcp-1f; /* 1 - 2^-19 */
        /* sched 7 scans runs of 8..32 users: a shape-specialised build ranks exactly one run per block */
        /* (the speculating schedulers carry this scan twice, here and in the serial phase: 32 products per block would spill) */
        constexpr int kP3Block = decltype(blk_tag)::v != 0 ? decltype(blk_tag)::v
                                 : (SCHED == 7 && FIXED && kCv.nvs_seg != 0) ? kCv.nvs_seg
                                 : ((kSpecSched && RS_P3_BLOCK > 16) ? 16 : RS_P3_BLOCK);
        const bool one_num = SCHED != 1 && !sl_eps;
        const float* numtab = one_num ? m->ones16 : s_num32; /* a table either way: no branch per user */
        /* this slice's window, indexed by user (drop-in NVS passes the served slice's users only: their own slice id) */
        const float* rcw = s_rcp32 + (SCHED == 1 ? 0 : m->rcp_off[(SCHED == 7 && kDirect) ? (int)p.user_slice[0] : seg]);
        /* stage 2 of one user: the reference's expression, real IEEE FP64 division */
        auto exact_metric = [&](int u, int c) -> double {
          if (SCHED == 1) {
            /* ref: dl-pf-packet-scheduler.cpp:128-140  (se*180000.)/avg */
            return s_num[c] / s_avg[u];
          }
          /* ref: :688-693  pow(se_kbps, eps) / pow(avg_kbps, psi), eps, psi in {0,1} */
          /* both table reads are issued whatever the slice's exponents are (no branch around an LDS read) */
          const double num_c = s_num[c], den_u = s_avgk[u];
          double num = sl_eps ? num_c : 1.0, den = sl_psi ? den_u : 1.0;
          if constexpr (DIRECT) {
            /* pow(se_kbps, epsilon) / pow(avg_kbps, psi) for any integers (ref: :690-693): both powers come from the host's libm
             * -- 16 numerators per slice at rs_create, the denominator of every user per call -- the device only divides */
            if (p.gen_exp) { num = p.gen_num[sl_id * 16 + c]; den = den_u; }
          }
          if (QUEUE && (prio_in[u] & 2) == 0) return -2.0; /* not in UsersToSchedule: below the scan's start value of -1 */
          /* (schedulers 1 and 7 with queues do not come here: serial allocator below) */
          if (sl_custom && prio_in && (prio_in[u] & 1) == 0) return 0.0;
          if (sl_custom == 2) return hol_in[u] * num / den; /* HoL * pow(se) / pow(avg), left to right */
          return num / den;
        };
        if constexpr (DIRECT) {
          /* The caller's averages / head-of-line delays are arbitrary doubles (the batch EWMA keeps its own in [1, ~1e12]): when
           * one of them is not an ordinary FP32 number -- huge, tiny, negative, infinite, NaN -- the stage-1 error bound does not
           * hold, the host says so (rs_schedule_tti), and every user of the segment is compared with the reference's expression
           * itself, ascending, strict '>' (a NaN metric never wins, as in the reference's scan). */
          if (p.exact_scan) {
            for (int u = ub; u < ue; ++u) {
              const double metric = exact_metric(u, rowp[u]);
              if (metric > best) { best = metric; bu = u; }
            }
            exact = true;
            ub = ue; /* nothing left for the block loop */
          }
        }
        /* (an empty segment must not enter: its 8-aligned start lies before its end, inside a neighbour's window) */
        for (int blk = ue > ub ? (ub & ~7) : ue; blk < ue; blk += kP3Block) {
          /* a~ of the 32 users blk..blk+31 (0 for users outside [ub, ue) and for the padding) */
          float av[kP3Block];
          float best_a = 0.0f;
#pragma unroll
          for (int g = 0; g < kP3Block / 8; ++g) {
            const int u0 = blk + 8 * g;
            uint2 cw = make_uint2(0u, 0u);
            float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
            if (u0 < ue) {
              cw = *(const uint2*)(rowp + u0);
              ra = *(const float4*)(rcw + u0);
              rb = *(const float4*)(rcw + u0 + 4);
            }
            const float rc[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
            float nm[8];
            /* CQI bytes are <= 15, so four of them scale to table byte offsets with one shift and each address is
             * one byte-select add */
            const uint32_t cx4 = cw.x << 2, cy4 = cw.y << 2;
#pragma unroll
            for (int k = 0; k < 8; ++k)
              nm[k] = *(const float*)((const char*)numtab + (((k < 4 ? cx4 : cy4) >> (8 * (k & 3))) & 0xffu));
#pragma unroll
            for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(nm[k])); /* eight table reads in flight, none behind a branch */
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              /* no range test: a slot outside the slice (or, sched 1, beyond the last user) reads a zero reciprocal */
              const float a = nm[k] * rc[k];
              av[8 * g + k] = a;
              best_a = fmaxf(best_a, a);
              if constexpr (kHoldSched) {
                top2 = fmaxf(top2, fminf(top1, a));
                top1 = fmaxf(top1, a);
              }
            }
          }
          if (!sl_custom) {
            /* The leader so far is known by its stage-1 value run_a; its exact metric is only worked out when somebody comes
             * within the tolerance of it.  A block whose maximum is below (1 - 2^-19) run_a cannot win or tie; otherwise the
             * users at or above (1 - 2^-19) of the larger of the two maxima are the only possible winners: a single one that
             * leaves the old leader below the threshold simply takes over (no division at all -- the common case), several, or
             * one next to a leader still in range, are compared exactly, ascending user order, strict '>'. */
            if (best_a > 0.0f && best_a >= run_a * kTol) {
              const float thr = fmaxf(best_a, run_a) * kTol;
              uint32_t cand = 0;
#pragma unroll
              for (int k = 0; k < kP3Block; ++k) cand |= av[k] >= thr ? (1u << k) : 0u;
              const bool leader_in = run_a >= thr; /* false while there is no leader: thr > 0 */
              if (!leader_in && (cand & (cand - 1u)) == 0u) {
                bu = blk + __ffs((int)cand) - 1;
                run_a = best_a;
                exact = false;
              } else {
                if (leader_in) {
                  if (!exact) best = exact_metric(bu, rowp[bu]);
                } else {
                  best = SCHED == 1 ? 0.0 : (SCHED == 7 ? -1.7976931348623157e308 : -1.0);
                  bu = -1;
                }
                while (cand) {
                  const int j = __ffs((int)cand) - 1;
                  cand &= cand - 1;
                  const int u = blk + j;
                  const double metric = exact_metric(u, rowp[u]);
                  if (metric > best) { best = metric; bu = u; }
                }
                exact = true;
                run_a = *(const float*)((const char*)numtab + ((uint32_t)rowp[bu] << 2)) * rcw[bu];
              }
            }
          } else {
            /* customised slices (drop-in mode only): every survivor of the block is evaluated.  Survivors: a~ >= (1 - 2^-19)
             * max a~ and a~ > 0; with an all-zero block an infinite threshold leaves no survivor */
            const float thr = best_a > 0.0f ? best_a * kTol : __builtin_inff();
            uint32_t cand = 0;
#pragma unroll
            for (int k = 0; k < kP3Block; ++k) cand |= av[k] >= thr ? (1u << k) : 0u;
            /* customised slices can rank every user at 0 (no prioritized data): the reference's scan then
             * keeps the first user (0 > -1), so that user goes to stage 2 */
            if (!cand) {
              if (QUEUE) { /* users without queued data are not in the list: every slot of the slice, the first listed one wins */
#pragma unroll
                for (int k = 0; k < kP3Block; ++k) cand |= (blk + k >= ub && blk + k < ue) ? (1u << k) : 0u;
              } else {
                cand = 1u << ((ub > blk ? ub : blk) - blk);
              }
            }
            while (cand) {
              const int j = __ffs((int)cand) - 1;
              cand &= cand - 1;
              const int u = blk + j;
              const double metric = exact_metric(u, rowp[u]);
              if (metric > best) { best = metric; bu = u; }
            }
            exact = true;
          }
        }
        const int bkey = bu >= 0 ? rowp[bu] : 0;
        if ((SCHED == 1 || nvs_split) && !exact && bu >= 0) best = exact_metric(bu, bkey); /* the winners' metrics meet in P4 */
        bu_out[it] = (uint16_t)bu;
        if constexpr (kHoldSched) {
          /* Held until the next full scan?  The winner's stage-1 value must BE the segment's largest and lead the second
           * largest by mu = 2^-18 + 2 / (1 + avg_w) (DESIGN.md 2.12: 2^-18 covers the stage-1 error on both sides, 2 / (1 + avg_w)
           * what RS_HOLD_MAX_AGE unserved TTIs take from the winner through the "+1" of (1 + avg) / 1000; avg_w >= 64 keeps the
           * clamp at 1 out of reach).  A psi = 0 slice ranks on the CQI alone: its winner stands whoever is served. */
          if (bu >= 0) {
            if (!sl_psi) {
              held = true;
            } else {
              const float la = *(const float*)((const char*)numtab + ((uint32_t)bkey << 2)) * rcw[bu];
              const double aw = s_avg[bu];
              const float mu = 0x1p-18f + 2.0f / (1.0f + (float)aw);
              held = aw >= 64.0 && la >= top1 && top2 * (1.0f + mu) * 1.000001f <= la;
            }
          }
        }
        if (SCHED == 10) {
          /* UpperBound sorts one vector per slice (:229-233): slice-major */
          rec_out[sg * R + r] = ((uint32_t)bkey << 16) | ((uint32_t)r << 8) | (uint32_t)sg;
        } else if (kTransport) {
          /* MaximizeCell's vector is RBG-major, slice-minor (:357-360) */
          rec_out[r * Sn + sg] = ((uint32_t)bkey << 16) | ((uint32_t)r << 8) | (uint32_t)sg;
        } else if (SCHED == 1 || nvs_split) {
          s_best_metric[it] = best;
        }
      }
      return held;
    };
    if constexpr (kQSerial && SCHED == 7) {
      /* m_requiredRBs (packet-scheduler.cpp:319-334): the data of the bearer that created the user's record, in PRBs of the
       * wideband MCS -- EESM over every PRB of the band in order, G identical terms per RBG */
      const int ub = m->seg_begin[seg_lo], ue = m->seg_begin[seg_lo + 1];
      for (int u = ub + tid; u < ue; u += nt) {
        int need = 0;
        if (prio_in[u] & 2) {
          double sum = 0;
          if (per_prb) { /* per-PRB reports: every PRB of the band as the user reported it */
            for (int r = 0; r < R; ++r) {
              const uint8_t* pr = prb_ptr(u, r);
              for (int k = 0; k < G; ++k) sum += s_e[pr[k]];
            }
          } else {
            for (int r = 0; r < R; ++r) {
              const double ev = s_e[s_cqi[r * Upad + u]];
              for (int k = 0; k < G; ++k) sum += ev;
            }
          }
          const double x = sum / (double)(R * G);
          int wide = 15;
          if (!(x == 0)) {
            wide = 1;
#pragma unroll
            for (int k = 1; k <= 13; ++k) wide += (x <= xthr_k[k - 1]) ? 1 : 0;
          }
          const int first = q_data0[u] > 0 ? q_data0[u] : q_data1[u];
          need = (first * 8) / tab->tbs1_of_cqi[wide];
        }
        q_need[u] = need;
      }
      /* The metric of a (user, RBG) pair depends on the RBG through the CQI only: 16 quotients per user of the served slice,
       * divided here by all threads, instead of one division per candidate and RBG on the serial wave (the idle sort buffers
       * hold the table when the slice fits: 128 bytes per user) */
      if (ue - ub <= 64 && (ue - ub) * 128 <= o.items - o.elems) {
        const int sl_eps7 = m->eps_psi[seg_lo] & 1, sl_psi7 = (m->eps_psi[seg_lo] >> 1) & 1;
        const bool custom7 = (m->eps_psi[seg_lo] & 4) != 0;
        double* const qt = (double*)s_elems;
        for (int i = tid; i < (ue - ub) * 16; i += nt) {
          const int u = ub + (i >> 4), cq = i & 15;
          const double num = sl_eps7 ? s_num[cq] : 1.0, den = sl_psi7 ? s_avgk[u] : 1.0;
          qt[i] = !custom7 ? num / den : ((prio_in[u] & 1) == 0 ? 0.0 : hol_in[u] * num / den); /* ref: nvs :375-387 */
        }
      }
    }
    /* ---- one (slice, RBG) item on FOUR LANES: 8 (or 16) users of the slice's zero-padded window per lane, the stage-1 products as in
     * scan_item, the window's two largest by two butterfly steps inside the lane quad, then the lane that holds the only user
     * within 2^-19 of the largest is the `writer` (no division); several such users are compared exactly, ascending, strict '>'
     * (metrics are > 0: their bit patterns order like the values).  Used by the held winners' pass over the listed items and by
     * NVS's scan of the next TTI's slice (rs_phase_next.inc): a ~900-cycle chain instead of scan_item's ~4 000. */
    struct QuadWinner { bool writer; int user, bits; float la, g1, g2; };
    constexpr bool kQuadScan = kHoldSched || kQuad7;
    /* groups of 8 users per lane: one for windows of up to 32 users, two up to 64 (a compile-time fact when the host passed the
     * batch's longest window) */
    constexpr int kMaxGrp = (FIXED && RS_JIT_WIN > 0 && RS_JIT_WIN <= 32) ? 1 : 2;
    auto quad_scan = [&](const bool on, const int sg, const int r) -> QuadWinner {
      const float kTolH = 0x1.ffffcp-1f; /* 1 - 2^-19 */
      const int q4 = lane & 3;
      const int ngrp = kMaxGrp == 1 ? 1 : (hold_win <= 32 ? 1 : 2);
      auto quad_max_i = [&](int v) -> int { /* every lane of the quad gets the quad's maximum: quad_perm [1,0,3,2], [2,3,0,1] */
        int o1 = __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false);
        v = v > o1 ? v : o1;
        int o2 = __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false);
        return v > o2 ? v : o2;
      };
            const int ub = m->seg_begin[sg], ue = m->seg_begin[sg + 1];
            const int bits = m->eps_psi[sg];
            const float* numtab = (bits & 1) ? s_num32 : m->ones16;
            const float* rcw = s_rcp32 + m->rcp_off[sg];
            const uint8_t* rowp = s_cqi + r * Upad;
            const int wend = (ue + 7) & ~7;
            const int u0 = (ub & ~7) + q4 * 8 * ngrp;
            float t1 = 0.0f, t2 = 0.0f; /* my users' largest and second largest stage-1 value */
            float av[8 * kMaxGrp];
#pragma unroll
            for (int g = 0; g < kMaxGrp; ++g) {
              const int ug = u0 + 8 * g;
              uint2 cw = make_uint2(0u, 0u);
              float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
              if (on && g < ngrp && ug < wend) {
                cw = *(const uint2*)(rowp + ug);
                ra = *(const float4*)(rcw + ug);
                rb = *(const float4*)(rcw + ug + 4);
              }
              const float rc[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
              const uint32_t cx4 = cw.x << 2, cy4 = cw.y << 2;
              float nm[8];
#pragma unroll
              for (int k = 0; k < 8; ++k)
                nm[k] = *(const float*)((const char*)numtab + (((k < 4 ? cx4 : cy4) >> (8 * (k & 3))) & 0xffu));
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                const float a = nm[k] * rc[k]; /* 0 outside the slice: zero reciprocals around it */
                av[8 * g + k] = a;
                t2 = fmaxf(t2, fminf(t1, a));
                t1 = fmaxf(t1, a);
              }
            }
            /* the quad's two largest: (t1, t2) pairs meet in two butterfly steps */
            float g1 = t1, g2 = t2;
#pragma unroll
            for (int step = 0; step < 2; ++step) {
              const float o1 = __int_as_float(step == 0 ? __builtin_amdgcn_update_dpp(0, __float_as_int(g1), 0xB1, 0xf, 0xf, false)
                                                        : __builtin_amdgcn_update_dpp(0, __float_as_int(g1), 0x4E, 0xf, 0xf, false));
              const float o2 = __int_as_float(step == 0 ? __builtin_amdgcn_update_dpp(0, __float_as_int(g2), 0xB1, 0xf, 0xf, false)
                                                        : __builtin_amdgcn_update_dpp(0, __float_as_int(g2), 0x4E, 0xf, 0xf, false));
              g2 = fmaxf(fmaxf(g2, o2), fminf(g1, o1));
              g1 = fmaxf(g1, o1);
            }
            /* my users within the tolerance of the window's largest */
            /* (an all-zero window -- only an empty slice, which is never listed -- gets an unreachable threshold instead of a
             * second comparison per user) */
            const float thr = g1 > 0.0f ? g1 * kTolH : __builtin_inff();
            unsigned cm = 0u;
#pragma unroll
            for (int k = 0; k < 8 * kMaxGrp; ++k) cm |= av[k] >= thr ? (1u << k) : 0u;
            int cnt = __popc(cm);
            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0xB1, 0xf, 0xf, false);
            cnt += __builtin_amdgcn_update_dpp(0, cnt, 0x4E, 0xf, 0xf, false);
            bool writer = on && cnt == 1 && cm != 0u;
            int ul = u0 + __ffs((int)cm) - 1; /* (writer: my only survivor) */
            float la = t1;
            if (__ballot(on && cnt > 1) != 0ull) {
              /* several users within the tolerance of each other: the reference's expression, first maximum */
              int bhi = -1, blo = (int)0x80000000, bu_l = 0;
              if (on && cnt > 1) {
                unsigned c2 = cm;
                while (c2) {
                  const int j = __ffs((int)c2) - 1;
                  c2 &= c2 - 1u;
                  const int u = u0 + j;
                  const double metric = ((bits & 1) ? s_num[rowp[u]] : 1.0) / ((bits & 2) ? s_avgk[u] : 1.0);
                  const int hi = __double2hiint(metric), lo = (int)((unsigned)__double2loint(metric) ^ 0x80000000u);
                  if (hi > bhi || (hi == bhi && lo > blo)) { bhi = hi; blo = lo; bu_l = u; } /* metrics > 0: (high, low unsigned) order */
                }
              }
              const int mhi = quad_max_i(bhi);
              const int mlo = quad_max_i(bhi == mhi ? blo : (int)0x80000000);
              const unsigned long long eq = __ballot(on && cnt > 1 && bhi == mhi && blo == mlo);
              const unsigned quad = (unsigned)(eq >> (lane & ~3)) & 0xfu; /* lanes of my quad that reach the maximum: the lowest wins */
              if (on && cnt > 1 && (quad & ((1u << q4) - 1u)) == 0u && ((quad >> q4) & 1u)) {
                writer = true;
                ul = bu_l;
                la = numtab[rowp[bu_l]] * rcw[bu_l];
              }
            }
      return QuadWinner{writer, ul, bits, la, g1, g2};
    };
    (void)kQuadScan;
    bool hold_full = true; /* held winners: this TTI scanned every item (their records are in cur_rec) */
    if constexpr (kHoldSched) {
      /* ---- held winners: scan only what can have changed (DESIGN.md 2.12) ---- */
      /* The items to scan again -- winner not held, or served in the previous TTI (a psi = 0 slice ignores the averages) -- are
       * packed into a wave-private list (items are dealt to the waves round robin: no shared list, no atomics, no workgroup
       * barrier) and scanned FOUR LANES PER ITEM,
       * 8 (or 16) users of the slice's zero-padded window per lane: the stage-1 products as in scan_item, the window's two
       * largest by two-step butterflies inside the lane quad, then the lane that holds the only user within 2^-19 of the
       * largest writes the winner (no division); several such users are compared exactly, ascending, strict '>'.
       * ~60 of 500 items per TTI at the benchmark's shape: one pass of 16 items on every wave. */
      bool full = !hold_ok || tti == 0 || grid_loaded || hold_age >= RS_HOLD_MAX_AGE;
      int hold_listed = 0;
#if defined(RS_STAMPS) && defined(RS_STAMPS_HOLD)
      unsigned long long hs_prev = __builtin_readcyclecounter();
#define RS_HSTAMP(i) do { if (tid == 0) { unsigned long long n_ = __builtin_readcyclecounter(); sort_sub[i] += n_ - hs_prev; hs_prev = n_; } } while (0)
#else
#define RS_HSTAMP(i) do { } while (0)
#endif
      if (!full) {
        const int grp = lane >> 2;
        uint16_t* const wl = hold_wl; /* this wave's list */
        for (int k0 = 0; k0 * nwaves < n_items; k0 += 64) {
          /* (a one-chunk shape: the list may have been packed in the previous TTI's serial phase already) */
          const int n_list = (pre_listed >= 0 && k0 == 0) ? pre_listed : hold_pack(k0, wave);
          hold_listed += n_list;
          RS_HSTAMP(0);
          /* issue priority of the pass (same-box A/B, 512 cells): GreedyByRow 101.4 against 99.7 M TTIs/s at priority 1 -- the
           * co-resident cell is mostly in its one-wave serial phase, which runs at 3 anyway; MaximizeCell 32.8 against 33.7 -- there
           * the pass would take issue slots from the co-resident cell's sort levels (priority 1, a barrier every few dozen
           * instructions) */
          constexpr int kHoldPrio = SCHED == 8 ? 1 : 0;
          if (kHoldPrio) RS_SETPRIO(kHoldPrio);
          for (int base = 0; base < n_list; base += 16) {
            const bool on = base + grp < n_list;
            const int it = on ? (int)wl[base + grp] : 0;
            const int sg = FIXED ? it / RS_JIT_R : idiv_small(it, R), r = it - sg * R;
            const QuadWinner w = quad_scan(on, sg, r);
            const bool writer = w.writer;
            const int ul = w.user, bits = w.bits;
            const float la = w.la, g1 = w.g1, g2 = w.g2;
            const uint8_t* rowp = s_cqi + r * Upad;
            if (writer) {
              const int key = rowp[ul];
              bool held = false;
              if (!(bits & 2)) {
                held = true;
              } else {
                const double aw = s_avg[ul];
                const float mu = 0x1p-18f + 2.0f / (1.0f + (float)aw);
                held = aw >= 64.0 && la >= g1 && g2 * (1.0f + mu) * 1.000001f <= la;
              }
              cur_bu[it] = (uint16_t)ul;
              /* (MaximizeCell rebuilds its records from the winners right before the sort: the sort permutes them in place) */
              if (SCHED != 9) cur_rec[r * Sn + sg] = ((uint32_t)key << 16) | ((uint32_t)r << 8) | (uint32_t)sg;
              /* (item = k * nwaves + wave: bit k & 63 of this wave's word k >> 6; the quads of one wave write it side by side) */
              const int kk = FIXED ? it / (RS_JIT_NT / 64) : idiv_small(it, nwaves);
              unsigned long long* const word = &hold_bits[(kk >> 6) * nwaves + wave];
              if (held) atomicOr(word, 1ull << (kk & 63));
              else atomicAnd(word, ~(1ull << (kk & 63)));
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          if (kHoldPrio) RS_SETPRIO(0);
          RS_HSTAMP(1);
        }
        hold_age += 1;
      }
      if (full) {
        for (int k0 = 0; k0 * nwaves < n_items; k0 += 64) { /* the same dealing of the items as above */
          const int j = (k0 + lane) * nwaves + wave;
          bool held = false;
          if (j < n_items) held = scan_item(j, cur_bu, cur_rec, RsInt<RS_P3_BLOCK_TOP>{});
          const unsigned long long hm = __ballot(held);
          if (hold_ok && lane == 0) hold_bits[(k0 >> 6) * nwaves + wave] = hm;
        }
        hold_age = 0;
      }
      hold_full = full;
      pre_listed = -1;
#ifdef RS_STAMPS
      if (tid == 0) sort_sub[6] += (unsigned long long)hold_listed + ((unsigned long long)(full ? 1 : 0) << 32); /* (wave 0's chunk) */
#endif
    } else
    if constexpr (kPf1) {
      /* ---- per-flow PF, every user backlogged (ref: downlink-packet-scheduler.cpp:221-237, dl-pf-packet-scheduler.cpp:128-140):
       * per RBG the first maximum of (se * 180000.) / avg over ALL users, from 0 with '>'.  The RBGs are dealt out to the waves
       * (RBG nwaves - 1 - wave, + nwaves, ...); a wave holds every user, kUL consecutive ones per lane (their stage-1 reciprocals in
       * registers for the whole TTI), and works on up to four RBGs side by side (independent chains: one wave issues a dependent
       * instruction every ~8.5 cycles, an independent one every ~5.3).  Stage 1 per user: the FP32 product of DESIGN.md 3.2 with the
       * user's position in the lane written into its five low mantissa bits (a relative change below 2^-18, so the filter's
       * tolerance widens from 2^-19 to 2^-16: (1 - 2^-19)(1 - 2^-18)^2 > 1 - 2^-16), the lane's largest and second largest of these
       * words (v_max / v_med3), one DPP reduction per RBG.  An RBG whose largest word leads every other user's by the tolerance is
       * settled on the scalar unit -- winner = (first lane at the maximum, position from the word's low bits), no division; several
       * users within the tolerance are compared with the reference's expression, ascending user id, strict '>'. */
      constexpr int kUL = (((RS_JIT_U + 63) / 64) + 7) & ~7; /* users per lane: lane l owns users kUL * l ... kUL * l + kUL - 1 */
      static_assert(kUL <= 32, "per-flow PF lanes: five position bits");
      const float kTol16 = 0x1.fffep-1f; /* 1 - 2^-16 */
      const int u_first = kUL * lane;
      float rcl[kUL];
#pragma unroll
      for (int q = 0; q < kUL / 4; ++q) {
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u_first + 4 * q < U) rv = *(const float4*)(s_rcp32 + u_first + 4 * q); /* zeros behind the last user (Upad is a multiple of 8) */
        rcl[4 * q] = rv.x; rcl[4 * q + 1] = rv.y; rcl[4 * q + 2] = rv.z; rcl[4 * q + 3] = rv.w;
      }
      /* several users of one RBG within the tolerance `thr` of its largest word: every lane evaluates its own candidates exactly
       * (ascending, strict '>'), the wave takes the largest metric and the lowest lane among equals (= the lowest user id) */
      auto settle_exactly = [&](int r, int thr) -> int {
        const uint8_t* rowp = s_cqi + r * Upad;
        double best = 0.0; /* the scan starts from 0 with '>' */
        int bu = -1;
#pragma unroll 1
        for (int k = 0; k < kUL; ++k) {
          const int u = u_first + k;
          if (u < U) {
            const int c = rowp[u];
            const int w = (__float_as_int(s_num32[c] * s_rcp32[u]) & ~31) | (31 - k);
            if (w >= thr) {
              const double metric = s_num[c] / s_avg[u];
              if (metric > best) { best = metric; bu = u; }
            }
          }
        }
        const int hi = bu >= 0 ? __double2hiint(best) : -1; /* metrics > 0: (high word, low word unsigned) orders like the values */
        const int lo = (int)((unsigned)__double2loint(best) ^ 0x80000000u);
        const int mhi = wave_max(hi);
        const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
        const unsigned long long eq = __ballot(bu >= 0 && hi == mhi && lo == mlo);
        return mhi >= 0 ? __builtin_amdgcn_readlane(bu, __ffsll((long long)eq) - 1) : -1;
      };
      auto scan_rbgs = [&](int r0, auto jtag) {
        constexpr int J = decltype(jtag)::v; /* RBGs r0, r0 + nwaves, ... side by side */
        int top1[J], top2[J];
#pragma unroll
        for (int j = 0; j < J; ++j) { top1[j] = 0; top2[j] = 0; }
#pragma unroll
        for (int g = 0; g < kUL / 8; ++g) {
          uint2 cw[J];
#pragma unroll
          for (int j = 0; j < J; ++j) {
            cw[j] = make_uint2(0u, 0u);
            if (u_first + 8 * g < U) cw[j] = *(const uint2*)(s_cqi + (r0 + j * nwaves) * Upad + u_first + 8 * g);
          }
          /* table reads of all J RBGs first (8 J loads in flight), then the J update chains side by side, user by user */
          float nm[J][8];
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const uint32_t cx4 = cw[j].x << 2, cy4 = cw[j].y << 2; /* CQI <= 15: four table byte offsets per word */
#pragma unroll
            for (int k = 0; k < 8; ++k)
              nm[j][k] = *(const float*)((const char*)s_num32 + (((k < 4 ? cx4 : cy4) >> (8 * (k & 3))) & 0xffu));
          }
#pragma unroll
          for (int j = 0; j < J; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) asm volatile("" : "+v"(nm[j][k]));
#pragma unroll
          for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
              /* (two users per v_pk_mul_f32 measured slower: 158.2 against 161.5 M TTIs/s at 500 UEs) */
              const int w = (__float_as_int(nm[j][k] * rcl[8 * g + k]) & ~31) | (31 - (8 * g + k));
              /* (the second largest costs one of the five vector instructions per (user, RBG) product: without it -- a tie inside one
               * lane would go unnoticed -- the scan measured 173 against 161 M TTIs/s: the phase is bound by instruction issue) */
              int t2;
              asm("v_med3_i32 %0, %1, %2, %3" : "=v"(t2) : "v"(top1[j]), "v"(top2[j]), "v"(w)); /* top1 >= top2: the new second largest */
              top2[j] = t2;
              top1[j] = w > top1[j] ? w : top1[j];
            }
          }
        }
        int mx[J];
#pragma unroll
        for (int j = 0; j < J; ++j) mx[j] = wave_max(top1[j]);
        int mypick = -1; /* lane j: the winner of RBG r0 + j * nwaves */
#pragma unroll
        for (int j = 0; j < J; ++j) {
          /* a word above 31 is a real product (>= 2^-126: numerators are >= 16 000, averages <= 1e12) */
          const int thr = __float_as_int(__int_as_float(mx[j]) * kTol16);
          const unsigned long long holders = __ballot(top1[j] >= thr), multi = __ballot(top2[j] >= thr);
          int bpick = -1;
          if (mx[j] > 31) {
            if (multi == 0ull && __popcll(holders) == 1) bpick = kUL * (__ffsll((long long)holders) - 1) + (31 - (mx[j] & 31));
            else bpick = settle_exactly(r0 + j * nwaves, thr);
          }
          if (lane == j) mypick = bpick;
        }
        if (lane < J) cur_bu[r0 + lane * nwaves] = (uint16_t)mypick; /* 0xFFFF: nobody */
      };
      {
        int r0 = nwaves - 1 - wave; /* (wave 0 runs the serial end of the TTI: it takes the short share when the RBGs do not divide evenly) */
        for (; r0 + 3 * nwaves < R; r0 += 4 * nwaves) scan_rbgs(r0, RsInt<4>{});
        if (r0 + 2 * nwaves < R) scan_rbgs(r0, RsInt<3>{});
        else if (r0 + nwaves < R) scan_rbgs(r0, RsInt<2>{});
        else if (r0 < R) scan_rbgs(r0, RsInt<1>{});
      }
    } else
    if constexpr (SCHED != 11 && !kQSerial) {
     if (!(kEarly17 && have_scan)) { /* (NVS: the winners may be in place already, found during the previous TTI's serial phase) */
      /* fix-up of a speculated TTI: only the items whose speculative winner was served in the previous TTI (listed by the
       * scanning waves) are scanned again, now with the true averages; a list that overflowed means all of them.  One loop
       * for both cases: the scan is inlined once here and once in the serial phase. */
      /* The serial phase scans whole rounds only (every scanning lane one item per round): the items beyond them were not
       * speculated at all and are scanned here, behind the listed ones -- a second, nearly empty round in the serial phase
       * would cost a whole item's latency there, here they ride along in lanes that are idle anyway. */
      const int n_fix = have_spec ? rs_lds_load(&fl_prev->n_fix) : 0;
      const bool listed = have_spec && n_fix <= RS_FIX_CAP;
      const int n_spec = spec_items(n_items); /* items the serial phase speculated: [0, n_spec) */
      const int n_scan = listed ? n_fix + (n_items - n_spec) : n_items;
      for (int j = tid; j < n_scan; j += nt)
        scan_item(listed ? (j < n_fix ? (int)fix_list[j] : n_spec + (j - n_fix)) : j, cur_bu, cur_rec, RsInt<RS_P3_BLOCK_TOP>{});
     }
    }
    /* (an NVS TTI whose averages, slice and winners were all prepared has written nothing since the previous TTI's closing barrier) */
    if (!(kEarly17 && SCHED == 7 && have_scan)) __syncthreads();
    if (kTransport && p.log_keys) {
      /* parity tests only: what the inter-slice step is about to read, [R][S] per TTI: CQI key of the slice's best user
       * (0: no user) | (user + 1) << 8 -- flow_spectraleff / user_index of ref :545-567 */
      for (int i = tid; i < R * S; i += nt) {
        const int r = SCHED == 10 ? i % R : i / S, sg = SCHED == 10 ? i / R : i % S;
        /* (an absent slice has no item and no record: its entries are 0; the records of the others lie Sn to an RBG) */
        const bool absent = ragged_s && sg >= Sn;
        const int bu = absent ? 0xFFFF : (int)cur_bu[sg * R + r];
        const uint32_t key = absent ? 0u : kHoldSched ? (bu == 0xFFFF ? 0u : (uint32_t)s_cqi[r * Upad + bu]) : (cur_rec[(SCHED == 10 || !ragged_s) ? i : r * Sn + sg] >> 16);
        p.log_keys[((size_t)cell * p.n_ttis + tti) * R * S + r * S + sg] = key | ((bu == 0xFFFF ? 0u : (uint32_t)bu + 1u) << 8);
      }
    }
    RS_STAMP(2);

