/* rs_phase_next.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: what the waves other than wave 0 do during the serial end: prepare TTI t+1 -- NVS slice pick and scan (kEarly17), EWMA decay, next quotas and pre-packed lists (held winners), or round 2's speculative scan with its served check (kSpecSched). */
    /* ---- the next epoch's CQI grid, fetched beside wave 0 (kGridAhead): the loads are issued first, the LDS writes come last ---- */
    constexpr int kGaN16 = FIXED ? rs_round_up(kCv.Upad * RS_JIT_R, 16) / 16 : 1;
    constexpr int kGaLanes = FIXED ? (RS_JIT_NT > 64 ? RS_JIT_NT - 64 : 64) : 1;
    constexpr int kGaRegs = FIXED ? (kGaN16 + kGaLanes - 1) / kGaLanes : 1; /* 16-byte words per scanning thread */
    constexpr bool kGaRegForm = FIXED && kGaRegs <= 6;
    uint4 ga_buf[kGaRegForm ? kGaRegs : 1];
    const uint4* const ga_src = (kGridAhead && grid_next)
        ? (const uint4*)(p.epochs + ((size_t)cell * p.n_epochs + (size_t)epoch_next) * p.grid_stride) : nullptr;
    if (kGridAhead && grid_next && wave != 0) {
      if constexpr (kGaRegForm) {
#pragma unroll
        for (int j = 0; j < kGaRegs; ++j) {
          const int i = tid - 64 + j * kGaLanes;
          ga_buf[j] = i < kGaN16 ? ga_src[i] : make_uint4(0u, 0u, 0u, 0u);
        }
      }
    }
    if (kEarly17 && SCHED == 7 && early17 && wave == quota_wave) {
      /* SelectSliceToServe of TTI t+1 first: the scanning waves wait for it */
      nvs_pick(nvs_word_nxt);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) atomicExch(&fl_cur->n_fix, 1);
    }
    if (((kHoldSched && ewma_next) || early17) && wave != 0) {
      const int nsp = nt - 64, me = tid - 64;
      for (int u = me; u < Un; u += nsp) {
        double a = s_avg[u];
        if (a < 1) a = 1;
        const double beta = 0.02;
        const double us = (1 - beta) * a;
        if (SCHED == 1) {
          /* the per-flow PF scheduler divides by s_avg itself: it keeps the clamped value, the raw product waits in s_avgk (unused
           * by this scheduler) for wave 0 */
          s_avgk[u] = us;
          s_avg[u] = us < 1 ? 1.0 : us;
          s_rcp32[u] = __builtin_amdgcn_rcpf((float)(us < 1 ? 1.0 : us));
        } else {
          s_avg[u] = us; /* unclamped: a served user's exact update adds beta * rate to it */
          pf_terms(u, us < 1 ? 1.0 : us);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) atomicAdd(&fl_cur->ctr_p1, 1);
    }
    if (kEarly17 && SCHED == 7 && early17) {
      /* TTI t+1's slice is known once the quota wave has published it; its metric scan can run now when that slice is not the one
       * wave 0 is serving (then no average it reads changes any more) and TTI t+1 reads this CQI grid */
      if (wave != 0) {
        while (rs_lds_load(&fl_cur->n_fix) < 1) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int seg_next = rs_lds_load(nvs_word_nxt);
        if (early_scan_ok && seg_next != seg_this) {
          /* every decayed average first (the scan reads other threads' users), and wave 0 must have read TTI t's winners */
          while (rs_lds_load(&fl_cur->ctr_p1) < nwaves - 1) __builtin_amdgcn_s_sleep(1);
          while (rs_lds_load(&fl_cur->greedy_done) < 1) __builtin_amdgcn_s_sleep(1);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          seg_lo = seg_next; /* (this wave's copies: wave 0 keeps TTI t's; everybody re-reads them at the top of TTI t+1) */
          int n_next = o.n_items;
          if (nvs_split) {
            nvs_lo = m->seg_begin[seg_lo];
            nvs_hi = m->seg_begin[seg_lo + 1];
            nvs_first = nvs_lo & ~7;
            nvs_runs = idiv_small(nvs_hi - nvs_first + nvs_seg - 1, nvs_seg);
            n_next = R * nvs_runs;
          }
          if constexpr (kQuad7) {
            /* sixteen RBGs per scanning wave and pass, four lanes each (the whole slice is one window) */
            for (int r0 = (wave - 1) * 16; r0 < R; r0 += 16 * (nwaves - 1)) {
              const int r = r0 + (lane >> 2);
              const bool on = r < R;
              const QuadWinner w = quad_scan(on, seg_lo, on ? r : 0);
              if (w.writer) cur_bu[r] = (uint16_t)w.user;
            }
          } else {
            const int nsp = nt - 64, me = tid - 64;
            for (int it = me; it < n_next; it += nsp) scan_item(it, cur_bu, cur_rec, RsInt<0>{});
          }
        }
      }
    }
    if (quota_next && wave == quota_wave) {
      /* TTI t+1's draws and remainder rotations need nothing of TTI t (unless the error model's draws, one per UE served, come
       * first on the shared stream); its targets need the slice offsets wave 0 publishes with the allocation */
      if (!p.phy_draws) quota_draws(0);
      const int need_stage = p.phy_draws ? 2 : 1;
      while (rs_lds_load(&fl_cur->greedy_done) < need_stage) __builtin_amdgcn_s_sleep(RS_SPEC_NAP);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (p.phy_draws) quota_draws(rs_lds_load(&m->served));
      quota_targets();
    }
    if (prelist_next && wave != 0) {
      /* my list for TTI t+1 (the held bits, the winners and -- once wave 0 has published it -- the served set are what the top
       * of TTI t+1 would read; if that TTI turns out to scan everything, the list is simply not used) */
      while (rs_lds_load(&fl_cur->greedy_done) < 2) __builtin_amdgcn_s_sleep(RS_SPEC_NAP);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      pre_listed = hold_pack(0, wave);
      /* wave 0 is busy until the TTI ends: wave 1 packs its list too (the count travels in an LDS word) */
      if (wave == 1) {
        const int n0 = hold_pack(0, 0);
        if (lane == 0) m->pad[1] = n0;
      }
    }
    if (kSpecSched && spec_next && wave != 0) {
      /* ---------------- the other waves meanwhile: TTI t+1 as if nobody were served in TTI t ---------------- */
      const int nsp = nt - 64, me = tid - 64; /* scanning threads and my index among them */
#if defined(RS_STAMPS) && defined(RS_STAMPS_W1)
      stamp1_prev = __builtin_readcyclecounter();
#endif
      RS_SETPRIO(RS_SPEC_PRIO);
      /* P1: avg' = (1 - beta) * avg + beta * 0 = (1 - beta) * avg exactly; the unclamped product stays in s_avg (a served
       * user's exact update adds beta * rate to it), the PF terms use the clamped value */
      for (int u = me; u < Un; u += nsp) {
        double a = s_avg[u];
        if (a < 1) a = 1;
        const double beta = 0.02;
        const double us = (1 - beta) * a;
        s_avg[u] = us;
        pf_terms(u, us < 1 ? 1.0 : us);
      }
      RS_STAMP1(0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) atomicAdd(&fl_cur->ctr_p1, 1);
      while (rs_lds_load(&fl_cur->ctr_p1) < nwaves - 1) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      RS_STAMP1(1);
      /* P3 on the speculative state */
      const int n_spec = spec_items(n_items);
      for (int it = me; it < n_spec; it += nsp) scan_item(it, nxt_bu, nxt_rec, RsInt<0>{});
      /* TTI t+1's draws and remainder rotations need nothing of TTI t (unless the error model's draws, one per UE served,
       * come first on the shared stream) */
      if (wave == quota_wave && !p.phy_draws) quota_draws(0);
      /* which of my winners were served?  (wave 0 publishes the served set as soon as the allocation is decided) */
      RS_STAMP1(2);
      if (wave == quota_wave) {
        /* TTI t+1's quotas as soon as TTI t's slice offsets are final (with the error model's draws on the stream: once the
         * served count is known too); wave 0 will wait for this wave, so it runs at wave 0's priority from here on */
        RS_SETPRIO(3);
        const int need_stage = p.phy_draws ? 2 : 1;
        while (rs_lds_load(&fl_cur->greedy_done) < need_stage) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (p.phy_draws) quota_draws(rs_lds_load(&m->served));
        quota_targets();
        RS_STAMP1(5);
      }
      while (rs_lds_load(&fl_cur->greedy_done) < 2) __builtin_amdgcn_s_sleep(RS_SPEC_NAP);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      RS_STAMP1(3);
      for (int it0 = (wave - 1) * 64; it0 < n_spec; it0 += nsp) {
        const int it = it0 + lane;
        bool need = false;
        if (it < n_spec) {
          const int w = nxt_bu[it];
          need = w != 0xFFFF && ((served_bits[w >> 5] >> (w & 31)) & 1u) != 0u;
        }
        const unsigned long long mk = __ballot(need);
        if (mk != 0ull) {
          int base = 0;
          if (lane == 0) base = atomicAdd(&fl_cur->n_fix, __popcll(mk));
          base = __builtin_amdgcn_readfirstlane(base);
          const int slot = base + __popcll(mk & ((1ull << lane) - 1ull));
          if (need && slot < RS_FIX_CAP) fix_list[slot] = (uint16_t)it;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) atomicAdd(&fl_cur->ctr_p3, 1);
      RS_STAMP1(4);
    }
    if (kGridAhead && grid_next && wave != 0) {
      while (rs_lds_load(&m->grid_free) < tti + 1) __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if constexpr (kGaRegForm) {
#pragma unroll
        for (int j = 0; j < kGaRegs; ++j) {
          const int i = tid - 64 + j * kGaLanes;
          if (i < kGaN16) ((uint4*)s_cqi)[i] = ga_buf[j];
        }
      } else {
        const int n16 = (int)(p.grid_stride >> 4);
        for (int i = tid - 64; i < n16; i += nt - 64) ((uint4*)s_cqi)[i] = ga_src[i];
      }
    }
