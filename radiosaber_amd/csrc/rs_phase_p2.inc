/* rs_phase_p2.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: P2 on the quota wave: the transport schedulers' quotas (two rand() rotations, C truncation) in two halves, or NVS SelectSliceToServe. */
    /* ---------------- P2: quotas / slice choice (one wave, lanes = slices) ---------------- */
    /* the quota phase of the transport schedulers in two halves: the draws and the two rotations (which slice receives
     * the remainders) depend on the rand() stream only; the targets need slice_rbs_offset_ of the previous TTI.  In a
     * speculated TTI the quota wave runs the first half while wave 0 is still deciding the allocation. */
    bool q_has = false;
    int q_nonempty = 0;
    bool q_first0 = false, q_first1 = false; /* my slice receives the remainder of the PRBs / of the RBGs */
    auto quota_draws = [&](int served_before) {
      /* ref: :463-521 */
      const bool in = lane < Sn;
      q_has = in && (QUEUE ? q_slice_act[lane] != 0 : (m->seg_begin[lane + 1] > m->seg_begin[lane]));
      q_nonempty = __popcll(__ballot(q_has));
      if (QUEUE && lane == 0) *q_any = q_nonempty;
      int r0 = p.rand0, r1 = p.rand1;
      if (!kDirect && !(QUEUE && q_nonempty == 0)) { /* (no user with queued data: RBsAllocation does not run, :160-165) */
        if (p.phy_draws)
          for (int i = 0; i < served_before; i++) (void)rng.next();
        r0 = rng.next();
        r1 = rng.next();
      }
      /* first non-empty slice in the rotation k = (i + rand) % S, i = 0..S-1 (num_slices_ is the cell's own count: Sn) */
      const int r0m = (int)((unsigned)r0 % (unsigned)Sn), r1m = (int)((unsigned)r1 % (unsigned)Sn);
      int pos0 = lane - r0m;
      pos0 = pos0 < 0 ? pos0 + Sn : pos0;
      pos0 = q_has ? pos0 : 1 << 20;
      q_first0 = pos0 == wave_min(pos0);
      int pos1 = lane - r1m;
      pos1 = pos1 < 0 ? pos1 + Sn : pos1;
      pos1 = q_has ? pos1 : 1 << 20;
      q_first1 = pos1 == wave_min(pos1);
    };
    auto quota_targets = [&]() {
      const bool in = lane < Sn;
      int target = 0;
      if (q_has) target = (int)(nb_rbs * s_w[lane] + s_sstate[lane]);
      int extra = nb_rbs - wave_sum(target);
      if (QUEUE && q_nonempty == 0) { /* nothing to schedule this TTI */
        m->target[lane] = 0;
        m->quota[lane] = 0;
        return;
      }
      const int share = idiv_small(extra, q_nonempty), rem = extra - share * q_nonempty; /* C '/' and '%' */
      if (q_has) {
        target += share;
        if (q_first0) target += rem;
      }
      int quota = in ? idiv_small(target, G) : 0;
      int extra_g = R - wave_sum(quota);
      const int share_g = idiv_small(extra_g, q_nonempty), rem_g = extra_g - share_g * q_nonempty;
      if (q_has) {
        quota += share_g;
        if (q_first1) quota += rem_g;
      }
      m->target[lane] = target;
      m->quota[lane] = quota;
    };
    /* SelectSliceToServe (one wave, lanes = slices); also called one TTI ahead, during the previous TTI's serial phase (kEarly17) */
    auto nvs_pick = [&](int32_t* slice_out) {
        /* SelectSliceToServe, ref: downlink-nvs-scheduler.cpp:94-142 */
        int pick;
        if (kDirect) {
          pick = 0; /* the caller passes only the served slice's users */
        } else {
          const bool in = lane < Sn;
          /* slices with queued data (ref: :101-121; with queues: a bearer with packets and dataToTransmit > 0) */
          const bool has = in && (QUEUE ? q_slice_act[lane] != 0 : (m->seg_begin[lane + 1] > m->seg_begin[lane]));
          double ew = in ? s_sstate[lane] : 1.0;
          unsigned long long zero = __ballot(has && ew == 0);
          unsigned long long hasm = __ballot(has);
          /* a zero-ewma slice ends the scan and wins outright; otherwise '>=' keeps the LAST maximum */
          if (zero) {
            pick = __ffsll((long long)zero) - 1;
          } else {
            /* scores are >= 0 (-1 for a slice without users), so they order like the integer pair (high word signed, low
             * word unsigned): two DPP max reductions instead of a shuffle tree on doubles */
            const double score = has ? s_w[lane] / ew : -1.0;
            const int hi = __double2hiint(score);
            const int lo = (int)((unsigned)__double2loint(score) ^ 0x80000000u);
            const int mhi = wave_max(hi);
            const int mlo = wave_max(hi == mhi ? lo : (int)0x80000000);
            const unsigned long long top = __ballot(hi == mhi && lo == mlo) & hasm;
            pick = top ? 63 - __clzll((long long)top) : 0;
          }
          const double beta = 0.01;
          if (has) {
            double e2 = (1 - beta) * ew;
            if (lane == pick) e2 += beta * 1;
            s_sstate[lane] = e2;
          }
        }
        if (lane == 0) *slice_out = pick;
        m->target[lane] = 0;
        m->quota[lane] = 0;
    };
    /* the served slice's word, by TTI parity when picks are made a TTI ahead: a TTI that starts without a barrier may still be
     * reading its own while the quota wave already writes the next one's */
    int32_t* const nvs_word_cur = (kEarly17 && (tti & 1)) ? &m->pad[0] : &m->nvs_slice;
    int32_t* const nvs_word_nxt = (kEarly17 && !(tti & 1)) ? &m->pad[0] : &m->nvs_slice;
    auto quota_phase = [&](int served_before) {
      if (!kTransport && !kDirect && p.phy_draws)
        for (int i = 0; i < served_before; i++) (void)rng.next();
      if (kTransport) {
        quota_draws(served_before);
        quota_targets();
      } else if (SCHED == 7 || SCHED == 11) {
        nvs_pick(nvs_word_cur);
      } else {
        m->target[lane] = 0;
        m->quota[lane] = 0;
      }
    };
    if (wave == quota_wave && !have_spec && !have_quota) quota_phase(served_prev);
    if (kEarly17 && SCHED == 7 && have_quota && wave == quota_wave && p.phy_draws) /* the pick was made a TTI ahead; the error model's */
      for (int i = 0; i < served_prev; i++) (void)rng.next();                       /* draws (one per user served) still come first   */
    int seg_lo = 0;   /* NVS: the served slice */
    int nvs_runs = 1; /* sched 7: runs of the served slice scanned in P3 */
    if (SCHED == 7 || SCHED == 11) {
      if (!(kEarly17 && have_quota)) __syncthreads(); /* P3 scans the slice P2 picked (a pick made a TTI ahead lies behind that TTI's closing barrier) */
      seg_lo = kDirect ? 0 : *nvs_word_cur;
    }
    const int seg_this = seg_lo; /* (the scanning waves of an NVS cell move seg_lo on to the next TTI's slice in the serial phase) */
    RS_STAMP(1);

