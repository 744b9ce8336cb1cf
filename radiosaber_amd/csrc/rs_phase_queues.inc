/* rs_phase_queues.inc -- fragment of rs_cell_body (rs_kernels.hip), included inside the function: the queue model (finite MAC queues, two bearers per user; SURVEY 8f N3): scratch pointers, the bearers' words in LDS or HBM, RLC dequeue, DoStopSchedule per user, load of a cell's bearers.  Used when QUEUE (and, the gate scratch, by drop-in PF / NVS contexts). */
  /* queue model scratch in LDS: m->hist is free outside the counting sort (and the speculation, which the queue model does not use) */
  /* schedulers 1 and 7: per-bearer scratch (rs_carve_with) */
  int32_t* const q_grant1 = (int32_t*)(lds + o.queue);   /* [U] sched 1: this TTI's grant of the user's second flow (the first: s_tx) */
  int32_t* const q_data0 = q_grant1 + U;                 /* [U] m_dataToTransmit of bearer 0 (0: no packets) */
  int32_t* const q_data1 = q_data0 + U;                  /* [U] ... of bearer 1 */
  int32_t* const q_need = q_data1 + U;                   /* [U] sched 7: m_requiredRBs minus the PRBs allocated so far */
  uint8_t* const q_done = (uint8_t*)(q_need + U);        /* [2U] sched 1: the flow is satisfied */
  if constexpr (kQSerial) {
    for (int u = tid; u < U; u += nt) q_grant1[u] = 0; /* (a launch ends with every grant consumed) */
    __syncthreads();
  }
  int32_t* const q_slice_prio = (int32_t*)m->hist;      /* [64] highest bearer priority with packets, per slice */
  int32_t* const q_slice_act = (int32_t*)m->hist + 64;  /* [64] the slice has a user with queued data */
  int32_t* const q_any = &m->nvs_slice; /* slices with data this TTI (0: RBsAllocation does not run); read in the serial phase,
                                         * i.e. after the counting sort reused m->hist: its own word (unused by these schedulers) */
    /* ---------------- finite queues (SURVEY 8f N3): the bearers' MAC queues, one thread per user ----------------
   * ref: src/flows/MacQueue.cpp:86-200, src/protocolStack/rlc/um-rlc-entity.cpp:126-196, src/flows/radio-bearer.cpp:281-367,
   * downlink-transport-scheduler.cpp:105-221, packet-scheduler.cpp:305-335.  Per bearer (index = priority) the queue is a
   * window [head, tail) of its uploaded arrival bursts plus the progress inside the head burst; a burst = n_full packets of
   * RS_FULL_PACKET bytes and one last packet.  Order per TTI: DoStopSchedule of the previous TTI (grant split from the highest
   * priority down, RLC dequeue with 8 bytes of overhead per packet, fragmenting the last), EWMA of every bearer, the arrivals
   * up to now, then the user's record (bearers with packets, dataToTransmit, slice priority, head-of-line delay). */
  auto bearer_index = [&](int u, int b) -> size_t { return ((size_t)cell * 2 + b) * U + u; };
  /* the seven 32-bit words of bearer (b, u) -- HBM: seven arrays [cells][2][U] one after the other (RsLaunch::q_head ... b_tx);
   * LDS: [7][2][U] -- and its average */
  enum { QF_HEAD = 0, QF_TAIL = 1, QF_PK = 2, QF_FRAG = 3, QF_BYTES = 4, QF_PKTS = 5, QF_TX = 6 };
  int32_t* const qi_base = !QUEUE ? nullptr : (q_lds ? qs_i : p.q_head + (size_t)cell * 2 * U);
  const size_t qi_stride = !QUEUE ? 0 : (q_lds ? (size_t)2 * U : (size_t)p.n_cells * 2 * U);
  double* const qavg_base = !QUEUE ? nullptr : (q_lds ? qs_avg : p.b_avg + (size_t)cell * 2 * U);
  const uint8_t* const kind_of = !QUEUE ? nullptr : (q_lds ? qs_kind : p.bearer_kind);   /* [U][2] */
  const uint8_t* const slice_of = (QUEUE && q_lds) ? qs_slice : p.user_slice;
  uint8_t* const q_fl = !QUEUE ? nullptr : (q_lds ? qs_flags : p.q_flags + (size_t)cell * U);
  double* const q_ho = !QUEUE ? nullptr : (q_lds ? qs_hol : p.q_hol + (size_t)cell * U);
  auto QI = [&](int f, int b, int u) -> int32_t& { return qi_base[(size_t)f * qi_stride + b * U + u]; };
  auto queue_data = [&](int kind, int b, int u) -> int { /* m_dataToTransmit of a bearer with packets, else 0 */
    if (kind == 1) return 100000000;
    if (kind != 2) return 0;
    const int pk = QI(QF_PKTS, b, u);
    return pk > 0 ? QI(QF_BYTES, b, u) + 8 * pk : 0; /* GetQueueSizeWithMACHoverhead */
  };
  /* RadioBearer::m_cumulativeBytes / m_cumulativeRBs stay in HBM: touched for served bearers only, fire-and-forget adds */
  auto cum_add = [&](int64_t* w, long long v) { (void)atomicAdd((unsigned long long*)w, (unsigned long long)v); };
  /* ... unless the thread owns exactly one user (shape-specialised build, U <= threads): then a launch's counts ride in six
   * registers of the owner thread -- stop_schedule_user is only ever run by the owner -- and reach HBM once, at the end of the
   * launch (round 4: these atomics were the queue mode's 3.2 KB of extra HBM traffic per cell-TTI, profiles/queue_mode.json) */
  constexpr bool kQCumRegs = FIXED && QUEUE && RS_JIT_U <= RS_JIT_NT;
  int qc_bytes[2] = {0, 0}, qc_rbs[2] = {0, 0}, qc_ubytes = 0, qc_urbs = 0; /* 32-bit per launch (RS_MAX_TTIS_PER_LAUNCH) */
  auto count_bearer = [&](int u, int b, int bytes, int nprb) {
    if constexpr (kQCumRegs) {
      qc_bytes[b] += bytes; /* (b is the index of a two-trip loop: unrolled, static) */
      qc_rbs[b] += nprb;
    } else {
      const size_t bi = bearer_index(u, b);
      cum_add(&p.b_cumb[bi], bytes);
      cum_add(&p.b_cumr[bi], nprb);
    }
  };
  auto count_user = [&](int u, long long bytes, long long rbs) {
    if constexpr (kQCumRegs) {
      qc_ubytes += (int)bytes;
      qc_urbs += (int)rbs;
    } else {
      cum_add(&p.cum_bytes[(size_t)cell * U + u], bytes); /* per-user totals for rs_batch_slice_bytes / read_state */
      cum_add(&p.cum_rbs[(size_t)cell * U + u], rbs);
    }
  };
  /* DoStopSchedule of TTI k runs at the top of TTI k + 1 (or at the end of the launch): the TTI it belongs to is n_done - 1 then, and
   * its clock value is kept here (t_k exactly, not t_{k+1} - 0.001) */
  double q_stop_t = t;
  /* one bearer's RLC dequeue of `sent` bytes (TransmissionProcedure): whole packets cost their data + 8 bytes, the last one may
   * leave as a fragment.  A burst is one InternetFlow flow (InternetFlow::Send): where its last packet leaves, whole or as its last
   * fragment, the flow completion record gets the TTI and its clock (um-rlc-entity.cpp:143-160, "ipflow end") -- one store each */
  auto rlc_dequeue = [&](int u, int b, int sent) {
    int left = sent, head = QI(QF_HEAD, b, u), pk = QI(QF_PK, b, u), frag = QI(QF_FRAG, b, u), qb = QI(QF_BYTES, b, u), qp = QI(QF_PKTS, b, u);
    const int head0 = head;
    const size_t a0 = q_lds ? (size_t)qs_a0[b * U + u] : (size_t)p.arr_off[(size_t)(cell * U + u) * 2 + b];
    /* the head burst's shape: cached beside the queue words (LDS) or read where it lies */
    int nfull = 0, last = 0;
    if (left > 8 && qp > 0) {
      nfull = q_lds ? qs_hnf[b * U + u] : p.arr_nfull[a0 + head];
      last = q_lds ? qs_hla[b * U + u] : p.arr_last[a0 + head];
    }
    while (left > 8 && qp > 0) {
      const int size_cur = pk < nfull ? RS_FULL_PACKET : last;
      const int data_cur = size_cur - frag;
      if (data_cur + 8 > left) { /* fragment */
        frag += left - 8;
        qb -= left - 8;
        left = 0;
        break;
      }
      left -= data_cur + 8;
      qb -= data_cur;
      qp -= 1;
      frag = 0;
      pk += 1;
      if (pk < nfull) { /* a run of untouched full packets leaves in one step */
        int k = left / (RS_FULL_PACKET + 8);
        k = k < nfull - pk ? k : nfull - pk;
        left -= k * (RS_FULL_PACKET + 8);
        qb -= k * RS_FULL_PACKET;
        qp -= k;
        pk += k;
      }
      if (pk >= nfull + (last > 0 ? 1 : 0)) {
        if (p.flow_tti) {
          p.flow_tti[a0 + head] = (int32_t)(n_done - 1);
          p.flow_time[a0 + head] = q_stop_t;
        }
        head += 1;
        pk = 0;
        if (qp > 0) { nfull = p.arr_nfull[a0 + head]; last = p.arr_last[a0 + head]; } /* (packets left: the next burst exists) */
      }
    }
    QI(QF_HEAD, b, u) = head; QI(QF_PK, b, u) = pk; QI(QF_FRAG, b, u) = frag; QI(QF_BYTES, b, u) = qb; QI(QF_PKTS, b, u) = qp;
    if (q_lds && head != head0 && qp > 0) {
      qs_headt[b * U + u] = p.arr_time[a0 + head];
      qs_hnf[b * U + u] = nfull;
      qs_hla[b * U + u] = last;
    }
  };
  /* logged launches: one row per (TTI, user, bearer) -- the bytes DoStopSchedule credited and RadioBearer::GetHeadOfLinePacketDelay
   * at that moment, before the RLC dequeue (radio-bearer.cpp:282-307: 0 with an empty MAC queue or an InfiniteBuffer bearer, else
   * now - the head packet's time stamp, at least 1e-5; the slice-priority bearer's value is the q_ho its metric used in that TTI) */
  auto bearer_hol = [&](int u, int b, int kind) -> double { /* the one expression both outputs below carry */
    double hol = 0.0;
    if (kind == 2 && QI(QF_BYTES, b, u) != 0) {
      const double head_time = q_lds ? qs_headt[b * U + u]
                                     : p.arr_time[(size_t)p.arr_off[(size_t)(cell * U + u) * 2 + b] + QI(QF_HEAD, b, u)];
      hol = q_stop_t - head_time;
      if (hol < 0.00001) hol = 0.00001;
    }
    return hol;
  };
  /* ... and unlogged launches that were asked for records (rs_batch_run_records): one RsBearerRecord per credited bearer instead of
   * the dense rows.  The record block rides in the launch block's grp_sent / grp_sent_stride (rs_device.h; null in every other
   * launch): per cell a list of grp_sent_stride places, and behind all lists the cells' count words, zeroed by the host.  A place comes
   * from the cell's count word, one add per credited bearer by the thread that credits it -- stop_schedule_user runs under a
   * per-thread user loop whose trips differ between the lanes of a wave, so there is no ballot to aggregate; workgroup scope, the
   * workgroup owns the cell.  All places of TTI k are handed out before any of TTI k + 1 (barriers lie between); inside a TTI they
   * come as the threads arrive, and the host sorts.  A place at or behind the capacity is not written: the count tells the host.
   * (Block, capacity and count word are formed from the launch block where a record is written, like p.flow_tti in rlc_dequeue:
   * nothing of them stays live across the TTI.) */
  auto log_bearer = [&](int u, int b, int kind, int bytes, int nprb, int row) {
    const bool dense = p.log_bbytes && row >= 0;
    if (!dense && !p.grp_sent) return;
    const double hol = bearer_hol(u, b, kind);
    if (dense) {
      const size_t i = (((size_t)cell * p.n_ttis + row) * U + u) * 2 + b;
      p.log_bbytes[i] = bytes;
      p.log_bhol[i] = hol;
    }
    if (p.grp_sent) {
      /* The TTI is n_done - 1, as the flow completion record takes it, whatever `row` says: row < 0 is DoStopSchedule at the top of a
       * launch's first TTI, and it finds no grant -- a launch ends with every grant consumed (the loop behind the last TTI), a fresh
       * batch has none -- so every record of a launch belongs to one of its own TTIs. */
      RsBearerRecord* const lists = (RsBearerRecord*)p.grp_sent;
      const size_t cap = (size_t)p.grp_sent_stride;
      uint32_t* const count = (uint32_t*)(lists + (size_t)p.n_cells * cap) + cell;
      const uint32_t place = __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if ((size_t)place < cap) {
        int4* const dst = (int4*)(lists + (size_t)cell * cap + place);
        dst[0] = make_int4((int)(n_done - 1), u, b, bytes);
        dst[1] = make_int4(nprb, 0, __double2loint(hol), __double2hiint(hol));
      }
    }
  };
  /* row: the launch's TTI whose grant this is (its log row) */
  auto stop_schedule_user = [&](int u, int row) {
    if constexpr (SCHED == 1) {
      /* DL_PF_PacketScheduler::DoStopSchedule (dl-pf-packet-scheduler.cpp:60-125): every flow is credited its own transport
       * block in full and hands it to its RLC */
      long long user_bytes = 0, user_rbs = 0;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        int32_t* slot = b == 0 ? &s_tx[u] : &q_grant1[u];
        const int grant = *slot;
        if (grant == 0) continue;
        *slot = 0;
        const int bytes = grant & RS_TX_BYTES_MASK, nprb = (grant >> RS_TX_NPRB_SHIFT) & RS_TX_NPRB_MASK;
        QI(QF_TX, b, u) += bytes;
        count_bearer(u, b, bytes, nprb);
        user_bytes += bytes;
        user_rbs += nprb;
        const int kind = kind_of[u * 2 + b];
        log_bearer(u, b, kind, bytes, nprb, row);
        if (kind == 2) rlc_dequeue(u, b, bytes);
      }
      if (user_bytes) count_user(u, user_bytes, user_rbs);
      return;
    }
    const int grant = s_tx[u];
    if (grant == 0) return;
    s_tx[u] = 0;
    int avail = grant & RS_TX_BYTES_MASK;
    const int nprb = (grant >> RS_TX_NPRB_SHIFT) & RS_TX_NPRB_MASK;
    long long user_bytes = 0;
#pragma unroll
    for (int b = 1; b >= 0; --b) {
      if (avail <= 0) break;
      const int kind = kind_of[u * 2 + b];
      const int data = queue_data(kind, b, u);
      if (data <= 0) continue;
      const int sent = avail < data ? avail : data;
      avail -= sent;
      QI(QF_TX, b, u) += sent;
      count_bearer(u, b, sent, nprb);
      user_bytes += sent;
      log_bearer(u, b, kind, sent, nprb, row);
      if (kind == 2) rlc_dequeue(u, b, sent);
    }
    if (user_bytes) count_user(u, user_bytes, nprb);
  };
  if constexpr (QUEUE) {
    if (q_lds) {
      /* load the bearers of this cell: every thread the users it owns in P1 (the only writer of these words) */
      const double kNever = __builtin_inf();
      for (int u = tid; u < U; u += nt) {
        for (int b = 0; b < 2; ++b) {
          const size_t bi = bearer_index(u, b);
          const int kind = p.bearer_kind[u * 2 + b];
          qs_kind[u * 2 + b] = (uint8_t)kind;
          qs_avg[b * U + u] = p.b_avg[bi];
          const size_t n = (size_t)p.n_cells * 2 * U;
#pragma unroll
          for (int f = 0; f < 7; ++f) qs_i[(f * 2 + b) * U + u] = p.q_head[(size_t)f * n + bi];
          double next = kNever, headt = 0.0;
          long long a0 = 0;
          int n_arr = 0, hnf = 0, hla = 0;
          if (kind == 2) {
            a0 = (long long)p.arr_off[(size_t)(cell * U + u) * 2 + b];
            n_arr = (int)((long long)p.arr_off[(size_t)(cell * U + u) * 2 + b + 1] - a0);
            const int tail = p.q_tail[bi];
            if (tail < n_arr) next = p.arr_time[a0 + tail];
            if (p.q_pkts[bi] != 0) {
              const int head = p.q_head[bi];
              headt = p.arr_time[a0 + head];
              hnf = p.arr_nfull[a0 + head];
              hla = p.arr_last[a0 + head];
            }
          }
          qs_next[b * U + u] = next;
          qs_headt[b * U + u] = headt;
          qs_a0[b * U + u] = a0;
          qs_narr[b * U + u] = n_arr;
          qs_hnf[b * U + u] = hnf;
          qs_hla[b * U + u] = hla;
        }
        qs_slice[u] = p.user_slice[u];
        qs_flags[u] = 0;
        qs_hol[u] = 0.0;
      }
      __syncthreads();
    }
  }
