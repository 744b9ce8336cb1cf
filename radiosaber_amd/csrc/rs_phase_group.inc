/* rs_phase_group.inc -- one TTI for a group of drop-in cells in one launch (rs_group_schedule_tti): workgroup k serves call slot k.  It reads the slot's
 * header (which cell, how many users, the rand() pair, where the slot's arrays lie, what to do with the cell's CQI image), moves every
 * per-cell pointer of the launch block to its slot / its cell and runs the one-TTI body on that block -- the phases never learn that other cells exist.
 * Completion: every thread's outputs are out at system scope (fence), then the workgroup counts itself in on a device word; the
 * workgroup that brings the count to the number of slots -- the last to finish, whichever it is and whenever the others ran: nothing
 * here assumes that the workgroups are resident together -- puts the word back to 0 for the next launch and publishes the call's
 * sequence number to the host.  Its acquire of the counter orders it behind every other workgroup's fence and release.
 *
 * The entry points of rs_kernels.hip include this text as their body, as rs_cell_body includes its phases: the six kernel templates
 * built into the library (shape in the launch block) and the <name>_jit entry point of a group's run-time builds.  (Text, not a
 * function of its own: the built-in instantiations must stay the machine code they were, and a wrapper function around the inlined
 * cell body changed their instruction counts.)  The includer provides `p` (the launch block), `lds` and five constants:
 *   kGrpForm             the form of the call, a row of rs_group_form (rs_device.h): the table says which of the texts below a form
 *                        takes (res, que, cnt, flow, run), which launch-block pointers they dereference, and which schedulers it has
 *                        kernels for; with a fact false none of its text reaches the instantiation
 *   kGrpSched, kGrpEpt   the body's scheduler and sort form
 *   kGrpFixed            a run-time build: shape, workgroup size and LDS carve are the constants RS_JIT_* -- RS_JIT_U being the user
 *                        CAPACITY while the users of a slot stay the slot header's word --, so the updates' ranges, the stores' strides,
 *                        the loop strides and the LDS offsets below are constants too.  Order of operations and arithmetic are the
 *                        same in both kinds of kernel, in every form.  (The update of the averages stands written out in each of the
 *                        four texts that have one, and each text sets up its own shape words: one helper function for the update,
 *                        and one preamble for the shape words, each changed instruction streams -- profiles/group_forms_table.md.)
 *   kGrpLean             the plain call's per-launch options are constants too (the slots' HoL delays and priority flags are not read)
 *
 * res (rs_group_schedule_tti_at): the cell keeps its users' PF averages, the bytes granted since their last update and the time of that
 *   update in HBM.  Before the body the workgroup applies RadioBearer::UpdateAverageTransmissionRate to EVERY user of the cell
 *   (ref: src/flows/radio-bearer.cpp:139-164, the operations of rs_phase_p0_p1.inc's batch EWMA in their order), hands the body the
 *   averages of the call's users, and behind the body adds each served user's grant -- which the one-TTI body leaves per call position
 *   in LDS (s_tx, rs_phase_p5.inc) -- to the user's pending bytes.
 * que (rs_group_schedule_tti_queued; never with res): the cell keeps BOTH bearers of every user -- average, pending bytes, existence --
 *   and the slot brings m_dataToTransmit[2] per call position.  The update strides over the 2 U bearers, the call's averages are the
 *   sums over the bearers with data, the grant is split over the bearers from the highest priority down (DoStopSchedule), and a slot
 *   without users (U = 0 in its header) does the update alone: the body and the credit are skipped, uniformly for the workgroup.
 * cnt (rs_group_schedule_tti_counted; only with que): the cell also keeps m_cumulateBytes / m_cumulateRBs of both bearers of every
 *   user, and the slot gets back the bytes sent per call position and bearer.  All of it sits in step 4's per-position loop: the thread
 *   that credits a bearer adds the bytes and the position's allocated PRBs to the bearer's 64-bit counters and writes the position's
 *   row of the slot's sent block.  The PRB count is G times the RBGs the position holds -- the body's link adaptation leaves, per call
 *   position, the set of RBG lanes that share it in RsMisc::maskA / maskB (rs_phase_p5.inc), and the closing barrier hands them to
 *   every thread as it hands over the grants.
 * flow (rs_group_schedule_tti_flows; scheduler 1, never with res / que): DL_PF_PacketScheduler races FLOWS -- bearers --, not users, so a
 *   call position is one bearer of one user (RRC-container order: a user may hold two adjacent positions).  The cell keeps the queued
 *   form's bearer stores and the counted form's counters; the update is the queued form's step 1, the call's average of a position is
 *   the flow's own (scheduler 1 divides by it as it is: no sum, no 1 +), and behind the body the WHOLE transport block goes to the
 *   flow -- pending bytes, bytes counter, PRB counter --, no min with the data (ref: dl-pf-packet-scheduler.cpp:80-85).  The slot's
 *   bearer words (0 or 1 per call position) travel where the queued form's data words do (grp_qin), the gate is the plain PF call's
 *   (data_to_transmit, packed by the host).
 * run (rs_group_run_at; only with res, never NVS): the workgroup serves T consecutive TTIs of its cell -- the resident form's three
 *   steps, T times, in their order and arithmetic, then the completion chain once.  The header is read once; what changes per TTI --
 *   the clock and the rand() pair -- comes from the slot's table (RsGroupCell::run_table), output block t lies run_out_step bytes
 *   behind block t - 1, and the users are the slot's for the whole run.  TTI 0 does with the CQI reports what the slot's image_mode
 *   says; under a cqi_epoch the later TTIs load the cell's image (and read the cell's per-PRB store) as calls of their own would,
 *   without one they read the slot's blocks again.  Between two TTIs stands one workgroup barrier behind a device-scope fence: the
 *   credit of TTI t goes by call position, the update of TTI t + 1 by user id -- other threads --, and the body's load phase overwrites
 *   the LDS grants the credit reads.  A text of its own below: the other instantiations' resident text is left as it is.
 * run with cnt (rs_group_run_counted_at): the cell also keeps m_cumulateBytes / m_cumulateRBs per USER -- a backlogged cell holds one
 *   bearer per user -- in a [U] store of its own (grp_cbytes / grp_crbs point at it in this form), and step 3's thread adds the
 *   position's grant and its PRBs to them (DoStopSchedule, ref: downlink-transport-scheduler.cpp:177-190; scheduler 1:
 *   dl-pf-packet-scheduler.cpp:84-85).  The PRB count: the counted form's lane masks for the schedulers whose link adaptation runs in
 *   rs_phase_p5.inc; UpperBound (10) adapts in rs_phase_p4.inc and leaves no masks -- there the count is the user's taken entries of
 *   its slice's list in LDS, which is what its user_nprb is made of (an RBG that two slices took counts for both, so the owner map
 *   would fall short).  With the slot header's run_no_out set the body's log pointers are null for the whole run: no output block is
 *   written.  Both counter adds of one user in TTIs t and t + 1 are ordered by the fence and barrier that order the credit.
 * run with cnt and the slot header's run_rec_cap set (rs_group_run_records_at): step 3's thread also writes a grant record -- position,
 *   user id, bytes, PRBs, both counters as just stored -- into the TTI's list of the slot's record block in device memory; places are
 *   handed out per wave (ballot, one add on the TTI's count word, prefix popcount), a place at or behind the capacity is not written.
 *   The counted run's step 3 is a text of its own for that: a trip count every lane of a wave shares. */
  constexpr RsGroupForm kGrpF = rs_group_form(kGrpForm);
  constexpr bool kGrpRes = kGrpF.res, kGrpQue = kGrpF.que, kGrpCnt = kGrpF.cnt, kGrpFlow = kGrpF.flow, kGrpRun = kGrpF.run;
  static_assert(kGrpFixed ? rs_group_form_builds(kGrpForm, kGrpSched) : rs_group_form_serves(kGrpForm, kGrpSched), "no kernel of this form for this scheduler (rs_group_form, rs_device.h)");
  const uint8_t* const in = p.grp_in + (size_t)blockIdx.x * (size_t)p.grp_in_stride;
  uint8_t* const out = p.grp_out + (size_t)blockIdx.x * (size_t)p.grp_out_stride;
  const RsGroupCell* const h = (const RsGroupCell*)in;
  /* (one address for the whole workgroup: the values are wave-uniform, and the compiler is told so) */
  auto word = [](const int32_t* q) { return __builtin_amdgcn_readfirstlane(*q); };
  const uint8_t* const data = in + RS_GROUP_HDR_BYTES;
  RsLaunch q = p;
  const int cell = word(&h->cell);
  q.U = word(&h->U);
  q.Upad = word(&h->Upad);
  q.n_seg = word(&h->n_seg);
  q.n_items = word(&h->n_items);
  q.rand0 = word(&h->rand0);
  q.rand1 = word(&h->rand1);
  const int in_slice = word(&h->in_slice);
  q.epochs = data;
  q.grid_stride = (int64_t)in_slice;
  q.user_slice = data + in_slice;
  q.avg = (double*)(data + word(&h->in_avg));
  q.hol = (const double*)(data + word(&h->in_hol));
  q.prio = data + word(&h->in_prio);
  q.gate = p.gate ? (const int32_t*)(data + word(&h->in_gate)) : nullptr;
  q.prb_cqi = p.prb_cqi ? data + word(&h->in_prb) : nullptr;
  q.log_tbs = (int32_t*)out;
  q.log_uinfo = (int32_t*)(out + word(&h->out_uinfo));
  q.log_map = (int16_t*)(out + word(&h->out_map));
  q.log_quota = (int16_t*)(out + word(&h->out_quota));
  q.log_target = (int16_t*)(out + word(&h->out_target));
  q.log_upper = p.log_upper ? (int32_t*)(out + word(&h->out_upper)) : nullptr;
  q.slice_state = p.slice_state + (size_t)cell * (kGrpFixed ? RS_JIT_S : p.S);
  q.scal = p.scal + cell;
  /* rs_tti_in.cqi_epoch, per slot: the image belongs to the CELL (the slot that serves it changes from call to call) */
  const int mode = word(&h->image_mode);
  q.image_mode = mode;
  q.grid_image = p.grp_image + (size_t)cell * (size_t)p.grp_image_stride;
  if (p.prb_cqi && mode != 0) {
    uint8_t* const store = p.grp_prb + (size_t)cell * (size_t)p.grp_prb_stride;
    if (mode == 2) {
      q.prb_cqi = store; /* same reports as the cell's last stored call: the slot's per-PRB block was not sent */
    } else {
      /* new reports: the cell's copy for the calls that follow, 16 bytes per lane.  Nothing in this launch reads it (the body reads
       * the slot's block), so the stores drain behind the body's first phase; the next launch is what orders them. */
      const uint4* const src = (const uint4*)q.prb_cqi;
      const int n16 = (q.U * (kGrpFixed ? RS_JIT_R : p.R) * (kGrpFixed ? RS_JIT_G : p.G) + 15) >> 4;
      for (int i = threadIdx.x; i < n16; i += (kGrpFixed ? (unsigned)RS_JIT_NT : blockDim.x)) ((uint4*)store)[i] = src[i];
    }
  }
  constexpr RsCarve kGrpCv = rs_carve(RS_JIT_S, RS_JIT_U, RS_JIT_R, RS_JIT_SCHED, RS_JIT_NT, RS_JIT_CARVEQ, RS_JIT_WIN); /* (the body's own carve: a run-time build's LDS offsets) */
#ifdef RS_STAMPS
  /* diagnostic build: every call slot stamps a row of its own (the body stamps row `cell` of its block, and cell is 0 there) */
  if (p.stamps) q.stamps = p.stamps + (size_t)blockIdx.x * 20;
  unsigned long long grp_res_cycles = 0;
#endif
  if constexpr (kGrpRun) {
    /* (shape and carve: the launch block's in the built-in kernels, the constants RS_JIT_* in a group's run-time build) */
    const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
    const int n_all = kGrpFixed ? RS_JIT_U : p.U; /* the config's users: the stores' stride and the update's range */
    double* const r_avg = p.grp_avg + (size_t)cell * (size_t)n_all;
    int32_t* const r_pend = p.grp_pending + (size_t)cell * (size_t)n_all;
    auto dword = [&](const double* d) { return __hiloint2double(word((const int32_t*)d + 1), word((const int32_t*)d)); };
    const int n_run = word(&h->run_ttis);
    const uint8_t* const table = in + word(&h->run_table);
    const int out_step = word(&h->run_out_step);
    const int in_uid = word(&h->in_uid);
    const int32_t* const uid = (const int32_t*)(data + in_uid);
    double* const row = p.grp_gather + (size_t)cell * (size_t)n_all;
    int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all;
    const int32_t* const granted = (const int32_t*)(lds + (kGrpFixed ? kGrpCv.off_tx : p.off_tx));
    if constexpr (kGrpLean) { /* (the lean build: as behind the other forms' preambles -- here the body is called inside the loop) */
      q.hol = nullptr;
      q.prio = nullptr;
    }
    /* (the cell's last-update time rides in a register: every thread reads the word here, thread 0 writes it behind the loop, whose
     * barriers lie between the two) */
    double last = dword(p.grp_last + cell);
    uint8_t* o = out;
    if constexpr (kGrpCnt) {
      /* grant records (rs_group_run_records_at): the slot's capacity word, read once per launch.  The counted run has no sent rows, so
       * the launch block's grp_sent / grp_sent_stride carry the record block; the workgroup's copy of the two words -- which the body
       * does not read -- keeps the slot's own block and the capacity (0: no records, nothing is read or written through the pointer). */
      const int rec_cap = word(&h->run_rec_cap);
      q.grp_sent = rec_cap != 0 ? p.grp_sent + (size_t)blockIdx.x * (size_t)p.grp_sent_stride : nullptr;
      q.grp_sent_stride = (int64_t)rec_cap;
    }
    for (int t = 0; t < n_run; ++t) {
      const uint8_t* const tr = table + (size_t)t * RS_GROUP_RUN_ROW_BYTES;
      const double now = dword((const double*)tr);
      q.rand0 = word((const int32_t*)tr + 2);
      q.rand1 = word((const int32_t*)tr + 3);
      q.log_tbs = (int32_t*)o;
      q.log_uinfo = (int32_t*)(o + word(&h->out_uinfo));
      q.log_map = (int16_t*)(o + word(&h->out_map));
      q.log_quota = (int16_t*)(o + word(&h->out_quota));
      q.log_target = (int16_t*)(o + word(&h->out_target));
      q.log_upper = p.log_upper ? (int32_t*)(o + word(&h->out_upper)) : nullptr;
      if constexpr (kGrpCnt) { /* (every word of the counted run stands inside an `if constexpr` of its own: the run kernels keep their text) */
        if (word(&h->run_no_out) != 0) { /* (wave-uniform: a header word.  Every store of the body to an output row stands behind one of these pointers) */
          q.log_tbs = nullptr;
          q.log_uinfo = nullptr;
          q.log_map = nullptr;
          q.log_quota = nullptr;
          q.log_target = nullptr;
          q.log_upper = nullptr;
        }
      }
      /* 1. the update, for every user id of the cell: the resident form's step 1, operation by operation */
      if (!(now == last)) {
        const double dt = now - last;
        for (int u = threadIdx.x; u < n_all; u += nthreads) {
          double a = r_avg[u];
          const int txb = r_pend[u];
          double rate = (double)(int32_t)((uint32_t)txb * 8u) / dt;
          const double beta = 0.02;
          a = ((1 - beta) * a) + (beta * rate);
          if (a < 1) a = 1;
          r_avg[u] = a;
          r_pend[u] = 0;
        }
        last = now;
      }
      if constexpr (kGrpCnt) {
        /* (the TTI's record count starts at 0: one thread's store ahead of the barrier below, which every wave passes before its
         * first add in step 3) */
        if (q.grp_sent_stride != 0 && threadIdx.x == 0)
          __hip_atomic_store((int32_t*)((RsGrantRecord*)q.grp_sent + (size_t)n_run * (size_t)q.grp_sent_stride) + t, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      /* behind it a thread reads averages that other threads wrote */
      __syncthreads();
      /* 2. the call's averages, gathered again behind every update.  Thread i writes row entry i and is the thread that reads it in the
       *    body's load phase; the ids are the slot's in TTI 0 (it may lie in host memory) and the cell's row afterwards. */
      q.avg = r_avg;
      if (in_uid != 0) {
        for (int i = threadIdx.x; i < q.U; i += nthreads) {
          const int id = t == 0 ? uid[i] : ids[i];
          row[i] = r_avg[id];
          if (t == 0) ids[i] = id;
        }
        q.avg = row;
      }
      rs_cell_body<kGrpSched, kGrpEpt, kGrpFixed, true, false, true>(q, lds);
      /* 3. the grants, from LDS, by call position: the resident form's step 3 */
      if constexpr (kGrpCnt) {
        /* The counted run's step 3, a text of its own: the credit above, operation by operation, plus the counters and -- with the
         * slot's run_rec_cap set -- one grant record per credited position.  The trip count is the workgroup's (every lane of a wave
         * stays for the ballot; a lane behind the last position holds no grant). */
        int64_t* const c_bytes = p.grp_cbytes + (size_t)cell * (size_t)n_all; /* the cell's counters, by user id */
        int64_t* const c_rbs = p.grp_crbs + (size_t)cell * (size_t)n_all;
        const int n_rbg = kGrpFixed ? RS_JIT_R : p.R, prb_per_rbg = kGrpFixed ? RS_JIT_G : p.G;
        const int rec_cap = (int)q.grp_sent_stride; /* (wave-uniform: from a header word, see above the loop) */
        RsGrantRecord* const rec_list = (RsGrantRecord*)q.grp_sent + (size_t)t * (size_t)rec_cap;
        int32_t* const rec_count = (int32_t*)((RsGrantRecord*)q.grp_sent + (size_t)n_run * (size_t)rec_cap) + t;
        for (int base = 0; base < q.U; base += nthreads) {
          const int i = base + (int)threadIdx.x;
          const bool inside = i < q.U;
          const int bytes = inside ? granted[i] : 0;
          /* GetListOfAllocatedRBs()->size() of the position's block.  A user is named once per call, a cell once per launch: plain
           * 64-bit adds by the position's thread, as the counted form's. */
          int n_held = 0;
          if (inside) {
            if constexpr (kGrpSched == 10) {
              /* (every thread walks its user's slice segment, grant or not: R entries of UpperBound's ent_user, rs_phase_p4.inc; the
               * ones past the slice's quota say "not taken") */
              const uint16_t* const taken = (const uint16_t*)(lds + (kGrpFixed ? kGrpCv.off_elems : p.off_elems));
              const uint16_t* const seg = taken + (int)q.user_slice[i] * n_rbg;
              for (int k = 0; k < n_rbg; ++k) n_held += seg[k] == (uint16_t)i ? 1 : 0;
            } else {
              const RsMisc* const cm = (const RsMisc*)(lds + (kGrpFixed ? kGrpCv.off_misc : p.off_misc));
              n_held = __popcll(cm->maskA[(i + 1) & 63] & cm->maskB[(i + 1) >> 6]);
            }
          }
          const int id = bytes != 0 ? (in_uid != 0 ? ids[i] : i) : 0;
          const int nprb = n_held * prb_per_rbg;
          int64_t cb = 0, cr = 0;
          if (bytes != 0) {
            r_pend[id] += bytes;
            cb = c_bytes[id] + (int64_t)bytes;
            cr = c_rbs[id] + (int64_t)nprb;
            c_bytes[id] = cb;
            c_rbs[id] = cr;
          }
          if (rec_cap != 0) {
            /* a place in the TTI's list per grant: one add per wave on the list's count word (device memory, zeroed ahead of this
             * TTI's first barrier; the workgroup owns the slot), the wave's first place broadcast, a lane's place behind those of the
             * granted lanes below it.  Across waves the places come as the waves arrive: the host sorts a list by position.  A place
             * at or behind the capacity is not written; the count says so to the host. */
            const unsigned long long got = __ballot(bytes != 0);
            if (got != 0ull) {
              const int lane = (int)(threadIdx.x & 63u);
              int first = 0;
              if (lane == 0) first = __hip_atomic_fetch_add(rec_count, (int)__popcll(got), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              first = __builtin_amdgcn_readfirstlane(first);
              const int place = first + (int)__popcll(got & ((1ull << lane) - 1ull));
              if (bytes != 0 && place < rec_cap) {
                int4* const dst = (int4*)(rec_list + place);
                dst[0] = make_int4(i, id, bytes, nprb);
                dst[1] = make_int4((int)(uint32_t)cb, (int)(cb >> 32), (int)(uint32_t)cr, (int)(cr >> 32));
              }
            }
          }
        }
      } else {
        for (int i = threadIdx.x; i < q.U; i += nthreads) {
          const int bytes = granted[i];
#if defined(RS_FAULT_INJECT_RUN)
          /* tests only (tests/test_gpu_group_run_specialize.py): a deliberately wrong run-time build of the RUN form -- in the LAST TTI of
           * a run every served user is credited a byte more; the outputs of all T TTIs stay right, so only the self-check's comparison
           * of the resident stores can catch it.  A value, no address or index, and never T; the twin of RS_FAULT_INJECT_RESIDENT. */
          if (bytes != 0) r_pend[in_uid != 0 ? ids[i] : i] += bytes + ((kGrpFixed && t + 1 == n_run) ? 1 : 0);
#else
          if (bytes != 0) r_pend[in_uid != 0 ? ids[i] : i] += bytes;
#endif
        }
      }
      if (t + 1 < n_run) {
        /* (wave-uniform: n_run is a header word.)  The next TTI: its output block; under a cqi_epoch the image that TTI 0 stored or
         * found, and the cell's per-PRB store; and the credit, the image, the per-PRB copy and the slice state out before any thread
         * of the workgroup reads them again. */
        o += out_step;
        if (mode != 0) {
          q.image_mode = 2;
          if (p.prb_cqi) q.prb_cqi = p.grp_prb + (size_t)cell * (size_t)p.grp_prb_stride;
        }
        __threadfence();
        __syncthreads();
      }
    }
    if (threadIdx.x == 0) p.grp_last[cell] = last; /* (now[T-1], or the word as it was when no TTI of the run moved the clock) */
  }
  if constexpr (kGrpRes && !kGrpRun) {
    /* (shape and carve: the launch block's in the built-in kernels, the constants RS_JIT_* in a group's run-time build) */
#ifdef RS_STAMPS
    const unsigned long long grp_res_entry = __builtin_readcyclecounter();
#endif
    const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
    const int n_all = kGrpFixed ? RS_JIT_U : p.U; /* the config's users: the stores' stride and the update's range */
    double* const r_avg = p.grp_avg + (size_t)cell * (size_t)n_all;
    int32_t* const r_pend = p.grp_pending + (size_t)cell * (size_t)n_all;
    /* (two words, one address for the workgroup, as the header's other words) */
    auto dword = [&](const double* d) { return __hiloint2double(word((const int32_t*)d + 1), word((const int32_t*)d)); };
    const double now = dword(&h->now);
    const double last = dword(p.grp_last + cell);
    /* 1. the update, for every user id of the cell whether or not this call names it (the reference updates every bearer, with or
     *    without data); Now == m_lastUpdate is the reference's early return.  The host has checked now >= last and bounded now - last. */
    if (!(now == last)) {
      const double dt = now - last;
      for (int u = threadIdx.x; u < n_all; u += nthreads) {
        double a = r_avg[u];
        const int txb = r_pend[u];
        /* (the reference's int product m_transmittedData * 8; written so that it wraps, as that one does on its machine, where calls
         * that repeat one clock value have piled up 2^28 bytes or more) */
        double rate = (double)(int32_t)((uint32_t)txb * 8u) / dt;
        const double beta = 0.02;
        a = ((1 - beta) * a) + (beta * rate);
        if (a < 1) a = 1;
        r_avg[u] = a;
        r_pend[u] = 0;
      }
    }
    /* every thread has read the cell's last-update word and written its share of the averages: the one barrier of this form (part of
     * the load phase; behind it a thread reads averages that other threads wrote) */
    __syncthreads();
    if (threadIdx.x == 0 && !(now == last)) p.grp_last[cell] = now;
    /* 2. the call's averages: the store itself when the call's users are 0..U-1, else gathered in call order.  Thread i writes row
     *    entry i and is the thread that reads it in the body's load phase (same stride), whose own first barrier serves the rest. */
    const int in_uid = word(&h->in_uid);
    q.avg = r_avg;
    if (in_uid != 0) {
      const int32_t* const uid = (const int32_t*)(data + in_uid);
      double* const row = p.grp_gather + (size_t)cell * (size_t)n_all;
      int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all; /* (kept for step 3: the slot may lie in host memory) */
      for (int i = threadIdx.x; i < q.U; i += nthreads) {
        const int id = uid[i];
        row[i] = r_avg[id];
        ids[i] = id;
      }
      q.avg = row;
    }
#ifdef RS_STAMPS
    grp_res_cycles = __builtin_readcyclecounter() - grp_res_entry;
#endif
  }
  if constexpr (kGrpQue) {
    /* (shape and carve: the launch block's in the built-in kernels, the constants RS_JIT_* in a group's run-time build) */
    const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
    const int n_all = kGrpFixed ? RS_JIT_U : p.U; /* the config's users: 2 n_all bearers, the stores' stride and the update's range */
    double* const b_avg = p.grp_qavg + (size_t)cell * 2 * (size_t)n_all;
    int32_t* const b_pend = p.grp_qpend + (size_t)cell * 2 * (size_t)n_all;
    const uint8_t* const b_has = p.grp_qhas + (size_t)cell * 2 * (size_t)n_all;
    auto dword = [&](const double* d) { return __hiloint2double(word((const int32_t*)d + 1), word((const int32_t*)d)); };
    const double now = dword(&h->now);
    const double last = dword(p.grp_last + cell);
    /* 1. the update, for every EXISTING bearer of every user id of the cell (a bearer that does not exist is neither read nor
     *    written); operations, wrap-around product and order of the resident form's step 1 */
    if (!(now == last)) {
      const double dt = now - last;
      for (int j = threadIdx.x; j < 2 * n_all; j += nthreads) {
        if (b_has[j] == 0) continue;
        double a = b_avg[j];
        const int txb = b_pend[j];
        double rate = (double)(int32_t)((uint32_t)txb * 8u) / dt;
        const double beta = 0.02;
        a = ((1 - beta) * a) + (beta * rate);
        if (a < 1) a = 1;
        b_avg[j] = a;
        b_pend[j] = 0;
      }
    }
    /* the one barrier of this form, as the resident form's: every thread has read the last-update word, and behind it a thread reads
     * averages that other threads wrote */
    __syncthreads();
    if (threadIdx.x == 0 && !(now == last)) p.grp_last[cell] = now;
    /* 2. the call's averages: per call position the sum over the bearers WITH DATA (the reference sums the bearers it inserted,
     *    ComputeSchedulingMetric :681-687) in the form whose 1 + x the body takes: a[b] alone, or ((1 + a0) + a1) - 1 -- exact while
     *    the sum stays below 2^53 (rs_group_set_bearers bounds the averages).  The slot's data words go to the cell's device row for
     *    step 4.  Thread i writes entry i of the three rows and is the thread that reads it (the body's load phase: same stride).
     *    q.U == 0, an update-only slot: nothing to gather, and the body is skipped below. */
    if (q.U != 0) {
      const int in_uid = word(&h->in_uid);
      const int32_t* const uid = (const int32_t*)(data + in_uid);
      const int32_t* const din = p.grp_qin + (size_t)blockIdx.x * (size_t)p.grp_qin_stride;
      double* const row = p.grp_gather + (size_t)cell * (size_t)n_all;
      int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all;
      int32_t* const keep = p.grp_qdata + (size_t)cell * 2 * (size_t)n_all;
      for (int i = threadIdx.x; i < q.U; i += nthreads) {
        const int id = in_uid != 0 ? uid[i] : i;
        const int d0 = din[2 * i], d1 = din[2 * i + 1];
        double v;
        if (d0 > 0 && d1 > 0) v = ((1 + b_avg[2 * id]) + b_avg[2 * id + 1]) - 1;
        else v = b_avg[2 * id + (d0 > 0 ? 0 : 1)]; /* (the host has checked: one of the two has data, and that bearer exists) */
        row[i] = v;
        ids[i] = id;
        keep[2 * i] = d0;
        keep[2 * i + 1] = d1;
      }
      q.avg = row;
    }
  }
  if constexpr (kGrpFlow) {
    /* (shape and carve: the launch block's in the built-in kernel, the constants RS_JIT_* in a group's run-time build) */
    const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
    const int n_all = kGrpFixed ? RS_JIT_U : p.U; /* the config's users: 2 n_all bearers, the stores' stride and the update's range */
    double* const b_avg = p.grp_qavg + (size_t)cell * 2 * (size_t)n_all;
    int32_t* const b_pend = p.grp_qpend + (size_t)cell * 2 * (size_t)n_all;
    const uint8_t* const b_has = p.grp_qhas + (size_t)cell * 2 * (size_t)n_all;
    auto dword = [&](const double* d) { return __hiloint2double(word((const int32_t*)d + 1), word((const int32_t*)d)); };
    const double now = dword(&h->now);
    const double last = dword(p.grp_last + cell);
    /* 1. the update, for every EXISTING bearer of every user id of the cell: the queued form's step 1, operation by operation */
    if (!(now == last)) {
      const double dt = now - last;
      for (int j = threadIdx.x; j < 2 * n_all; j += nthreads) {
        if (b_has[j] == 0) continue;
        double a = b_avg[j];
        const int txb = b_pend[j];
        double rate = (double)(int32_t)((uint32_t)txb * 8u) / dt;
        const double beta = 0.02;
        a = ((1 - beta) * a) + (beta * rate);
        if (a < 1) a = 1;
        b_avg[j] = a;
        b_pend[j] = 0;
      }
    }
    /* the one barrier of this form, as the queued form's */
    __syncthreads();
    if (threadIdx.x == 0 && !(now == last)) p.grp_last[cell] = now;
    /* 2. the call's averages: position i is bearer fb[i] of user uid[i] (the host has checked: 0 or 1, the bearer exists, the id is
     *    one of the config's), and its average is the flow's own.  Thread i writes entry i of both rows and is the thread that reads
     *    them (the body's load phase and step 4: same stride).  q.U == 0, an update-only slot: the body is skipped below. */
    if (q.U != 0) {
      const int in_uid = word(&h->in_uid);
      const int32_t* const uid = (const int32_t*)(data + in_uid);
      const int32_t* const fb = p.grp_qin + (size_t)blockIdx.x * (size_t)p.grp_qin_stride;
      double* const row = p.grp_gather + (size_t)cell * (size_t)n_all;
      int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all;
      for (int i = threadIdx.x; i < q.U; i += nthreads) {
        const int f = 2 * (in_uid != 0 ? uid[i] : i) + fb[i];
        row[i] = b_avg[f];
        ids[i] = f;
      }
      q.avg = row;
    }
  }
  if constexpr (kGrpLean) { /* the plain call (rs_group_kernel_jit): no customised slices -- the slots' HoL delays and priority flags are not read */
    q.hol = nullptr;
    q.prio = nullptr;
  }
  if constexpr (kGrpQue || kGrpFlow) {
    /* (q.U is one word of the slot header: the skip is uniform for the whole workgroup, no barrier of the body is left half met) */
    if (q.U != 0) rs_cell_body<kGrpSched, kGrpEpt, kGrpFixed, true, false, true>(q, lds);
  } else if constexpr (!kGrpRun) { /* (the run form has called the body in its loop) */
    rs_cell_body<kGrpSched, kGrpEpt, kGrpFixed, true, false, true>(q, lds);
  }
  if constexpr (kGrpQue) {
    /* 4. DoStopSchedule's loop (ref: downlink-transport-scheduler.cpp:170-221): the grant of a call position -- from LDS, as the
     *    resident form's -- goes to the user's bearers from the highest priority down, min(available, dataToTransmit) each */
    if (q.U != 0) {
      const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
      const int n_all = kGrpFixed ? RS_JIT_U : p.U;
      const int32_t* const granted = (const int32_t*)(lds + (kGrpFixed ? kGrpCv.off_tx : p.off_tx));
      int32_t* const b_pend = p.grp_qpend + (size_t)cell * 2 * (size_t)n_all;
      const int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all;    /* entry i: written by this thread before the body */
      const int32_t* const keep = p.grp_qdata + (size_t)cell * 2 * (size_t)n_all; /* entries 2i, 2i + 1: likewise */
      /* (the counted form: the cell's counters, the slot's sent rows -- zero-copy: in host memory, written once per position --, and
       * where the body's link adaptation left the RBG lanes of every call position) */
      int64_t* const c_bytes = kGrpCnt ? p.grp_cbytes + (size_t)cell * 2 * (size_t)n_all : nullptr;
      int64_t* const c_rbs = kGrpCnt ? p.grp_crbs + (size_t)cell * 2 * (size_t)n_all : nullptr;
      int32_t* const srow = kGrpCnt ? p.grp_sent + (size_t)blockIdx.x * (size_t)p.grp_sent_stride : nullptr;
      const RsMisc* const cm = (const RsMisc*)(lds + (kGrpFixed ? kGrpCv.off_misc : p.off_misc));
      for (int i = threadIdx.x; i < q.U; i += nthreads) {
        int available = granted[i];
        if (available <= 0) {
          if constexpr (kGrpCnt) *(int2*)(srow + 2 * i) = make_int2(0, 0); /* no grant: no counter moves, the row says so */
          continue;
        }
        const int id = ids[i];
        [[maybe_unused]] int row_sent[2] = {0, 0};
        [[maybe_unused]] int64_t nprb = 0;
        if constexpr (kGrpCnt) {
          /* GetListOfAllocatedRBs()->size(): owner + 1 = i + 1 in two base-64 digits, the lanes that share both hold the position's RBGs */
          const unsigned long long lanes = cm->maskA[(i + 1) & 63] & cm->maskB[(i + 1) >> 6];
          nprb = (int64_t)(__popcll(lanes) * (kGrpFixed ? RS_JIT_G : p.G));
        }
        for (int b = 1; b >= 0; --b) {
          if (available <= 0) break;
          const int d = keep[2 * i + b];
          if (d > 0) {
            const int sent = available < d ? available : d;
            available -= sent;
#if defined(RS_FAULT_INJECT_QUEUED)
            /* tests only (tests/test_gpu_group_queued_specialize.py): a deliberately wrong run-time build of the QUEUED form -- the last
             * bearer credited for a position gets a byte more; the outputs stay right, so only the self-check's comparison of the
             * bearer stores can catch it.  A value, no address or index; the twin of RS_FAULT_INJECT_RESIDENT. */
            b_pend[2 * id + b] += sent + ((kGrpFixed && (available <= 0 || b == 0 || keep[2 * i] <= 0)) ? 1 : 0);
#else
            b_pend[2 * id + b] += sent;
#endif
            if constexpr (kGrpCnt) { /* a user is named once per call, a cell once per launch: plain 64-bit adds by the position's thread */
              c_bytes[2 * id + b] += (int64_t)sent;
#if defined(RS_FAULT_INJECT_COUNTED) && RS_FAULT_INJECT_COUNTED == 1
              /* tests only (tests/test_gpu_group_counted_specialize.py): a deliberately wrong run-time build of the COUNTED form -- the
               * last bearer credited for a position gets a PRB more; outputs, sent rows and bearer stores stay right, so only the
               * self-check's comparison of the counters can catch it.  A value, no address or index; the twin of RS_FAULT_INJECT_QUEUED. */
              c_rbs[2 * id + b] += nprb + ((kGrpFixed && (available <= 0 || b == 0 || keep[2 * i] <= 0)) ? 1 : 0);
#else
              c_rbs[2 * id + b] += nprb;
#endif
#if defined(RS_FAULT_INJECT_COUNTED) && RS_FAULT_INJECT_COUNTED == 2
              /* tests only: ... the position's sent row gets a byte more for that bearer; pending bytes and counters stay right, so only
               * the self-check's comparison of the sent rows can catch it */
              row_sent[b] = sent + ((kGrpFixed && (available <= 0 || b == 0 || keep[2 * i] <= 0)) ? 1 : 0);
#else
              row_sent[b] = sent;
#endif
            }
          }
        }
        if constexpr (kGrpCnt) *(int2*)(srow + 2 * i) = make_int2(row_sent[0], row_sent[1]);
      }
    }
  }
  if constexpr (kGrpFlow) {
    /* 4. DL_PF_PacketScheduler::DoStopSchedule (ref: dl-pf-packet-scheduler.cpp:80-85): the grant of a call position -- tbs_bits / 8,
     *    from LDS, as the resident form's -- goes whole to the position's flow: UpdateTransmittedBytes(availableBytes) feeds the next
     *    update and m_cumulateBytes, UpdateCumulateRBs the PRBs of the flow's block.  The PRB count: the counted form's lane masks.
     *    A flow is named once per call, a cell once per launch: plain adds by the position's thread. */
    if (q.U != 0) {
      const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
      const int n_all = kGrpFixed ? RS_JIT_U : p.U;
      const int32_t* const granted = (const int32_t*)(lds + (kGrpFixed ? kGrpCv.off_tx : p.off_tx));
      int32_t* const b_pend = p.grp_qpend + (size_t)cell * 2 * (size_t)n_all;
      int64_t* const c_bytes = p.grp_cbytes + (size_t)cell * 2 * (size_t)n_all;
      int64_t* const c_rbs = p.grp_crbs + (size_t)cell * 2 * (size_t)n_all;
      const int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all; /* entry i: written by this thread before the body */
      const RsMisc* const cm = (const RsMisc*)(lds + (kGrpFixed ? kGrpCv.off_misc : p.off_misc));
      for (int i = threadIdx.x; i < q.U; i += nthreads) {
        const int bytes = granted[i];
        if (bytes <= 0) continue;
        const int f = ids[i];
        const unsigned long long lanes = cm->maskA[(i + 1) & 63] & cm->maskB[(i + 1) >> 6];
        b_pend[f] += bytes;
#if defined(RS_FAULT_INJECT_FLOWS)
        /* tests only (tests/test_gpu_group_flows_specialize.py): a deliberately wrong run-time build of the FLOWS form -- every credited
         * flow's byte counter gets one more; outputs, averages and pending bytes stay right, so only the self-check's comparison of the
         * counters can catch it.  A value, no address or index; the twin of RS_FAULT_INJECT_QUEUED. */
        c_bytes[f] += (int64_t)bytes + (kGrpFixed ? 1 : 0);
#else
        c_bytes[f] += (int64_t)bytes;
#endif
        c_rbs[f] += (int64_t)(__popcll(lanes) * (kGrpFixed ? RS_JIT_G : p.G));
      }
    }
  }
  if constexpr (kGrpRes && !kGrpRun) {
    /* 3. the grants (DoStopSchedule: min(tbs_bits / 8, 100000000) bytes, rs_phase_p5.inc) from LDS, where the body's closing barrier
     *    left them for every thread -- not from the slot's output rows, which lie in host memory in the zero-copy mode.  A user is
     *    named once per call, a cell once per launch: plain adds. */
    const int nthreads = kGrpFixed ? RS_JIT_NT : (int)blockDim.x;
    const int n_all = kGrpFixed ? RS_JIT_U : p.U;
    const int32_t* const granted = (const int32_t*)(lds + (kGrpFixed ? kGrpCv.off_tx : p.off_tx));
    int32_t* const r_pend = p.grp_pending + (size_t)cell * (size_t)n_all;
    const int in_uid = word(&h->in_uid);
    const int32_t* const ids = p.grp_uid + (size_t)cell * (size_t)n_all; /* entry i: written by this thread before the body */
    for (int i = threadIdx.x; i < q.U; i += nthreads) {
      const int bytes = granted[i];
#if defined(RS_FAULT_INJECT_RESIDENT)
      /* tests only (tests/test_gpu_group_resident_specialize.py): a deliberately wrong run-time build of the RESIDENT form -- every served
       * user is credited a byte more; the outputs stay right, so only the self-check's comparison of the resident stores can catch it.
       * A value, no address or index; the twin of RS_FAULT_INJECT_DIRECT. */
      if (bytes != 0) r_pend[in_uid != 0 ? ids[i] : i] += bytes + (kGrpFixed ? 1 : 0);
#else
      if (bytes != 0) r_pend[in_uid != 0 ? ids[i] : i] += bytes;
#endif
    }
#ifdef RS_STAMPS
    if (threadIdx.x == 0 && q.stamps) q.stamps[9] += grp_res_cycles; /* (the update and the gather belong to the load phase; this slot's own row) */
#endif
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t before = __hip_atomic_fetch_add(p.grp_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1u == (uint32_t)p.n_cells) {
      __hip_atomic_store(p.grp_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p.done_flag) __hip_atomic_store(p.done_flag, p.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
