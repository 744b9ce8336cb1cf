/* rs_phase_group.inc -- one TTI for a group of drop-in cells in one launch (rs_group_schedule_tti): workgroup k serves call slot k.  It reads the slot's
 * header (which cell, how many users, the rand() pair, where the slot's arrays lie, what to do with the cell's CQI image), moves every
 * per-cell pointer of the launch block to its slot / its cell and runs the one-TTI body on that block -- the phases never learn that other cells exist.
 * Completion: every thread's outputs are out at system scope (fence), then the workgroup counts itself in on a device word; the
 * workgroup that brings the count to the number of slots -- the last to finish, whichever it is and whenever the others ran: nothing
 * here assumes that the workgroups are resident together -- puts the word back to 0 for the next launch and publishes the call's
 * sequence number to the host.  Its acquire of the counter orders it behind every other workgroup's fence and release.
 *
 * Two entry points of rs_kernels.hip include this text as their body, as rs_cell_body includes its phases: the kernels built into the
 * library (rs_group_kernel: shape in the launch block) and a group's own run-time build (rs_group_kernel_jit, rs_group_specialize).
 * The includer provides `p` (the launch block), `lds` and four constants: kGrpSched, kGrpEpt, kGrpFixed -- shape, workgroup size and LDS
 * carve are the constants RS_JIT_*, RS_JIT_U being the user CAPACITY while the users of a slot stay the slot header's word -- and
 * kGrpLean -- the plain call's per-launch options are constants too.  (Text, not a function of its own: the built-in instantiations
 * must stay the machine code they were, and a wrapper function around the inlined cell body changed their instruction counts.) */
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
  if constexpr (kGrpLean) { /* the plain call (rs_group_kernel_jit): no customised slices -- the slots' HoL delays and priority flags are not read */
    q.hol = nullptr;
    q.prio = nullptr;
  }
  rs_cell_body<kGrpSched, kGrpEpt, kGrpFixed, true, false, true>(q, lds);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t before = __hip_atomic_fetch_add(p.grp_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1u == (uint32_t)p.n_cells) {
      __hip_atomic_store(p.grp_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p.done_flag) __hip_atomic_store(p.done_flag, p.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
