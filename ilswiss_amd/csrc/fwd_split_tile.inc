// fwd_split_tile.inc — the column-split forward of ONE 16-row tile slice, as TEXT: #included inside k_mlp2_fwd_split (its launch wrapper)
// and, once per stage, inside the merged phase kernels (k_sac_phase_a / _c).  A device function with the descriptors passed by reference
// compiled differently (the kernel-argument records stopped being read in place: +100 scalar-spill lane operations and a private
// segment in the backward kernel), so the body is shared as text and every user compiles it against its own kernel arguments.
// A workgroup processes ONE 16-row tile at a time.  (The macro-tile shape — MT = 2 | 4 row tiles together — was measured slower and removed,
// DESIGN §27.  Three blocks below still carry a loop `for (m < MT)` with MT = 1, defined here: written without the one-trip loop they compile
// to other instructions in the phase kernels, and this text does not change what the hot path executes.  They go in a change that measures it.)
// Names the including scope provides: template parameters H, ACT, CS, GRP, PH; `constexpr bool XCH` (see ldx / stx); `A` (FwdArgs),
// `T` (FwdTask), `GP` (const FwdGroup*, GRP only), `bx` (tile index in grid units), `cs` (column slice), `first_task` (this task's lead
// slice publishes the finished policy head), `smem` (dynamic LDS); the macros XCH_HOOK_STAGE (before the input rows are staged) and
// XCH_HOOK_FIN (before the producing policy's head is finished): empty in an ordinary launch, the wait for the previous stage in a phase kernel.
// `constexpr int FIN_CT`: 0 = everything about the input rows and the policy epilogue is decided at run time (the wrappers).  -1 = a stage of
// a phase kernel whose inputs carry no policy epilogue (the first stages: A.fin_on is 0 there, launch_phase_a / _c refuse anything else).
// 1 = phase A's target critics: rows read from T.x0 (no replay draw), every task's action columns the tanh-Gaussian policy's output in CS
// slabs, 16 a <= NTH, noise drawn in the kernel (launch_phase_a refuses anything else).  Then everything that does not depend on the
// awaited policy slices comes BEFORE XCH_HOOK_STAGE: the descriptor fields (held in scalar registers), the noise of pi(s') — the same
// philox_normal4 call and arguments — and the staging loop's index arithmetic; behind the wait: the rows' loads, the head partials
// (requested back to back), the squash.  Same expressions, same order.
  constexpr bool FINS = FIN_CT > 0;
  constexpr int NTH = 4 * H / CS, NWV = NTH / 64, NC = H / 16, SLW = H / CS, NCS = SLW / 16;
  constexpr int NT0 = PH == 1 ? 1 : CS;   // layer-0 column tiles per wave
  constexpr int LDH = H + ILSX_LDS_PAD, LDSL = SLW + ILSX_LDS_PAD;
  constexpr int MT = 1;             // row tiles per workgroup: one (see above)
  constexpr int MR = 16;            // rows of the tile
  static_assert(NCS == NWV, "one k16 chunk of the slice per wave in the head phase");
  const DevScalars* scal = GRP ? GP->scal : A.scal;
  const NetView& N = T.net;
  int KP = N.KP;
  if constexpr (FINS) XCH_PIN(KP);
  const int LDX = KP + ILSX_LDS_PAD, NO = N.NO, NCH0 = KP >> 4, NOT = (NO + 15) >> 4;
  float* xs = smem;                 // [MR][LDX]
  float* h0 = xs + MR * LDX;        // [MR][LDH]   layer-0 activations, all H columns
  float* hs = h0 + MR * LDH;        // [MR][LDSL]  this slice of the layer-1 activations
  float* red = hs + MR * LDSL;      // [4 tiles][NWV][4][64] head partial tiles
  constexpr int RNT = 4;            // head-output tiles in `red`
  if (bx & ((1u << A.xs) - 1u)) return;   // XCD confinement: the dispatcher deals workgroups round-robin to the 8 XCDs
  if ((int)(bx >> A.xs) * (A.rt > 0 ? A.rt : 1) * MR >= A.rows) return;   // grid.x is padded to a multiple of 8
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int rows = A.rows;
  const int RT = A.rt > 0 ? A.rt : 1;   // row tiles this workgroup walks with its weights held in registers
  const bool lead = cs == 0;
  ILSX_STAMP(A.dbg, 0);

  // ---- every small global operand is requested up front, in the order it is needed
  const int ct0 = PH == 1 ? cs * NWV + wave : wave * CS;   // this wave's first layer-0 column tile
  const float* w0p = N.base + N.off_W[0] + (size_t)ct0 * NCH0 * 256 + 4 * lane;
  constexpr int L0D = 8;   // PH 1: k16 chunks of layer-0 weights requested ahead of the MFMAs that consume them
  float4 b0[NT0], b0first[NT0];
  float4 l0first[PH == 1 ? L0D : 1];
  float bias0[NT0];
  if constexpr (PH == 1) {
#pragma unroll
    for (int d = 0; d < L0D; ++d) l0first[d] = *reinterpret_cast<const float4*>(w0p + (size_t)(d < NCH0 ? d : 0) * 256);
  }
  if constexpr (PH != 2) {
#pragma unroll
    for (int i = 0; i < NT0; ++i) b0[i] = *reinterpret_cast<const float4*>(w0p + (size_t)i * NCH0 * 256);
#pragma unroll
    for (int i = 0; i < NT0; ++i) b0first[i] = b0[i];
#pragma unroll
    for (int i = 0; i < NT0; ++i) bias0[i] = (N.base + N.off_b[0])[(ct0 + i) * 16 + li];
  }
  const int lc = wave * 16 + li, col1 = cs * SLW + lc;
  float bias1 = 0.0f;
  float4 whf[4];
  float4 wreg[NC];
  constexpr bool LATEW = GRP == 3 && PH == 0;
  if constexpr (PH != 1) {
    bias1 = (N.base + N.off_b[1])[col1];
    // head weights of this slice as MFMA B fragments: wave w owns k16 chunk w of the slice, rows j = 16t + li
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 16 * t + li;
      whf[t] = (t < NOT && j < NO) ? *reinterpret_cast<const float4*>(N.base + N.off_Wh + (size_t)j * H + cs * SLW + 16 * wave + 4 * g)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- this wave's slice of layer 1 (16 columns x H): one coalesced burst, held for every row tile
    if constexpr (!LATEW) {
      const float* wp = N.base + N.off_W[1] + (size_t)(cs * NWV + wave) * NC * 256 + 4 * lane;
#pragma unroll
      for (int c = 0; c < NC; ++c) wreg[c] = *reinterpret_cast<const float4*>(wp + 256 * c);
    }
  }
#ifdef XCH_FINE_DBG
  ILSX_STAMP_SYNC(XCH_FINE_DBG, 6);   // the weights have arrived
#endif
  const bool fin = FIN_CT >= 0 && (GRP ? GP->fin_on : A.fin_on) != 0 && !T.no_fin && T.d1 > 0;
  const GatherSpec& G = GRP ? GP->gather : A.gather;
  for (int rt = 0; rt < RT; ++rt) {
  const int r0 = ((bx >> A.xs) * RT + rt) * MR;
  if (r0 >= rows) break;   // workgroup-uniform
  const bool full_tile = r0 + MR <= rows;   // workgroup-uniform: every row of the tile is a batch row
  bool fin_logp = false;
  int sf_a = 0; float* sf_logp = nullptr;   // FINS: the epilogue's action count and (publishing slice) log-pi destination
  if constexpr (PH != 2) {
#pragma unroll
  for (int i = 0; i < NT0; ++i) b0[i] = b0first[i];
  if constexpr (FINS) {
    static_assert(PH == 0 && GRP == 0 && XCH, "the static epilogue is phase A's target-critic stage");
    const PolicyFinishArgs& FP = A.fin;   // (`P` is the phase kernel's own block, which the hook names)
    const bool pub = lead && first_task;
    int sf_d0 = T.d0, sf_s0 = T.s0, sf_ps = FP.part_stride;
    const float* sf_x0 = T.x0; const float* sf_part = FP.part; float* sf_xsave = lead ? T.xsave : nullptr;
    float* sf_raw = pub ? FP.raw : nullptr; float* sf_action = pub ? FP.action : nullptr; float* sf_epss = pub ? FP.eps_save : nullptr;
    sf_a = FP.a; sf_logp = pub ? FP.logp : nullptr;
    XCH_PIN(sf_d0); XCH_PIN(sf_s0); XCH_PIN(sf_ps); XCH_PIN(sf_x0); XCH_PIN(sf_part); XCH_PIN(sf_xsave);
    XCH_PIN(sf_raw); XCH_PIN(sf_action); XCH_PIN(sf_epss); XCH_PIN(sf_a); XCH_PIN(sf_logp);
    const int a = sf_a, NOp = 2 * a;
    // the epilogue element (row, action) this thread owns, and its noise
    const int fr = tid / a, fj = tid - fr * a, fgr = r0 + fr;
    const bool fon = tid < MR * a && fgr < rows;
    float fep = 0.0f;
    if (fon) {   // (drawn in the kernel: launch_phase_a refuses explicit noise, which only one-launch-per-stage steps take)
      const unsigned long long fstep = FP.scal ? (FP.use_gather_step ? FP.scal->gather_step : FP.scal->step) : FP.step_host;
      float z4[4];
      philox_normal4(FP.seed, fstep, FP.rng_stream, fgr, fj >> 2, z4);
      const int q = fj & 3;
      fep = q == 0 ? z4[0] : q == 1 ? z4[1] : q == 2 ? z4[2] : z4[3];
    }
    // the staged elements of the first STG trips (KP <= 32: all of them): row, column, what to do with it
    constexpr int STG = 2;
    int sr[STG], sk[STG];
#pragma unroll
    for (int t = 0; t < STG; ++t) { const int e = tid + t * NTH; sr[t] = e / KP; sk[t] = e - sr[t] * KP; }
    XCH_HOOK_STAGE
    {
      float sv[STG];
#pragma unroll
      for (int t = 0; t < STG; ++t) {
        const int gr = r0 + sr[t];
        sv[t] = (tid + t * NTH < MR * KP && gr < rows && sk[t] < sf_d0) ? xg<true>(sf_x0)[(size_t)gr * sf_s0 + sk[t]] : 0.0f;
      }
      // the CS head partials: all requested before any is summed
      float pm[4], pl[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t at = ((size_t)(c < CS ? c : 0) * sf_ps + (fon ? fgr : r0)) * NOp + fj;
        pm[c] = fon ? ldx<XCH>(xg<true>(sf_part + at)) : 0.0f;
        pl[c] = fon ? ldx<XCH>(xg<true>(sf_part + at + a)) : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < STG; ++t) {
        const int gr = r0 + sr[t];
        const bool act_col = sk[t] >= sf_d0 && sk[t] < sf_d0 + a;
        if (tid + t * NTH < MR * KP && !act_col) {   // the action columns: filled by the epilogue below
          if (sf_xsave && gr < rows) xg<true>(sf_xsave)[(size_t)gr * KP + sk[t]] = sv[t];
          xs[sr[t] * LDX + sk[t]] = sv[t];
        }
      }
      for (int e = tid + STG * NTH; e < MR * KP; e += NTH) {   // wider inputs: the further trips
        const int r = e / KP, k = e - r * KP, gr = r0 + r;
        if (k >= sf_d0 && k < sf_d0 + a) continue;
        float v = 0.0f;
        if (gr < rows) {
          if (k < sf_d0) v = xg<true>(sf_x0)[(size_t)gr * sf_s0 + k];
          if (sf_xsave) xg<true>(sf_xsave)[(size_t)gr * KP + k] = v;
        }
        xs[r * LDX + k] = v;
      }
      // combine the head partials, squash (policies.py:262-283, distributions.py:23-28,43-50,74-97); slice 0 of task 0 publishes
      float* lp3 = red;   // [MR][32][3] log-prob contributions (quad, log_std, jacobian)
      float act = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
      if (fon) {
        float mu = 0.f, lsr = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { mu += c < CS ? pm[c] : 0.0f; lsr += c < CS ? pl[c] : 0.0f; }   // slab order
        const float ls = fminf(fmaxf(lsr, LOG_SIG_MIN), LOG_SIG_MAX);
        const float sd = expf(ls);
        const float z = fep * sd + mu;
        act = tanhf(z);
        const float dm = mu - z;
        c0 = dm * dm / expf(2.0f * ls); c1 = ls; c2 = logf(1.0f - act * act + TANH_EPS);
        if (sf_raw) { stx<XCH>(xg<true>(sf_raw + (size_t)fgr * NOp + fj), mu); stx<XCH>(xg<true>(sf_raw + (size_t)fgr * NOp + a + fj), lsr); }
        if (sf_xsave) xg<true>(sf_xsave)[(size_t)fgr * KP + sf_d0 + fj] = act;
        if (sf_action) stx<XCH>(xg<true>(sf_action + (size_t)fgr * a + fj), act);
        if (sf_epss) stx<XCH>(xg<true>(sf_epss + (size_t)fgr * a + fj), fep);
      }
      if (tid < MR * a) {
        xs[fr * LDX + sf_d0 + fj] = act;
        lp3[(fr * 32 + fj) * 3 + 0] = c0; lp3[(fr * 32 + fj) * 3 + 1] = c1; lp3[(fr * 32 + fj) * 3 + 2] = c2;
      }
      fin_logp = sf_logp != nullptr;
    }
  } else {
  XCH_HOOK_STAGE
  if constexpr (PH == 0) {   // narrow inputs (the one-launch form): one element per thread, the row's index drawn where it is used
    long long* ridx0 = reinterpret_cast<long long*>(hs);   // hs is not live before layer 1
    if constexpr (GRP != 0) {   // grouped launches (throughput: every issued instruction counts): the row's index is drawn ONCE, by 16 lanes, not per element by every thread
      if (G.on) {
        if (tid < MR) ridx0[tid] = r0 + tid < rows ? replay_draw(G.seed, scal->gather_step, G.stream, (uint32_t)(r0 + tid), G.st->size) : 0;
        lds_barrier();
      }
    }
    for (int e = tid; e < MR * KP; e += NTH) {
      const int r = e / KP, k = e - r * KP, gr = r0 + r;
      const bool act_col = k >= T.d0 && k < T.d0 + T.d1;
      if (fin && act_col) continue;   // filled by the policy epilogue below
      float v = 0.0f;
      if (gr < rows) {
        if (G.on) {   // fused sample+index (simple_replay_buffer.py:239-293): row gr of the batch is record idx
          long long idx;
          if constexpr (GRP != 0) idx = ridx0[r];
          else idx = replay_draw(G.seed, scal->gather_step, G.stream, (uint32_t)gr, G.st->size);
          const float* rec = G.records + (size_t)idx * G.rec;
          if (k < T.d0) v = rec[T.g0_off + k];
          else if (act_col) v = rec[T.g1_off + (k - T.d0)];
          if (lead && T.publish == 1) {
            if (k < T.d0) G.s[(size_t)gr * G.o + k] = v;
            else if (act_col) G.a[(size_t)gr * G.adim + (k - T.d0)] = v;
            if (k == 0) { stx<XCH>(G.r + gr, rec[G.o + G.adim]); stx<XCH>(G.d + gr, rec[G.o + G.adim + 1]); }
          } else if (lead && T.publish == 2 && k < T.d0) {
            G.s2[(size_t)gr * G.o + k] = v;
          }
        } else {
          if (k < T.d0) v = T.x0[(size_t)gr * T.s0 + k];
          else if (act_col) v = T.x1[(size_t)gr * T.s1 + (k - T.d0)];
        }
        if (T.xsave && lead) T.xsave[(size_t)gr * KP + k] = v;
      }
      xs[r * LDX + k] = v;
    }
  } else {          // PH 1, wide inputs (Humanoid: 25 elements per thread): the index is drawn ONCE per row — the form above spent a Philox
                    // block and a division per element, 21 us per launch — and a wave walks whole rows in coalesced 64-float runs
    // one element of the staged input tile; rec = the replay record of row gr (fused sample+index, simple_replay_buffer.py:239-293)
    auto stage = [&](int r, int k, int gr, const float* rec) {
      const bool act_col = k >= T.d0 && k < T.d0 + T.d1;
      if (fin && act_col) return;   // filled by the policy epilogue below
      float v = 0.0f;
      if (gr < rows) {
        if (G.on) {
          if (k < T.d0) v = rec[T.g0_off + k];
          else if (act_col) v = rec[T.g1_off + (k - T.d0)];
          if (lead && T.publish == 1) {
            if (k < T.d0) G.s[(size_t)gr * G.o + k] = v;
            else if (act_col) G.a[(size_t)gr * G.adim + (k - T.d0)] = v;
            if (k == 0) { G.r[gr] = rec[G.o + G.adim]; G.d[gr] = rec[G.o + G.adim + 1]; }
          } else if (lead && T.publish == 2 && k < T.d0) {
            G.s2[(size_t)gr * G.o + k] = v;
          }
        } else {
          if (k < T.d0) v = T.x0[(size_t)gr * T.s0 + k];
          else if (act_col) v = T.x1[(size_t)gr * T.s1 + (k - T.d0)];
        }
        if (T.xsave && lead) T.xsave[(size_t)gr * KP + k] = v;
      }
      xs[r * LDX + k] = v;
    };
    long long* ridx = reinterpret_cast<long long*>(hs);   // hs is not live before layer 1
    if (G.on) {
      if (tid < MR) ridx[tid] = r0 + tid < rows ? replay_draw(G.seed, scal->gather_step, G.stream, (uint32_t)(r0 + tid), G.st->size) : 0;
      lds_barrier();
    }
    if (KP <= 512 && T.d1 <= 64) {
      // a row is [obs segment | action segment | zero padding]: the segments are copied with clamped, unconditional loads — every load of
      // the wave's four rows is in flight before the first store (a loop around load + store waits per trip: 28 serial HBM round trips
      // per wave for a 396-wide row; per-element source selection compiled to ~90 branchy instructions per element)
      constexpr int RW = 16 / NWV, U = 8;
      const bool acts = T.d1 > 0 && !fin;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {   // one 16-row tile at a time (RW rows per wave in flight)
      float vo[RW][U], va[RW];
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        const int r = 16 * mt + wave + NWV * rr, grc = r0 + r < rows ? r0 + r : rows - 1;
        const float* rec = G.on ? G.records + (size_t)ridx[r] * G.rec : nullptr;
        const float* s0p = G.on ? rec + T.g0_off : T.x0 + (size_t)grc * T.s0;
#pragma unroll
        for (int u = 0; u < U; ++u) { const int k = lane + 64 * u; vo[rr][u] = s0p[k < T.d0 ? k : T.d0 - 1]; }
        va[rr] = 0.0f;
        if (acts) { const float* s1p = G.on ? rec + T.g1_off : T.x1 + (size_t)grc * T.s1; va[rr] = s1p[lane < T.d1 ? lane : T.d1 - 1]; }
      }
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        const int r = 16 * mt + wave + NWV * rr, gr = r0 + r;
        const bool rowok = gr < rows;
        const bool pub1 = G.on && lead && T.publish == 1 && rowok, pub2 = G.on && lead && T.publish == 2 && rowok, xsv = T.xsave && lead && rowok;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = lane + 64 * u;
          if (k < T.d0) {
            const float x = rowok ? vo[rr][u] : 0.0f;
            if (pub1) G.s[(size_t)gr * G.o + k] = x;
            if (pub2) G.s2[(size_t)gr * G.o + k] = x;
            if (xsv) T.xsave[(size_t)gr * KP + k] = x;
            xs[r * LDX + k] = x;
          }
        }
        if (acts && lane < T.d1) {
          const float x = rowok ? va[rr] : 0.0f;
          if (pub1) G.a[(size_t)gr * G.adim + lane] = x;
          if (xsv) T.xsave[(size_t)gr * KP + T.d0 + lane] = x;
          xs[r * LDX + T.d0 + lane] = x;
        }
        if (pub1 && lane == 0) { const float* rec = G.records + (size_t)ridx[r] * G.rec; G.r[gr] = rec[G.o + G.adim]; G.d[gr] = rec[G.o + G.adim + 1]; }
        for (int k = T.d0 + T.d1 + lane; k < KP; k += 64) {   // zero padding up to the k16 multiple
          if (xsv) T.xsave[(size_t)gr * KP + k] = 0.0f;
          xs[r * LDX + k] = 0.0f;
        }
        if (T.d1 > 0 && !acts) { /* action columns: the policy epilogue below fills them */ }
      }
      }   // mt
    } else {
      for (int r = wave; r < MR; r += NWV) {
        const int gr = r0 + r;
        const float* rec = G.on ? G.records + (size_t)ridx[r] * G.rec : nullptr;
        for (int k = lane; k < KP; k += 64) stage(r, k, gr, rec);
      }
    }
  }
  XCH_HOOK_FIN
  if (fin) {
    // the action columns are pi's output: combine its CS head partials, squash (policies.py:262-283,
    // distributions.py:23-28,43-50,74-97); slice 0 of task 0 publishes action / logp / raw / eps for later kernels
    const PolicyFinishArgs& P = GRP ? GP->fin : A.fin;
    const bool det = P.head == HEAD_DET_TANH_NOISE || P.head == HEAD_DET_LIN_NOISE;   // TD3: max_act*tanh(pre) (or max_act*pre) + clipped noise, one head (policies.py:166-188)
    const int a = P.a, NOp = det ? a : 2 * a;
    const bool pub = lead && (GRP ? T.first != 0 : first_task);
    float* lp3 = red;   // [MR][LPS][3] log-prob contributions (quad, log_std, jacobian)
    const unsigned long long fstep = P.scal ? (P.use_gather_step ? P.scal->gather_step : P.scal->step) : P.step_host;   // requested with the partials, not after them
    constexpr int LPS = 32;   // row stride of lp3
    for (int e = tid; e < MR * a; e += NTH) {
      const int row = e / a, j = e - row * a, gr = r0 + row;
      float act = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
      if (gr < rows) {
        // the CS (<= 4) head partials: all requested before any is summed (a loop with a run-time trip count waits for its
        // loads on every trip: four serial round trips at the head of the launch's longest dependent chain)
        float pm[4], pl[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const size_t at = ((size_t)(c < P.cs ? c : 0) * P.part_stride + gr) * NOp + j;
          pm[c] = ldx<XCH>(P.part + at);
          pl[c] = det ? 0.0f : ldx<XCH>(P.part + at + a);
        }
        float mu = 0.f, lsr = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) { mu += c < P.cs ? pm[c] : 0.0f; lsr += c < P.cs ? pl[c] : 0.0f; }   // slab order
        float ep = 0.0f;
        if (!det || P.noise != 0.0f) {
          if (P.eps) {
            ep = P.eps[(size_t)gr * a + j];
          } else {
            float z4[4];
            philox_normal4(P.seed, fstep, P.rng_stream, gr, j >> 2, z4);
            const int q = j & 3;
            ep = q == 0 ? z4[0] : q == 1 ? z4[1] : q == 2 ? z4[2] : z4[3];
          }
        }
        if (det) {
          act = P.max_act * (P.head == HEAD_DET_LIN_NOISE ? mu : tanhf(mu));
          if (P.noise != 0.0f) act += fminf(fmaxf(P.noise * ep, -P.noise_clip), P.noise_clip);
          if (pub && P.raw) stx<XCH>(P.raw + (size_t)gr * a + j, mu);
        } else {
          const float ls = fminf(fmaxf(lsr, LOG_SIG_MIN), LOG_SIG_MAX);
          const float sd = expf(ls);
          const float z = ep * sd + mu;
          act = tanhf(z);
          const float dm = mu - z;
          c0 = dm * dm / expf(2.0f * ls); c1 = ls; c2 = logf(1.0f - act * act + TANH_EPS);
          if (pub && P.raw) { stx<XCH>(P.raw + (size_t)gr * NOp + j, mu); stx<XCH>(P.raw + (size_t)gr * NOp + a + j, lsr); }
        }
        if (T.xsave && lead) T.xsave[(size_t)gr * KP + T.d0 + j] = act;
        if (pub) {
          if (P.action) stx<XCH>(P.action + (size_t)gr * a + j, act);
          if (P.eps_save) stx<XCH>(P.eps_save + (size_t)gr * a + j, ep);
        }
      }
      xs[row * LDX + T.d0 + j] = act;
      lp3[(row * LPS + j) * 3 + 0] = c0; lp3[(row * LPS + j) * 3 + 1] = c1; lp3[(row * LPS + j) * 3 + 2] = c2;
    }
    fin_logp = pub && P.logp && !det;
  }
  }  // !FINS
  }  // PH != 2
  else {   // PH == 2: layer-0 activations of the tile, as the layer-0 launch left them
    const float* hsrc = T.hsave[0];
    for (int e = tid; e < MR * (H / 4); e += NTH) {
      const int row = e / (H / 4), c4 = e - row * (H / 4), gr = r0 + row;
      const float4 v = gr < rows ? *reinterpret_cast<const float4*>(hsrc + (size_t)gr * H + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(h0 + row * LDH + 4 * c4) = v;
    }
  }
  lds_barrier();
  XCH_STAMP(1);
  if (fin_logp && tid < MR && r0 + tid < rows) {   // log pi of the tile's rows from the staged contributions: after the tile's ONE
    const PolicyFinishArgs& P = GRP ? GP->fin : A.fin;   // barrier instead of behind a barrier of its own (`red` is next written two
    float q = 0.f, l = 0.f, jc = 0.f;                    // barriers from here)
    const int pa = FINS ? sf_a : P.a;
    constexpr int LPS = 32;
    for (int j = 0; j < pa; ++j) { q += red[(tid * LPS + j) * 3]; l += red[(tid * LPS + j) * 3 + 1]; jc += red[(tid * LPS + j) * 3 + 2]; }
    stx<XCH>(xg<FINS>((FINS ? sf_logp : P.logp) + r0 + tid), -0.5f * q - (l + HALF_LOG_2PI) - jc);
  }
  // ---- layer 0: CS column tiles per wave, full width (PH 0) ; this slice's own tile (PH 1)
  if constexpr (PH == 1) {
    // a wide layer 0 is a long K loop (25 k16 chunks for Humanoid): with the next chunk requested one step ahead every trip waited
    // for an L2 round trip (24 us per launch); here L0D chunks are in flight while the previous L0D are consumed
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* ap = xs + li * LDX + 4 * g;
    float4 cur[L0D], nxt[L0D];
#pragma unroll
    for (int d = 0; d < L0D; ++d) cur[d] = l0first[d];
    for (int cb = 0; cb < NCH0; cb += L0D) {
#pragma unroll
      for (int d = 0; d < L0D; ++d) {
        const int c = cb + L0D + d;
        nxt[d] = *reinterpret_cast<const float4*>(w0p + (size_t)(c < NCH0 ? c : 0) * 256);
      }
#pragma unroll
      for (int d = 0; d < L0D; ++d) {
        if (cb + d < NCH0) {   // uniform
          const float4 a = *reinterpret_cast<const float4*>(ap + 16 * (cb + d));
          acc = MFMA16(a.x, cur[d].x, acc); acc = MFMA16(a.y, cur[d].y, acc);
          acc = MFMA16(a.z, cur[d].z, acc); acc = MFMA16(a.w, cur[d].w, acc);
        }
      }
#pragma unroll
      for (int d = 0; d < L0D; ++d) cur[d] = nxt[d];
    }
    float* hsv = T.hsave[0];
    const int col = ct0 * 16 + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 4 * g + v;
      if (r0 + row < rows) hsv[(size_t)(r0 + row) * H + col] = act_fn<ACT>(acc[v] + bias0[0]);
    }
  } else if constexpr (PH != 2) {
    f32x4 acc[NT0];
#pragma unroll
    for (int i = 0; i < NT0; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* ap = xs + li * LDX + 4 * g;
    for (int kc = 0; kc < KP; kc += 16) {
      float4 bn[NT0];
#pragma unroll
      for (int i = 0; i < NT0; ++i) {
        bn[i] = b0[i];
        if (kc + 16 < KP) bn[i] = *reinterpret_cast<const float4*>(w0p + (size_t)i * NCH0 * 256 + (kc + 16) * 16);
      }
      const float4 a = *reinterpret_cast<const float4*>(ap + kc);
#pragma unroll
      for (int i = 0; i < NT0; ++i) acc[i] = MFMA16(a.x, b0[i].x, acc[i]);
#pragma unroll
      for (int i = 0; i < NT0; ++i) acc[i] = MFMA16(a.y, b0[i].y, acc[i]);
#pragma unroll
      for (int i = 0; i < NT0; ++i) acc[i] = MFMA16(a.z, b0[i].z, acc[i]);
#pragma unroll
      for (int i = 0; i < NT0; ++i) acc[i] = MFMA16(a.w, b0[i].w, acc[i]);
#pragma unroll
      for (int i = 0; i < NT0; ++i) b0[i] = bn[i];
    }
    float* hsv = (PH == 1 || lead) ? T.hsave[0] : nullptr;
    // saved activations: one 64-bit address per row tile (rows 4g + v and column tiles i are immediate offsets from it), and no row
    // guards when the whole tile is inside the batch (workgroup-uniform): the guarded form was a compare, an EXEC branch and three address
    // instructions per stored element
    float* const hrow = hsv ? hsv + (size_t)(r0 + 4 * g) * H + ct0 * 16 + li : nullptr;
#pragma unroll
    for (int i = 0; i < NT0; ++i) {
      const int col = (ct0 + i) * 16 + li;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 4 * g + v;
        const float h = act_fn<ACT>(acc[i][v] + bias0[i]);
        if constexpr (PH == 0) h0[row * LDH + col] = h;
        acc[i][v] = h;
      }
    }
    if (hsv) {   // workgroup-uniform
      if (full_tile) {
#pragma unroll
        for (int i = 0; i < NT0; ++i)
#pragma unroll
          for (int v = 0; v < 4; ++v) stx<XCH>(hrow + v * H + i * 16, acc[i][v]);
      } else {
#pragma unroll
        for (int i = 0; i < NT0; ++i)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (r0 + 4 * g + v < rows) stx<XCH>(hrow + v * H + i * 16, acc[i][v]);
      }
    }
  }
  if constexpr (PH == 1) {
    lds_barrier();   // the next row tile restages xs
    continue;
  }
  if constexpr (PH == 0) lds_barrier();
  XCH_STAMP(2);
  // ---- layer 1, this slice: straight out of registers
  if constexpr (LATEW) {
    const float* wp = N.base + N.off_W[1] + (size_t)(cs * NWV + wave) * NC * 256 + 4 * lane;
#pragma unroll
    for (int c = 0; c < NC; ++c) wreg[c] = *reinterpret_cast<const float4*>(wp + 256 * c);
  }
  {
    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) { acc0[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[m] = acc0[m]; }
    const float* ap = h0 + li * LDH + 4 * g;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {   // one fetched B fragment, MT row tiles
        const float4 a = *reinterpret_cast<const float4*>(ap + m * 16 * LDH + 16 * c);
        acc0[m] = MFMA16(a.x, wreg[c].x, acc0[m]); acc1[m] = MFMA16(a.y, wreg[c].y, acc1[m]);
        acc0[m] = MFMA16(a.z, wreg[c].z, acc0[m]); acc1[m] = MFMA16(a.w, wreg[c].w, acc1[m]);
      }
    }
    float* hsv = T.hsave[1];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float* const hrow = hsv ? hsv + (size_t)(r0 + 16 * m + 4 * g) * H + col1 : nullptr;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * m + 4 * g + v;
        const float h = act_fn<ACT>(acc0[m][v] + acc1[m][v] + bias1);
        hs[row * LDSL + lc] = h;
        acc0[m][v] = h;
      }
      if (hsv) {   // workgroup-uniform
        if (full_tile) {
#pragma unroll
          for (int v = 0; v < 4; ++v) stx<XCH>(hrow + v * H, acc0[m][v]);
        } else {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (r0 + 16 * m + 4 * g + v < rows) stx<XCH>(hrow + v * H, acc0[m][v]);
        }
      }
    }
  }
  lds_barrier();
  XCH_STAMP(3);
  // ---- head partial sums over this column slice on the matrix pipe: wave w contracts k16 chunk w of the
  //      slice for every 16-output tile, the NWV partial tiles are summed through LDS
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const float4 a = *reinterpret_cast<const float4*>(hs + (16 * m + li) * LDSL + 16 * wave + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < NOT) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc = MFMA16(a.x, whf[t].x, acc); acc = MFMA16(a.y, whf[t].y, acc);
        acc = MFMA16(a.z, whf[t].z, acc); acc = MFMA16(a.w, whf[t].w, acc);
#pragma unroll
        for (int v = 0; v < 4; ++v) red[(((m * RNT + t) * NWV + wave) * 4 + v) * 64 + lane] = acc[v];
      }
    }
  }
  lds_barrier();
  const float* bh = N.base + N.off_bh;
#pragma unroll
  for (int m = 0; m < MT; ++m)
  for (int e = tid; e < NOT * 256; e += NTH) {
    const int t = e >> 8, v = (e >> 6) & 3, ol = e & 63;
    float sum = 0.0f;
#pragma unroll
    for (int w2 = 0; w2 < NWV; ++w2) sum += red[(((m * RNT + t) * NWV + w2) * 4 + v) * 64 + ol];
    const int row = 16 * m + 4 * (ol >> 4) + v, j = 16 * t + (ol & 15), gr = r0 + row;
    if (j < NO && gr < rows) stx<XCH>(T.part + ((size_t)cs * A.part_stride + gr) * NO + j, sum + (lead ? bh[j] : 0.0f));
  }
  lds_barrier();   // the next row tile reuses xs / h0 / hs / red
  }  // rt
  ILSX_STAMP(A.dbg, 7);
