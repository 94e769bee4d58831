// bwd_split_tile.inc — the column-split backward-to-activations of ONE 16-row tile slice, as TEXT (see fwd_split_tile.inc).
// Names the including scope provides: template parameters H, ACT, CS; `constexpr bool XCH`; `A` (BwdArgs), `T` (BwdTask), `bx`, `cs`, `smem`;
// `constexpr int LOSS_CT` (the stage's loss kind, -1 = T.loss at run time) and `constexpr int NO_CT` (head outputs, 0 = N.NO at run time).
// A phase-kernel stage (XCH) with a compile-time loss runs the STATIC HEAD: no dispatch over the loss kinds, every descriptor field the head
// and the delta_1 phase need read ahead of the waits (XCH_HOOK_*) and held in scalar registers, and every operand and sub-expression that
// does not depend on the awaited stage loaded / evaluated before the wait too.  Behind the wait come only the awaited operands, requested
// back to back, and the rest of the arithmetic: the same expressions in the same association as bwd_head_grad (the library is built
// with -ffp-contract=off, so where an expression is evaluated does not change it).
  constexpr int NTH = 4 * H / CS, NWV = NTH / 64, NC = H / 16, SLW = H / CS, RPW = 16 / NWV, KPL = SLW / 64;
  constexpr int RPT = 16 * H / NTH, RSTEP = NTH / H;   // delta_1: thread <-> one column, RPT rows RSTEP apart
  constexpr int LDH = H + ILSX_LDS_PAD, LDSL = SLW + ILSX_LDS_PAD;
  constexpr int MT = 1;   // row tiles per workgroup: one.  The loops `for (m < MT)` below are kept as text (see fwd_split_tile.inc)
  constexpr int MR = 16;
  static_assert(NTH % H == 0 && RPW >= 1 && KPL >= 1, "unsupported split geometry");
  const NetView& N = T.net;
  constexpr bool SH = XCH && LOSS_CT >= 0;
  int NO = NO_CT > 0 ? NO_CT : N.NO;
  if constexpr (SH && NO_CT == 0) XCH_PIN(NO);
  static_assert(!SH || LOSS_CT == LOSS_SAC_CRITIC || LOSS_CT == LOSS_SAC_ACTORQ || LOSS_CT == LOSS_SAC_POLICY, "static heads: the SAC step's three");
  static_assert(!SH || LOSS_CT == LOSS_SAC_POLICY || NO_CT == 1, "a critic has one head output");
  float* d1 = smem;                      // [MR][LDH]  delta_1, all H columns
  float* d0s = d1 + MR * LDH;            // [MR][LDSL] this slice of delta_0
  float* dout = d0s + MR * LDSL;         // [MR][ILSX_MAX_NO]
  if (bx & ((1u << A.xs) - 1u)) return;
  if ((int)(bx >> A.xs) * MR >= A.rows) return;   // grid.x is padded to a multiple of 8 (launch_bwd)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, g = lane >> 4;
  const int r0 = (bx >> A.xs) * MR, rows = A.rows;
  const bool lead = cs == 0;
  // Whole tile inside the batch — workgroup-uniform: the saved-activation loads and the delta stores below then go without row
  // guards and off one 64-bit address per run (the guarded form compiled to a compare, an EXEC branch and three address instructions per
  // element: ~200 of the backward's instructions per thread for the 16 h_1 loads alone)
  const bool full_tile = r0 + MR <= rows;
  ILSX_STAMP(A.dbg, 0);

  // ---- operands of the later phases, requested first (they land while the loss head is evaluated)
  const int k1 = tid % H, rb1 = tid / H;
  const int lc = wave * 16 + li, col0 = cs * SLW + lc;
  float h1v[MT][RPT];
  float h0v[MT][4];
  float4 wreg[NC];
  // Order of the requests.  Ordinary launch: activations, small weights, the loss head, then the 64 KB burst of W_1 (so that the
  // head's operands do not queue behind it).  Inside a phase kernel (XCH) everything that does not depend on another workgroup of the
  // launch — all weights — is requested BEFORE the wait for those workgroups (XCH_HOOK_ACT / XCH_HOOK_HEAD are that wait), so its
  // latency is spent while waiting; the values and the arithmetic are the same either way.
  // head weights of this thread's column for the delta_1 phase: requested now (inside that phase's loop they were dependent loads)
  constexpr int WHP = (XCH && LOSS_CT >= 0 && NO_CT != 1) ? 16 : 12;   // (the static wide head: see the delta_1 phase)
  float whp[WHP];
#pragma unroll
  for (int j = 0; j < WHP; ++j) whp[j] = (N.base + N.off_Wh)[(size_t)(j < NO ? j : 0) * H + k1];
  // first-layer weights of the dL/dx partial (last phase) as MFMA B fragments, requested here with the other operands: wave w
  // contracts k16 chunk w of this slice, lane (g, li) supplies W0[n = slice + 16w + 4g + s][column dx_col0 + 16t + li], s = 0..3
  constexpr int DXT = 2;   // 16-column tiles of dL/dx (dx_cols <= 32: a = 17 for Humanoid)
  static_assert(SLW / 16 == NWV, "one k16 chunk of the slice per wave in the dL/dx phase");
  float w0b[DXT][4];
  if (T.dx) {
    const float* W0 = N.base + N.off_W[0];
    const int ld0 = N.ld[0];
#pragma unroll
    for (int t = 0; t < DXT; ++t)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int c = 16 * t + li;
        w0b[t][s4] = c < T.dx_cols ? W0[pack_f(cs * SLW + 16 * wave + 4 * g + s4, T.dx_col0 + c, ld0)] : 0.0f;
      }
  }
  if constexpr (XCH) {
  // ---- this wave's slice of W_1 (backward-packed: all H rows x its 16 columns), one coalesced burst
    {
      const float* wp = N.base + N.off_Wb[1] + (size_t)(cs * NWV + wave) * NC * 256 + 4 * lane;
#pragma unroll
      for (int c = 0; c < NC; ++c) wreg[c] = *reinterpret_cast<const float4*>(wp + 256 * c);
    }
  }
  // ---- static head: descriptor fields, read here and pinned in scalar registers (a field of the constant table is otherwise a scalar
  //      load — and a wait for it — at every use, in series behind the hand-off)
  const float* sh_h1 = nullptr; const float* sh_h0 = nullptr; const float* sh_Wh = nullptr; float* sh_dhead = nullptr; float* sh_ds1 = nullptr;
  const float *sh_p0 = nullptr, *sh_p1 = nullptr, *sh_p2 = nullptr;   // CRITIC: tq1, tq2, logp_next ; ACTORQ: q1n, q2n ; POLICY: ga1, ga2
  int sh_i0 = 0, sh_i1 = 0;                                             // CRITIC / ACTORQ: the two slab strides ; POLICY: i0 = ga_stride * a
  int sh_which = 0;
  float sh_invB = 0.0f;
  if constexpr (SH) {
    sh_h1 = T.hsave[1]; sh_h0 = T.hsave[0]; sh_Wh = N.base + N.off_Wh; sh_dhead = lead ? T.dhead : nullptr; sh_ds1 = lead ? T.dsave[1] : nullptr;
    sh_invB = A.inv_B;
    if constexpr (LOSS_CT == LOSS_SAC_CRITIC) { sh_p0 = T.tq1.p; sh_i0 = T.tq1.stride; sh_p1 = T.tq2.p; sh_i1 = T.tq2.stride; sh_p2 = T.logp_next; }
    if constexpr (LOSS_CT == LOSS_SAC_ACTORQ) { sh_p0 = T.q1n.p; sh_i0 = T.q1n.stride; sh_p1 = T.q2n.p; sh_i1 = T.q2n.stride; sh_which = T.which; }
    if constexpr (LOSS_CT == LOSS_SAC_POLICY) { sh_p0 = T.ga1; sh_p1 = T.ga2; sh_i0 = A.ga_stride * (NO >> 1); }
    XCH_PIN(sh_h1); XCH_PIN(sh_h0); XCH_PIN(sh_Wh); XCH_PIN(sh_dhead); XCH_PIN(sh_ds1); XCH_PIN(sh_invB);
    XCH_PIN(sh_p0); XCH_PIN(sh_p1); XCH_PIN(sh_i0);
    if constexpr (LOSS_CT != LOSS_SAC_POLICY) XCH_PIN(sh_i1);
    if constexpr (LOSS_CT == LOSS_SAC_CRITIC) XCH_PIN(sh_p2);
    if constexpr (LOSS_CT == LOSS_SAC_ACTORQ) XCH_PIN(sh_which);
  }
  XCH_HOOK_ACT
  {
    const float* const h1p = (SH ? sh_h1 : T.hsave[1]) + (size_t)(r0 + rb1) * H + k1;
    const float* const h0p = (SH ? sh_h0 : T.hsave[0]) + (size_t)(r0 + 4 * g) * H + col0;
    if (full_tile) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) h1v[0][i] = ldx<XCH>(xg<SH>(h1p + (size_t)(RSTEP * i) * H));
#pragma unroll
      for (int v = 0; v < 4; ++v) h0v[0][v] = ldx<XCH>(xg<SH>(h0p + (size_t)v * H));
    } else {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int gr = r0 + rb1 + RSTEP * i;
        h1v[0][i] = gr < rows ? ldx<XCH>(xg<SH>(h1p + (size_t)(RSTEP * i) * H)) : 0.0f;
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int gr = r0 + 4 * g + v;
        h0v[0][v] = gr < rows ? ldx<XCH>(xg<SH>(h0p + (size_t)v * H)) : 0.0f;
      }
    }
  }
  // ---- static head.  Per trip of the head loop (one trip while 16 NO <= NTH, a <= 8; thread <-> (row, output)): first the operands and
  //      sub-expressions that do not depend on the stage XCH_HOOK_HEAD waits for, then — in the first trip — the wait, then the rest.
  //      (A further trip evaluates its first part behind the wait: the same values, the rare shape.)
  if constexpr (SH) {
  for (int e0 = 0; e0 < MR * NO; e0 += NTH) {
    const int e = e0 + tid;
    const int sh_row = NO_CT == 1 ? e : e / NO, sh_j = e - sh_row * NO, sh_gr = r0 + sh_row;
    const bool sh_on = e < MR * NO && sh_gr < rows;
    float sh_v0 = 0.0f, sh_v1 = 0.0f, sh_v2 = 0.0f, sh_v3 = 0.0f, sh_v4 = 0.0f, sh_alpha = 0.0f, sh_glp = 0.0f;
    bool sh_gate = false;
    size_t sh_at = 0;
    if constexpr (LOSS_CT == LOSS_SAC_CRITIC) {
      // sac_alpha.py:110-123: y = r + (1-d)*gamma*(min(TQ1,TQ2) - alpha*logpi'); dL/dq = (q-y)/B.  alpha: the including scope has waited for the
      // deferred tail (one value for the launch: kept as a scalar); reward, done and this critic's own q are stage 1's
      const DevScalars* scal = T.scal ? T.scal : A.scal;
      sh_alpha = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ldx_uniform<XCH>(&scal->alpha))));
      if (sh_on) {
        sh_v0 = A.reward_scale * ldx<XCH>(T.rew + sh_gr);
        sh_v1 = (1.0f - ldx<XCH>(T.done + sh_gr)) * A.gamma;
        sh_v2 = partval_get<XCH, CS>(T.q.p, T.q.stride, sh_gr);
      }
    }
    if constexpr (LOSS_CT == LOSS_SAC_POLICY) {
      // SURVEY Appendix A.1/A.2 ; j < a -> d mu_j, else d log_std_raw_{j-a}: everything but the critics' dQ/da (raw head, noise and action
      // are the previous launch's)
      const DevScalars* scal = T.scal ? T.scal : A.scal;
      const int a = NO >> 1, jj = sh_j < a ? sh_j : sh_j - a;
      const float alpha = scal->alpha;
      sh_glp = alpha * A.inv_B;
      const float inv_Ba = A.inv_B / (float)a;
      if (sh_on) {
        const float mu = ldx<XCH>(T.raw + (size_t)sh_gr * NO + jj), lsr = ldx<XCH>(T.raw + (size_t)sh_gr * NO + a + jj);
        const float ep = ldx<XCH>(T.eps + (size_t)sh_gr * a + jj), act = ldx<XCH>(T.action + (size_t)sh_gr * a + jj);
        const float ls = fminf(fmaxf(lsr, LOG_SIG_MIN), LOG_SIG_MAX);
        const float sd = expf(ls);
        const float om = 1.0f - act * act;
        sh_v0 = om;
        sh_v1 = sh_glp * (2.0f * act * om / (om + TANH_EPS));
        sh_v2 = sh_j < a ? 2.0f * A.w_mu * mu * inv_Ba : 2.0f * A.w_std * ls * inv_Ba;
        sh_v3 = sd; sh_v4 = ep;
        sh_gate = lsr >= LOG_SIG_MIN && lsr <= LOG_SIG_MAX;
        sh_at = (size_t)sh_gr * a + jj;
      }
    }
    if (e0 == 0) { XCH_HOOK_HEAD }
    // ---- head gradient (every slice recomputes it; the lead slice publishes it for the dW kernel)
    float d = 0.0f;
    if (sh_on) {
      if constexpr (LOSS_CT == LOSS_SAC_CRITIC) {
        const float t1 = partval_get<XCH, CS>(sh_p0, sh_i0, sh_gr), t2 = partval_get<XCH, CS>(sh_p1, sh_i1, sh_gr), lpn = ldx<XCH>(xg<true>(sh_p2 + sh_gr));
        const float y = sh_v0 + sh_v1 * (fminf(t1, t2) - sh_alpha * lpn);
        d = (sh_v2 - y) * sh_invB;
      } else if constexpr (LOSS_CT == LOSS_SAC_ACTORQ) {
        // sac_alpha.py:144-148: -mean(min(Q1,Q2)); torch.minimum splits ties evenly
        const float a1 = partval_get<XCH, CS>(sh_p0, sh_i0, sh_gr), a2 = partval_get<XCH, CS>(sh_p1, sh_i1, sh_gr);
        const float w1 = a1 < a2 ? 1.0f : (a1 == a2 ? 0.5f : 0.0f);
        d = -(sh_which == 0 ? w1 : 1.0f - w1) * sh_invB;
      } else {
        float ga = 0.0f;  // d(-min Q)/da~: both critics, each in CS column-slice partial slabs, all requested before any is summed
        float g1[4], g2[4];
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
          const size_t at = (size_t)(pc < CS ? pc : 0) * sh_i0 + sh_at;
          const float v1 = ldx<XCH>(xg<true>(sh_p0 + at)), v2 = ldx<XCH>(xg<true>(sh_p1 + at));
          g1[pc] = pc < CS ? v1 : 0.0f; g2[pc] = pc < CS ? v2 : 0.0f;
        }
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) ga += g1[pc] + g2[pc];
        const float dz = ga * sh_v0 + sh_v1;
        if (sh_j < (NO >> 1)) d = dz + sh_v2;
        else d = sh_gate ? dz * sh_v3 * sh_v4 - sh_glp + sh_v2 : 0.0f;
      }
      if (sh_dhead) xg<true>(sh_dhead)[(size_t)sh_gr * NO + sh_j] = d;
    }
    if (e < MR * NO) dout[sh_row * ILSX_MAX_NO + sh_j] = d;
    if constexpr (NO_CT == 1) break;   // 16 elements
  }
  } else {
  for (int e = tid; e < MR * NO; e += NTH) {  // only the NO live outputs per row: one pass, loads batched
    const int row = e / NO, j = e - row * NO, gr = r0 + row;
    float d = 0.0f;
    if (gr < rows) {
      d = bwd_head_grad<XCH, LOSS_CT>(T, A, gr, j, NO);
      if (T.dhead && lead) T.dhead[(size_t)gr * NO + j] = d;
    }
    dout[row * ILSX_MAX_NO + j] = d;
  }
  }
  constexpr bool LATEW = GRP == 3 && !XCH;
  if constexpr (!XCH && !LATEW) {
  // ---- this wave's slice of W_1 (backward-packed: all H rows x its 16 columns), one coalesced burst
    {
      const float* wp = N.base + N.off_Wb[1] + (size_t)(cs * NWV + wave) * NC * 256 + 4 * lane;
#pragma unroll
      for (int c = 0; c < NC; ++c) wreg[c] = *reinterpret_cast<const float4*>(wp + 256 * c);
    }
  }
  lds_barrier();
  XCH_STAMP(1);
  // ---- delta_1 = (dout Wh) * act'(h_1), full width on the VALU: thread <-> column k1
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const float* Wh = SH ? sh_Wh : N.base + N.off_Wh;
    const float* dom = dout + 16 * m * ILSX_MAX_NO;
    float accd[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) accd[i] = 0.0f;
    if constexpr (SH && NO_CT != 1) {
      // A static stage with a wide head (the policy).  NO <= 16 (a <= 8): the tile's head gradients — 16 rows x NO — are read from LDS ONCE
      // per wave, RPT / 4 words per lane (lane (g, li) of word q holds row rb1 + RSTEP (4 q + g), output li; outputs >= NO are read and not
      // used), and every (row, output) the thread's column needs is a lane of those words at a compile-time index, broadcast through a scalar
      // register — instead of RPT x NO LDS reads per thread with their waits.  The fma chain over j per element is the one below.
      static_assert(WHP == 16 && RPT % 4 == 0, "one lane per (row of four, output below 16)");
      if (NO <= 16) {
        int dreg[RPT / 4];
#pragma unroll
        for (int q = 0; q < RPT / 4; ++q) dreg[q] = __float_as_int(dom[(rb1 + RSTEP * (4 * q + g)) * ILSX_MAX_NO + li]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if (j < NO) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) accd[i] = fmaf(__int_as_float(__builtin_amdgcn_readlane(dreg[i >> 2], (i & 3) * 16 + j)), whp[j], accd[i]);
          }
        }
      } else {   // a wider head (a > 8): output by output
#pragma unroll 1
        for (int j = 0; j < NO; ++j) {
          const float w = xg<SH>(Wh)[(size_t)j * H + k1];
#pragma unroll
          for (int i = 0; i < RPT; ++i) accd[i] = fmaf(dom[(rb1 + RSTEP * i) * ILSX_MAX_NO + j], w, accd[i]);
        }
      }
    } else {
#pragma unroll
    for (int j = 0; j < WHP; ++j) {   // head rows requested at kernel entry (critics: 1, Hopper / Walker policies: 6 / 12)
      if (j < NO) {
#pragma unroll
        for (int i = 0; i < RPT; ++i) accd[i] = fmaf(dom[(rb1 + RSTEP * i) * ILSX_MAX_NO + j], whp[j], accd[i]);
      }
    }
#pragma unroll 4
    for (int j = WHP; j < NO; ++j) {
      const float w = xg<SH>(Wh)[(size_t)j * H + k1];
#pragma unroll
      for (int i = 0; i < RPT; ++i) accd[i] = fmaf(dom[(rb1 + RSTEP * i) * ILSX_MAX_NO + j], w, accd[i]);
    }
    }
    float* ds = SH ? sh_ds1 : lead ? T.dsave[1] : nullptr;
    float* const dsp = ds ? ds + (size_t)(r0 + 16 * m + rb1) * H + k1 : nullptr;
    if (full_tile) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const float dv = accd[i] * act_grad_from_out<ACT>(h1v[m][i]);
        if (ds) xg<SH>(dsp)[(size_t)(RSTEP * i) * H] = dv;
        d1[(16 * m + rb1 + RSTEP * i) * LDH + k1] = dv;
      }
    } else {
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int row = 16 * m + rb1 + RSTEP * i, gr = r0 + row;
        float dv = 0.0f;
        if (gr < rows) {
          dv = accd[i] * act_grad_from_out<ACT>(h1v[m][i]);
          if (ds) xg<SH>(dsp)[(size_t)(RSTEP * i) * H] = dv;
        }
        d1[row * LDH + k1] = dv;
      }
    }
  }
  if constexpr (LATEW) {
    const float* wp = N.base + N.off_Wb[1] + (size_t)(cs * NWV + wave) * NC * 256 + 4 * lane;
#pragma unroll
    for (int c = 0; c < NC; ++c) wreg[c] = *reinterpret_cast<const float4*>(wp + 256 * c);
  }
  lds_barrier();
  XCH_STAMP(2);
  // ---- delta_0 slice = (delta_1 W_1)[:, slice] * act'(h_0[:, slice])
  {
    f32x4 acc0[MT], acc1[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) { acc0[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[m] = acc0[m]; }
    const float* ap = d1 + li * LDH + 4 * g;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {   // one fetched B fragment, MT row tiles
        const float4 a = *reinterpret_cast<const float4*>(ap + m * 16 * LDH + 16 * c);
        acc0[m] = MFMA16(a.x, wreg[c].x, acc0[m]); acc1[m] = MFMA16(a.y, wreg[c].y, acc1[m]);
        acc0[m] = MFMA16(a.z, wreg[c].z, acc0[m]); acc1[m] = MFMA16(a.w, wreg[c].w, acc1[m]);
      }
    }
    float* ds = T.dsave[0];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float* const drow = ds ? ds + (size_t)(r0 + 16 * m + 4 * g) * H + col0 : nullptr;
      if (full_tile) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float dv = (acc0[m][v] + acc1[m][v]) * act_grad_from_out<ACT>(h0v[m][v]);
          if (ds) drow[v * H] = dv;
          d0s[(16 * m + 4 * g + v) * LDSL + lc] = dv;
        }
      } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 16 * m + 4 * g + v, gr = r0 + row;
          float dv = 0.0f;
          if (gr < rows) {
            dv = (acc0[m][v] + acc1[m][v]) * act_grad_from_out<ACT>(h0v[m][v]);
            if (ds) drow[v * H] = dv;
          }
          d0s[row * LDSL + lc] = dv;
        }
      }
    }
  }
  XCH_STAMP(3);
  // ---- partial dL/dx over this slice of the H contraction, on the matrix pipe: dx[16 rows][dx_cols] = d0s[16][SLW] . W0[slice][cols].
  //      (The first version reduced every (row, column) with a 6-step wave shuffle: 12 dependent butterflies per wave were 3 us of the
  //      actor's critic-backward launch.)  Wave w contracts k16 chunk w; the NWV partial tiles are summed through LDS in wave order.
  if (T.dx) {
    lds_barrier();
    float* red = d1;   // delta_1 is dead (every wave passed the barrier above after its last read): [MT][DXT][NWV][4][64] floats
    const int ntile = (T.dx_cols + 15) >> 4;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float4 a4 = *reinterpret_cast<const float4*>(d0s + (16 * m + li) * LDSL + 16 * wave + 4 * g);
#pragma unroll
      for (int t = 0; t < DXT; ++t) {
        if (t < ntile) {
          f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
          acc = MFMA16(a4.x, w0b[t][0], acc); acc = MFMA16(a4.y, w0b[t][1], acc);
          acc = MFMA16(a4.z, w0b[t][2], acc); acc = MFMA16(a4.w, w0b[t][3], acc);
#pragma unroll
          for (int v = 0; v < 4; ++v) red[(((m * DXT + t) * NWV + wave) * 4 + v) * 64 + lane] = acc[v];
        }
      }
    }
    lds_barrier();
#pragma unroll
    for (int m = 0; m < MT; ++m)
    for (int e = tid; e < ntile * 256; e += NTH) {
      const int t = e >> 8, v = (e >> 6) & 3, ol = e & 63;
      float sum = 0.0f;
#pragma unroll
      for (int w2 = 0; w2 < NWV; ++w2) sum += red[(((m * DXT + t) * NWV + w2) * 4 + v) * 64 + ol];
      const int row = 16 * m + 4 * (ol >> 4) + v, c = 16 * t + (ol & 15), gr = r0 + row;
      if (c < T.dx_cols && gr < rows) stx<XCH>(T.dx + ((size_t)cs * A.part_stride + gr) * T.dx_cols + c, sum);
    }
  }
  ILSX_STAMP(A.dbg, 7);
