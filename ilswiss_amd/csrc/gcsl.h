// gcsl.h — goal-conditioned supervised learning (rlkit/torch/algorithms/gcsl/gcsl.py) on the device: the horizon relabel gather and the
// BatchNorm categorical policy (CatagorialConditionPolicy(batch_norm=True): networks.py:118-145 CatagorialMlp, policies.py:759-840) trained by
// cross-entropy in GCSL's CLASS mode.
//
//   horizon gather    HindsightHorizonReplayBuffer.random_batch (relabel_horizon_replay_buffer.py:163-270) with her_ratio 1: every row's goal is
//                     the NEXT achieved goal of its relabel record, and horizons[b][j] = (j >= idx_relabel[b] - idx[b]) on RAW ring indices
//                     (no modulo: a trajectory that wraps the ring yields a negative length, an all-ones row — the reference's behaviour, kept).
//                     One launch writes X = observation | goal | horizon [B][d_obs + d_goal + T] and the action (float rows, or int32 class
//                     indices truncated like torch's .long()).
//   BN categorical    every hidden block Linear -> BatchNorm1d -> ReLU (the phases of disc_bn.h), then last_fc (no BN) -> logits [rows][n].
//     train step      forward with batch statistics (parked for the running update) ; a ROW phase per batch row: max-shifted softmax
//                     cross-entropy, dlogit = (p - onehot(y)) / B, a correct flag (argmax of the probabilities, first maximum) ; head weight
//                     gradients and the cotangent of the top block ; dbn_col_bwd + the dense phases down the blocks ; one last launch with
//                     the statistics (mean CE, accuracy, summed in a fixed order), the running-statistics update and torch-1.9 Adam.
//     eval forward    running statistics ; softmax probabilities and argmax per row (the stochastic draw is device-only: ilsx_gcsl.hip).
// The step is written once against a launcher `LN` (par / col / gemm, disc_bn_step.h) so that the same text runs as kernels (ilsx_gcsl.hip)
// and, under DBN_HOST_EMU, as serial loops (tests/harness/gcsl_bn_host.cpp).
#pragma once
#include "disc_bn.h"

#ifdef DBN_HOST_EMU
#define GCSL_LAMBDA [=]
#else
#define GCSL_LAMBDA [=] __device__
#endif

#define GCSL_MAX_BLK 3
#define GCSL_MAX_NO 64   // classes: one wavefront lane per class in the row phases

#ifdef DBN_HOST_EMU
static inline float gcsl_wmax(float v) { return v; }
static inline void gcsl_wargmax(float& v, int& j) {}
#else
__device__ __forceinline__ float gcsl_wmax(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// (value, index) -> the largest value, the smallest index among equal values: torch.argmax's first maximum
__device__ __forceinline__ void gcsl_wargmax(float& v, int& j) {
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oj = __shfl_xor(j, o, 64);
    if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
  }
}
#endif

// ---- horizon gather: element e of [B][D], D = d_obs + dg + T.  Ring record (ilsx_replay, observation segment observation | desired_goal |
// achieved_goal of width o = d_obs + 2 dg): obs [o] | action [a] | reward | done | next obs [o].  mode 0: act[r][c] = action floats (c < a),
// mode 1: label[r] = (int) action[0].  Indices must lie in [0, capacity): the device kernel (k_her_horizon_gather, ilsx_gcsl.hip) checks
// them before calling this and writes a row with an index outside the ring as zeros (label -1); the host harness passes valid ones.
DBN_HD void gcsl_gather_elem(int e, const float* data, int rec, const long long* idx, const long long* idx_rel, int d_obs, int dg, int a, int T,
                             int mode, float* X, float* act, int* label) {
  const int D = d_obs + dg + T, r = e / D, c = e - r * D, o = d_obs + 2 * dg;
  const float* R = data + (size_t)idx[r] * rec;
  float v;
  if (c < d_obs) {
    v = R[c];
  } else if (c < d_obs + dg) {
    v = data[(size_t)idx_rel[r] * rec + o + a + 2 + d_obs + dg + (c - d_obs)];   // next achieved goal of the relabel record
  } else {
    const long long len = idx_rel[r] - idx[r];
    v = (long long)(c - d_obs - dg) >= len ? 1.0f : 0.0f;
  }
  X[(size_t)r * D + c] = v;
  if (mode == 0 && c < a) act[(size_t)r * a + c] = R[o + c];
  if (mode == 1 && c == 0) label[r] = (int)R[o];   // truncation toward zero, as .long()
}

// parameters in torch's parameters() order: per block W [H][in] | b [H] | gamma [H] | beta [H] ; then Wo [n][H] | bo [n]
struct GcslNet {
  int D, H, nblk, n;
  float *P, *G, *M, *V;   // n_params floats each
  float *rmean, *rvar;    // [nblk][H]
  DBN_HDH int in_of(int l) const { return l == 0 ? D : H; }
  DBN_HDH int off_W(int l) const { int o = 0; for (int i = 0; i < l; ++i) o += H * in_of(i) + 3 * H; return o; }
  DBN_HDH int off_b(int l) const { return off_W(l) + H * in_of(l); }
  DBN_HDH int off_g(int l) const { return off_b(l) + H; }
  DBN_HDH int off_be(int l) const { return off_b(l) + 2 * H; }
  DBN_HDH int off_Wo() const { return off_W(nblk); }
  DBN_HDH int off_bo() const { return off_Wo() + n * H; }
  DBN_HDH int n_params() const { return off_bo() + n; }
};
// workspace for up to `rows` rows
struct GcslWs {
  float* X;                 // [rows][D] the gathered input (the horizon gather writes it)
  int* label;               // [rows] class targets
  float *ch[GCSL_MAX_BLK], *ah[GCSL_MAX_BLK], *h[GCSL_MAX_BLK], *p[GCSL_MAX_BLK], *s[GCSL_MAX_BLK];   // forward tape
  float *t0, *t1;           // [rows][H] cotangent scratch
  float *logit, *dlogit;    // [rows][n]
  float *ce_row, *correct;  // [rows]
  float* bstat;             // [nblk][mean | var][H]
};

// ---- row phases: one wavefront per row r, lanes over the classes (host emulation: one lane walks them all)
// cross-entropy of row r against label y: m = max_j z_j ; S = sum_j exp(z_j - m) ; ce = -((z_y - m) - log S) ; p_j = exp(z_j - m) / S ;
// dlogit_j = (p_j - [j == y]) / B ; correct = (first argmax_j p_j == y).  A label outside [0, n) gives ce = NaN and no one-hot term.
DBN_HD void gcsl_row_ce(int r, int lane, const float* logit, const int* label, int n, int B, float* dlogit, float* ce_row, float* correct) {
  const float* z = logit + (size_t)r * n;
  float m = -INFINITY;
  for (int j = lane; j < n; j += DBN_LANES) m = fmaxf(m, z[j]);
  m = gcsl_wmax(m);
  float S = 0.0f;
  for (int j = lane; j < n; j += DBN_LANES) S += expf(z[j] - m);
  S = dbn_wsum(S);
  const int y = label[r];
  const bool ok = y >= 0 && y < n;
  float bv = -INFINITY;
  int bj = 0x7fffffff;
  for (int j = lane; j < n; j += DBN_LANES) {
    const float pj = expf(z[j] - m) / S;
    if (pj > bv) { bv = pj; bj = j; }
    dlogit[(size_t)r * n + j] = (pj - (j == y ? 1.0f : 0.0f)) / (float)B;
  }
  gcsl_wargmax(bv, bj);
  if (lane == 0) {
    ce_row[r] = ok ? -((z[y] - m) - logf(S)) : NAN;
    correct[r] = (ok && bj == y) ? 1.0f : 0.0f;
  }
}
// eval rows: probabilities (nullable) and the first argmax of them (nullable, as a float index)
DBN_HD void gcsl_row_probs(int r, int lane, const float* logit, int n, float* probs, float* amax) {
  const float* z = logit + (size_t)r * n;
  float m = -INFINITY;
  for (int j = lane; j < n; j += DBN_LANES) m = fmaxf(m, z[j]);
  m = gcsl_wmax(m);
  float S = 0.0f;
  for (int j = lane; j < n; j += DBN_LANES) S += expf(z[j] - m);
  S = dbn_wsum(S);
  float bv = -INFINITY;
  int bj = 0x7fffffff;
  for (int j = lane; j < n; j += DBN_LANES) {
    const float pj = expf(z[j] - m) / S;
    if (pj > bv) { bv = pj; bj = j; }
    if (probs) probs[(size_t)r * n + j] = pj;
  }
  gcsl_wargmax(bv, bj);
  if (lane == 0 && amax) amax[r] = (float)bj;
}
// column sum of a [rows][n] matrix (lanes split the rows): out[c] = sum_r v[r][c]       (the output bias gradient: sum_r dlogit)
DBN_HD void gcsl_col_sum(int c, int lane, const float* v, int rows, int n, float* out) {
  float a = 0.0f;
  for (int r = lane; r < rows; r += DBN_LANES) a += v[(size_t)r * n + c];
  a = dbn_wsum(a);
  if (lane == 0) out[c] = a;
}

// ---- the phase lists
// forward of `rows` rows of x [rows][D] to the logits; train: batch statistics parked in W.bstat (no running update here), eval: running statistics
template <class LN>
void gcsl_forward(LN& L, const GcslNet& N, const GcslWs& W, const float* x, int rows, int train) {
  const int H = N.H;
  const float* in = x;
  int K = N.D;
  for (int l = 0; l < N.nblk; ++l) {
    const float *Wl = N.P + N.off_W(l), *bl = N.P + N.off_b(l), *gl = N.P + N.off_g(l), *bel = N.P + N.off_be(l);
    float *ch = W.ch[l], *ah = train ? W.ah[l] : nullptr, *h = W.h[l], *p = train ? W.p[l] : nullptr, *s = train ? W.s[l] : nullptr;
    float *rm = N.rmean + (size_t)l * H, *rv = N.rvar + (size_t)l * H, *bs = train ? W.bstat + (size_t)l * 2 * H : nullptr;
    const int Kl = K;
    L.gemm(dbn_g_dense(in, Kl, Wl, bl, ch, rows, H, Kl));
    L.col(H, GCSL_LAMBDA(int j, int lane) { dbn_col_fwd(j, lane, ch, ah, h, p, s, gl, bel, rm, rv, rows, H, DBN_RELU, train, 0, bs); });
    in = h; K = H;
  }
  L.gemm(dbn_g_dense(in, H, N.P + N.off_Wo(), N.P + N.off_bo(), W.logit, rows, N.n, H));
}

// eval-mode probabilities / argmax of `rows` rows of x (CatagorialPolicy.forward in eval mode, deterministic=True)
template <class LN>
void gcsl_eval(LN& L, const GcslNet& N, const GcslWs& W, const float* x, int rows, float* probs, float* amax) {
  gcsl_forward(L, N, W, x, rows, 0);
  const float* lg = W.logit;
  const int n = N.n;
  L.col(rows, GCSL_LAMBDA(int r, int lane) { gcsl_row_probs(r, lane, lg, n, probs, amax); });
}

// GCSL.train_step in CLASS mode on W.X / W.label (B rows): cross-entropy gradients into N.G (every word ASSIGNED: no zeroing launch), then
// stats[0] = mean CE, stats[1] = accuracy, the running-statistics update (torch: momentum 0.1, unbiased variance) and Adam(lr, (0.9, 0.999),
// eps 1e-8) with step count t (1-based).  Launches: 2 per block forward + head + CE rows + head gradients + 2 per block backward + finish.
template <class LN>
void gcsl_cat_step(LN& L, const GcslNet& N, const GcslWs& W, int B, float* stats, float lr, int t) {
  const int H = N.H, nb = N.nblk, n = N.n;
  gcsl_forward(L, N, W, W.X, B, 1);
  {
    const float* lg = W.logit;
    const int* lab = W.label;
    float *dl = W.dlogit, *ce = W.ce_row, *co = W.correct;
    L.col(B, GCSL_LAMBDA(int r, int lane) { gcsl_row_ce(r, lane, lg, lab, n, B, dl, ce, co); });
  }
  float* G = N.G;
  const float *dl = W.dlogit, *hL = W.h[nb - 1], *Wo = N.P + N.off_Wo();
  L.gemm(dbn_g_outer(dl, hL, H, G + N.off_Wo(), B, n, H, 0),    // dWo = dlogit^T h_L
         dbn_g_dense_t(dl, Wo, W.t1, B, n, H));                  // cotangent of h_L = dlogit Wo
  const float* uh = W.t1;
  for (int l = nb - 1; l >= 0; --l) {
    const float *gl = N.P + N.off_g(l), *Wl = N.P + N.off_W(l), *pl = W.p[l], *ahl = W.ah[l], *sl = W.s[l];
    const float* xin = l > 0 ? W.h[l - 1] : W.X;
    float *ua = W.t0, *dg = G + N.off_g(l), *dbe = G + N.off_be(l), *db = G + N.off_b(l), *dW = G + N.off_W(l), *dbo = G + N.off_bo();
    const int K = N.in_of(l), top = l == nb - 1;
    const float* uhl = uh;
    L.col(H + (top ? n : 0), GCSL_LAMBDA(int j, int lane) {
      if (j < H) dbn_col_bwd(j, lane, uhl, nullptr, nullptr, pl, ahl, sl, gl, ua, nullptr, nullptr, nullptr, nullptr, nullptr, dg, dbe, db, B, H, 0);
      else gcsl_col_sum(j - H, lane, dl, B, n, dbo);   // the output bias: dbo = sum_r dlogit (top block's launch)
    });
    if (l > 0) L.gemm(dbn_g_outer(ua, xin, K, dW, B, H, K, 0), dbn_g_dense_t(ua, Wl, W.t1, B, H, K));
    else L.gemm(dbn_g_outer(ua, xin, K, dW, B, H, K, 0));
    uh = W.t1;
  }
  // the last launch: statistics (one wavefront), running statistics (lanes over block x column), Adam (lanes over the parameters)
  const float *ce = W.ce_row, *co = W.correct, *bstat = W.bstat;
  const double bc1 = 1.0 - pow(0.9, (double)t), bc2 = 1.0 - pow(0.999, (double)t);
  const float step = (float)((double)lr / bc1), bc2s = (float)sqrt(bc2);
  float *P = N.P, *M = N.M, *V = N.V, *rmean = N.rmean, *rvar = N.rvar;
  const int nbh = nb * H, np = N.n_params();
  const int cr = (nbh + DBN_LANES - 1) / DBN_LANES, ca = (np + DBN_LANES - 1) / DBN_LANES;
  L.col(1 + cr + ca, GCSL_LAMBDA(int j, int lane) {
    if (j == 0) {
      float a = 0.0f, b = 0.0f;
      for (int r = lane; r < B; r += DBN_LANES) { a += ce[r]; b += co[r]; }
      a = dbn_wsum(a); b = dbn_wsum(b);
      if (lane == 0) { stats[0] = a / (float)B; stats[1] = b / (float)B; }
    } else if (j <= cr) {
      const int idx = (j - 1) * DBN_LANES + lane;
      if (idx < nbh) dbn_running_update(idx, rmean, rvar, bstat, nb, H, B, 0);
    } else {
      const int i = (j - 1 - cr) * DBN_LANES + lane;
      if (i < np) dbn_adam(i, P, G, M, V, step, bc2s, 0.9f, 0.999f, 1e-8f);
    }
  });
}
