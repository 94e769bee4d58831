// ilsx_gcsl.hip — GCSL (rlkit/torch/algorithms/gcsl/): the horizon relabel gather, the BatchNorm categorical policy (`ilsx_bncat`) and the
// GCSL trainer (`ilsx_gcsl`).  The phases and their order are csrc/gcsl.h; every phase is one launch on the ctx stream (DbnLaunch of
// disc_bn_launch.h).  CLASS mode trains an ilsx_bncat by cross-entropy; MSE mode drives an ilsx_bc in MSE mode (LOSS_BC_MSE on the fused
// MLP kernels) with its noise held at zero, so its sampled action is tanh(mean): GCSL's max_act * tanh(last_fc) with max_act = 1.
#include "host_common.h"
#include "disc_bn.h"
#include "gcsl.h"

namespace gcsl_dev {   // this translation unit's own instances of the BN launcher kernels
#include "disc_bn_launch.h"
}
using gcsl_dev::DbnLaunch;

// one thread per element of X [B][d_obs + d_goal + T]; a row whose record index lies outside the ring is written as zeros (label -1)
__global__ __launch_bounds__(256) void k_her_horizon_gather(const float* __restrict__ data, int rec, long long cap, const long long* __restrict__ idx,
                                                            const long long* __restrict__ idx_rel, int B, int d_obs, int dg, int a, int T, int mode,
                                                            float* __restrict__ X, float* __restrict__ act, int* __restrict__ label) {
  const int D = d_obs + dg + T, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * D) return;
  const int r = e / D, c = e - r * D;
  const long long i0 = idx[r], i1 = idx_rel[r];
  if (i0 < 0 || i0 >= cap || i1 < 0 || i1 >= cap) {
    X[e] = 0.0f;
    if (mode == 0 && c < a) act[(size_t)r * a + c] = 0.0f;
    if (mode == 1 && c == 0) label[r] = -1;
    return;
  }
  gcsl_gather_elem(e, data, rec, idx, idx_rel, d_obs, dg, a, T, mode, X, act, label);
}

extern "C" int ilsx_her_horizon_gather(ilsx_replay* rb, const int64_t* idx, const int64_t* idx_relabel, int B, int d_obs, int d_goal, int T,
                                       int mode, float* X, float* act, int32_t* label) {
  if (!rb || !idx || !idx_relabel || !X || B < 1 || T < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_her_horizon_gather: bad argument");
  if (mode != 0 && mode != 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_her_horizon_gather: mode must be 0 (float actions) or 1 (class indices)");
  if ((mode == 0 && !act) || (mode == 1 && !label)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_her_horizon_gather: NULL action output");
  if (d_obs < 1 || d_goal < 1 || d_obs + 2 * d_goal != rb->o)
    ILSX_FAIL(ILSX_ERR_ARG, "ilsx_her_horizon_gather: ring observation width %d != d_obs %d + 2 * d_goal %d", rb->o, d_obs, d_goal);
  if (rb->size < 1) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_her_horizon_gather: buffer is empty");
  HIPCHK(hipSetDevice(rb->ctx->device));
  const int total = B * (d_obs + d_goal + T);
  hipLaunchKernelGGL(k_her_horizon_gather, dim3((total + 255) / 256), dim3(256), 0, rb->ctx->stream, rb->data, rb->rec, (long long)rb->cap,
                     (const long long*)idx, (const long long*)idx_relabel, B, d_obs, d_goal, rb->a, T, mode, X, act, (int*)label);
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// ------------------------------------------------------------------------------------------------ BatchNorm categorical policy
struct ilsx_bncat {
  ilsx_ctx* ctx = nullptr;
  GcslNet N;
  GcslWs W;
  int rows = 0;                // workspace rows
  int64_t t = 0;               // Adam step count
  unsigned long long draws = 0;   // Philox counter of the stochastic act calls
  uint32_t rng_stream = 0;
  float* stats = nullptr;      // device [2]: mean CE, accuracy of the last step
  DevOwner own;
};

extern "C" int ilsx_bncat_destroy(ilsx_bncat* b) {
  if (!b) return ILSX_OK;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->own.release();
  delete b;
  return ILSX_OK;
}

// parameters, running statistics and the step workspace of a new policy
static int bncat_setup(ilsx_bncat* b) {
  GcslNet& N = b->N;
  GcslWs& W = b->W;
  const size_t np = (size_t)N.n_params(), H = (size_t)N.H, R = (size_t)b->rows, nb = (size_t)N.nblk;
  auto A = [&](float** p, size_t cnt) { return b->own.alloc(p, cnt); };
  for (float** p : {&N.P, &N.G, &N.M, &N.V}) ILSX_TRY(A(p, np));
  ILSX_TRY(A(&N.rmean, nb * H)); ILSX_TRY(A(&N.rvar, nb * H));
  ILSX_TRY(A(&W.X, R * N.D));
  ILSX_TRY(A((float**)&W.label, R));
  for (int l = 0; l < N.nblk; ++l) {
    for (float** p : {&W.ch[l], &W.ah[l], &W.h[l], &W.p[l]}) ILSX_TRY(A(p, R * H));
    ILSX_TRY(A(&W.s[l], H));
  }
  ILSX_TRY(A(&W.t0, R * H)); ILSX_TRY(A(&W.t1, R * H));
  ILSX_TRY(A(&W.logit, R * N.n)); ILSX_TRY(A(&W.dlogit, R * N.n));
  ILSX_TRY(A(&W.ce_row, R)); ILSX_TRY(A(&W.correct, R));
  ILSX_TRY(A(&W.bstat, nb * 2 * H));
  ILSX_TRY(A(&b->stats, 2));
  // BatchNorm1d's initial running statistics: mean 0, variance 1 — on the ctx stream, behind the zeroing of the allocation
  std::vector<float> ones(nb * H, 1.0f);
  HIPCHK(hipMemcpyAsync(N.rvar, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}

extern "C" int ilsx_bncat_create(ilsx_ctx* ctx, int in_dim, int hidden, int n_blocks, int n_classes, int max_rows, ilsx_bncat** out) {
  if (!ctx || !out) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_create: NULL argument");
  if (in_dim < 1 || hidden < 1 || hidden > 4096) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_create: in_dim=%d hidden=%d", in_dim, hidden);
  if (n_blocks < 1 || n_blocks > GCSL_MAX_BLK) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_bncat_create: n_blocks=%d not in 1..%d", n_blocks, GCSL_MAX_BLK);
  if (n_classes < 1 || n_classes > GCSL_MAX_NO) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_bncat_create: n_classes=%d not in 1..%d", n_classes, GCSL_MAX_NO);
  if (max_rows < 2 || max_rows > (1 << 20)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_create: max_rows=%d out of range", max_rows);
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_bncat* b = new ilsx_bncat();
  b->ctx = b->own.ctx = ctx;
  b->rows = max_rows;
  b->rng_stream = ctx->next_rng_stream++;
  GcslNet& N = b->N;
  N.D = in_dim; N.H = hidden; N.nblk = n_blocks; N.n = n_classes;
  int rc = bncat_setup(b);
  if (rc != ILSX_OK) { ilsx_bncat_destroy(b); return rc; }
  *out = b;
  return ILSX_OK;
}

extern "C" int ilsx_bncat_num_params(const ilsx_bncat* b, int* n) {
  if (!b || !n) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_num_params: NULL argument");
  *n = b->N.n_params();
  return ILSX_OK;
}

static float* bncat_array(ilsx_bncat* b, int which, size_t* cnt) {
  const size_t np = (size_t)b->N.n_params(), nr = (size_t)b->N.nblk * b->N.H;
  switch (which) {
    case ILSX_BNCAT_PARAMS: *cnt = np; return b->N.P;
    case ILSX_BNCAT_RUNNING_MEAN: *cnt = nr; return b->N.rmean;
    case ILSX_BNCAT_RUNNING_VAR: *cnt = nr; return b->N.rvar;
    case ILSX_BNCAT_ADAM_M: *cnt = np; return b->N.M;
    case ILSX_BNCAT_ADAM_V: *cnt = np; return b->N.V;
    default: return nullptr;
  }
}
extern "C" int ilsx_bncat_get(ilsx_bncat* b, int which, float* dst_host, size_t n) {
  if (!b || !dst_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_get: NULL argument");
  size_t cnt = 0;
  float* src = bncat_array(b, which, &cnt);
  if (!src) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_get: which=%d unknown", which);
  if (n != cnt) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_get: n=%zu, expected %zu", n, cnt);
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipMemcpyAsync(dst_host, src, cnt * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}
extern "C" int ilsx_bncat_set(ilsx_bncat* b, int which, const float* src_host, size_t n) {
  if (!b || !src_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_set: NULL argument");
  size_t cnt = 0;
  float* dst = bncat_array(b, which, &cnt);
  if (!dst) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_set: which=%d unknown", which);
  if (n != cnt) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_set: n=%zu, expected %zu", n, cnt);
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipMemcpyAsync(dst, src_host, cnt * sizeof(float), hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}
extern "C" int ilsx_bncat_get_meta(const ilsx_bncat* b, int64_t* t, uint64_t* draws) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_get_meta: NULL argument");
  if (t) *t = b->t;
  if (draws) *draws = b->draws;
  return ILSX_OK;
}
extern "C" int ilsx_bncat_set_meta(ilsx_bncat* b, int64_t t, uint64_t draws) {
  if (!b || t < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_set_meta: bad argument");
  b->t = t;
  b->draws = draws;
  return ILSX_OK;
}
extern "C" int ilsx_bncat_input(ilsx_bncat* b, float** X, int32_t** label) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_input: NULL argument");
  if (X) *X = b->W.X;
  if (label) *label = (int32_t*)b->W.label;
  return ILSX_OK;
}

// one CLASS-mode step on the input buffer (ilsx_bncat_input), B rows; stats2_host (nullable): {CE Loss, Accuracy} of this batch (syncs)
extern "C" int ilsx_bncat_train_step(ilsx_bncat* b, int B, float lr, float* stats2_host) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_train_step: NULL argument");
  if (B < 2 || B > b->rows) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_train_step: B=%d not in 2..%d (batch statistics need 2 rows)", B, b->rows);
  HIPCHK(hipSetDevice(b->ctx->device));
  DbnLaunch L{b->ctx->stream};
  gcsl_cat_step(L, b->N, b->W, B, b->stats, lr, (int)(++b->t));
  HIPCHK(hipGetLastError());
  if (stats2_host) {
    HIPCHK(hipMemcpyAsync(stats2_host, b->stats, 2 * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
  }
  return ILSX_OK;
}

// eval mode (running statistics): act[r] = first argmax of the probabilities (deterministic) or a Gumbel-max draw — argmax_j z_j - log(-log u_j),
// u_j from Philox (row, j / 4, this call's counter) as k_categorical_act draws them — as a float index; probs (nullable) [rows][n].  x, act and
// probs are device pointers.
extern "C" int ilsx_bncat_act(ilsx_bncat* b, const float* x, int rows, int deterministic, float* act, float* probs) {
  if (!b || !x || rows < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_act: bad argument");
  if (rows > b->rows) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bncat_act: rows=%d > workspace rows %d", rows, b->rows);
  if (rows == 0) return ILSX_OK;
  HIPCHK(hipSetDevice(b->ctx->device));
  DbnLaunch L{b->ctx->stream};
  if (deterministic || !act) {
    gcsl_eval(L, b->N, b->W, x, rows, probs, act);
  } else {
    gcsl_eval(L, b->N, b->W, x, rows, probs, nullptr);
    const float* lg = b->W.logit;
    const int n = b->N.n;
    const uint64_t seed = b->ctx->seed;
    const uint32_t stream = b->rng_stream;
    const unsigned long long step = ++b->draws;
    L.col(rows, [=] __device__(int r, int lane) {
      float v = -INFINITY;
      int bj = 0x7fffffff;
      if (lane < n) {
        uint32_t c[4] = {(uint32_t)r, (uint32_t)(lane >> 2), (uint32_t)step, (uint32_t)(step >> 32) ^ (stream * 0x9E3779B9u)};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ stream);
        const int q = lane & 3;
        const uint32_t w = q == 0 ? c[0] : q == 1 ? c[1] : q == 2 ? c[2] : c[3];
        v = lg[(size_t)r * n + lane] - logf(-logf(u01_open(w)));
        bj = lane;
      }
      gcsl_wargmax(v, bj);
      if (lane == 0) act[r] = (float)bj;
    });
  }
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// ------------------------------------------------------------------------------------------------ GCSL trainer
struct ilsx_gcsl {
  ilsx_ctx* ctx = nullptr;
  ilsx_gcsl_cfg cfg;
  ilsx_bncat* cat = nullptr;   // CLASS
  ilsx_bc* bc = nullptr;       // MSE
  int a = 0;                   // MSE: action width
  float *X = nullptr, *act = nullptr, *zeros = nullptr;   // MSE: gathered input, actions, the BC trainer's (zero) noise
  DevOwner own;
};

extern "C" int ilsx_gcsl_destroy(ilsx_gcsl* g) {
  if (!g) return ILSX_OK;
  hipSetDevice(g->ctx->device);
  hipStreamSynchronize(g->ctx->stream);
  g->own.release();
  delete g;
  return ILSX_OK;
}

extern "C" int ilsx_gcsl_create(ilsx_ctx* ctx, const ilsx_gcsl_cfg* cfg, ilsx_bncat* cat, ilsx_bc* bc, int act_dim, ilsx_gcsl** out) {
  if (!ctx || !cfg || !out) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_create: NULL argument");
  if (cfg->mode != ILSX_GCSL_MSE && cfg->mode != ILSX_GCSL_CLASS) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_gcsl_create: mode=%d (MSE or CLASS)", cfg->mode);
  if ((cfg->mode == ILSX_GCSL_CLASS) != (cat != nullptr) || (cfg->mode == ILSX_GCSL_MSE) != (bc != nullptr))
    ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_create: CLASS mode takes an ilsx_bncat, MSE mode an ilsx_bc (MSE mode)");
  if (cfg->d_obs < 1 || cfg->d_goal < 1 || cfg->horizon < 0 || cfg->max_batch < 2) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_create: bad dimensions");
  const int D = cfg->d_obs + cfg->d_goal + cfg->horizon;
  if (cat && (cat->N.D != D || cat->rows < cfg->max_batch))
    ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_create: policy input %d / rows %d, expected %d / >= %d", cat->N.D, cat->rows, D, cfg->max_batch);
  if (bc && act_dim < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_create: act_dim=%d", act_dim);
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_gcsl* g = new ilsx_gcsl();
  g->ctx = g->own.ctx = ctx; g->cfg = *cfg; g->cat = cat; g->bc = bc; g->a = act_dim;
  if (bc) {
    const size_t B = (size_t)cfg->max_batch;
    int rc = g->own.alloc(&g->X, B * D);
    if (rc == ILSX_OK) rc = g->own.alloc(&g->act, B * act_dim);
    if (rc == ILSX_OK) rc = g->own.alloc(&g->zeros, B * act_dim);
    if (rc != ILSX_OK) { ilsx_gcsl_destroy(g); return rc; }
  }
  *out = g;
  return ILSX_OK;
}

static int gcsl_step(ilsx_gcsl* g, int B, float* stats2) {
  if (g->cat) return ilsx_bncat_train_step(g->cat, B, g->cfg.policy_lr, stats2);
  float st = 0.0f;
  ILSX_TRY(ilsx_bc_train_step(g->bc, g->X, g->act, B, g->zeros, stats2 ? &st : nullptr));
  if (stats2) { stats2[0] = st; stats2[1] = 0.0f; }
  return ILSX_OK;
}

// GCSL.train_step on a batch drawn from the ring: idx / idx_relabel are device int64 [B] (the host-drawn indices of
// HindsightHorizonReplayBuffer); the gather writes straight into the trainer's input.  stats2_host (nullable, syncs): CLASS {CE Loss,
// Accuracy}, MSE {MSE, 0}.
extern "C" int ilsx_gcsl_train_from_replay(ilsx_gcsl* g, ilsx_replay* rb, const int64_t* idx, const int64_t* idx_relabel, int B, float* stats2_host) {
  if (!g || !rb) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_train_from_replay: NULL argument");
  if (B < 2 || B > g->cfg.max_batch) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_train_from_replay: B=%d not in 2..%d", B, g->cfg.max_batch);
  const ilsx_gcsl_cfg& c = g->cfg;
  if (g->cat) {
    ILSX_TRY(ilsx_her_horizon_gather(rb, idx, idx_relabel, B, c.d_obs, c.d_goal, c.horizon, 1, g->cat->W.X, nullptr, (int32_t*)g->cat->W.label));
  } else {
    if (rb->a != g->a) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_train_from_replay: ring act_dim %d != %d", rb->a, g->a);
    ILSX_TRY(ilsx_her_horizon_gather(rb, idx, idx_relabel, B, c.d_obs, c.d_goal, c.horizon, 0, g->X, g->act, nullptr));
  }
  return gcsl_step(g, B, stats2_host);
}
// the same on an explicit batch: X [B][d_obs + d_goal + horizon] and the targets (CLASS: int32 [B], MSE: float [B][act_dim]), device pointers
extern "C" int ilsx_gcsl_train_step(ilsx_gcsl* g, const float* X, const void* target, int B, float* stats2_host) {
  if (!g || !X || !target) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_train_step: NULL argument");
  if (B < 2 || B > g->cfg.max_batch) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_gcsl_train_step: B=%d not in 2..%d", B, g->cfg.max_batch);
  const ilsx_gcsl_cfg& c = g->cfg;
  const size_t D = (size_t)(c.d_obs + c.d_goal + c.horizon);
  HIPCHK(hipSetDevice(g->ctx->device));
  hipStream_t st = g->ctx->stream;
  if (g->cat) {
    HIPCHK(hipMemcpyAsync(g->cat->W.X, X, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(g->cat->W.label, target, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  } else {
    HIPCHK(hipMemcpyAsync(g->X, X, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(g->act, target, (size_t)B * g->a * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return gcsl_step(g, B, stats2_host);
}
