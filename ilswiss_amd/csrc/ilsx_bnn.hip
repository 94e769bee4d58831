// ilsx_bnn.hip — host side of the MBPO ensemble (bnn.h): layout, init, parameter / optimiser / normaliser I/O, the launches of
// one train batch, holdout MSE, predict, normaliser statistics and the fused model-rollout step.
#include <algorithm>
#include <cmath>
#include <random>

#include "bnn.h"
#include "host_common.h"

struct ilsx_bnn {
  ilsx_ctx* ctx = nullptr;
  DevOwner own;   // the slab, `part` and the rollout buffers s_*
  ilsx_bnn_cfg cfg{};
  int nl = 0, HP = 0, NOP = 0, D = 0, KP0 = 0;
  int in_l[ILSX_BNN_MAX_LAYERS] = {0}, out_l[ILSX_BNN_MAX_LAYERS] = {0};
  int kp[ILSX_BNN_MAX_LAYERS] = {0}, np[ILSX_BNN_MAX_LAYERS] = {0};
  int off_w[ILSX_BNN_MAX_LAYERS] = {0}, off_wt[ILSX_BNN_MAX_LAYERS] = {0}, off_b[ILSX_BNN_MAX_LAYERS] = {0};
  long long mstride = 0;
  size_t n_flat = 0;
  float *P = nullptr, *M = nullptr, *V = nullptr;   // [E][mstride]
  float *mean = nullptr, *std = nullptr;            // [KP0]
  float h_mean[256], h_std[256];
  int64_t t = 0;                                    // Adam step count (shared by every parameter group)
  uint64_t rng_step = 0;                            // Philox step of the model-rollout draws
  uint32_t rng_stream = 0;
  // train scratch (max_batch rows)
  long long ldr = 0;
  float *xs = nullptr, *pre = nullptr, *hs = nullptr, *dpre = nullptr, *dhead = nullptr, *loss = nullptr;
  // row-count dependent scratch (grown on demand)
  float* part = nullptr; size_t part_n = 0;
  int step_cap = 0;
  float *s_mean = nullptr, *s_lv = nullptr, *s_x = nullptr, *s_act = nullptr, *s_rew = nullptr, *s_nobs = nullptr;
  uint8_t* s_done = nullptr; int32_t *s_midx = nullptr, *s_elites = nullptr; int* s_count = nullptr;
};

static int r16(int x) { return (x + 15) / 16 * 16; }

// hidden widths above 256 run k_bnn_wide: a wave owns ILSX_BNN_SPW_WIDE slices of a hidden layer
static bool bnn_wide(const ilsx_bnn* b) { return b->HP > 256; }

static int bnn_threads(const ilsx_bnn* b) {
  const int hs = b->HP / 16, hw = bnn_wide(b) ? (hs + ILSX_BNN_SPW_WIDE - 1) / ILSX_BNN_SPW_WIDE : hs;
  return 64 * std::max(std::max(hw, b->KP0 / 16), b->NOP / 16);
}

template <int MODE>
static void bnn_launch_fwd(const ilsx_bnn* b, int ntiles, const BnnFwdArgs& A) {
  const dim3 grid(ntiles, b->cfg.ensemble), block(bnn_threads(b));
  if (bnn_wide(b)) hipLaunchKernelGGL(k_bnn_wide<MODE>, grid, block, 0, b->ctx->stream, A);
  else hipLaunchKernelGGL(k_bnn_fwd<MODE>, grid, block, 0, b->ctx->stream, A);
}

static BnnNet bnn_net(const ilsx_bnn* b) {
  BnnNet N{};
  N.P = b->P; N.mstride = b->mstride;
  for (int l = 0; l < b->nl; ++l) {
    N.off_w[l] = b->off_w[l]; N.off_wt[l] = b->off_wt[l]; N.off_b[l] = b->off_b[l]; N.kp[l] = b->kp[l]; N.np[l] = b->np[l];
  }
  N.nl = b->nl; N.HP = b->HP; N.NOP = b->NOP; N.D = b->D; N.in_dim = b->cfg.in_dim;
  N.mean = b->mean; N.std = b->std;
  return N;
}

static int bnn_grow(ilsx_bnn* b, float** p, size_t* have, size_t need) {
  if (need <= *have) return ILSX_OK;
  ILSX_TRY(b->own.free(*p));
  *p = nullptr;
  ILSX_TRY(b->own.alloc(p, need));
  *have = need;
  return ILSX_OK;
}

extern "C" int ilsx_bnn_create(ilsx_ctx* ctx, const ilsx_bnn_cfg* cfg, ilsx_bnn** out) {
  if (!ctx || !cfg || !out) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_create: NULL argument");
  const ilsx_bnn_cfg& c = *cfg;
  if (c.ensemble < 1 || c.in_dim < 1 || c.out_dim < 2 || c.hidden < 1 || c.max_batch < 1)
    ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_create: bad shape (E=%d in=%d out=%d H=%d max_batch=%d)", c.ensemble, c.in_dim, c.out_dim, c.hidden, c.max_batch);
  if (c.n_hidden < 1 || c.n_hidden > ILSX_BNN_MAX_HID) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_create: n_hidden=%d outside 1..%d", c.n_hidden, ILSX_BNN_MAX_HID);
  if (r16(c.hidden) > ILSX_BNN_MAX_WIDE || r16(c.in_dim) > 256 || r16(2 * c.out_dim) > 256)
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_bnn_create: hidden width above %d or input / head width above 256 (hidden %d, in %d, head %d) is not supported",
              ILSX_BNN_MAX_WIDE, c.hidden, c.in_dim, 2 * c.out_dim);
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_bnn* b = new ilsx_bnn();
  b->ctx = b->own.ctx = ctx; b->cfg = c;
  b->nl = c.n_hidden + 1; b->HP = r16(c.hidden); b->D = c.out_dim; b->NOP = r16(2 * c.out_dim); b->KP0 = r16(c.in_dim);
  long long off = 0;
  for (int l = 0; l < b->nl; ++l) {
    b->in_l[l] = l == 0 ? c.in_dim : c.hidden;
    b->out_l[l] = l == b->nl - 1 ? 2 * c.out_dim : c.hidden;
    b->kp[l] = l == 0 ? b->KP0 : b->HP;
    b->np[l] = l == b->nl - 1 ? b->NOP : b->HP;
    b->off_w[l] = (int)off; off += (long long)b->kp[l] * b->np[l];
    b->off_wt[l] = (int)off; off += (long long)b->kp[l] * b->np[l];
    b->off_b[l] = (int)off; off += b->np[l];
    b->n_flat += (size_t)c.ensemble * ((size_t)b->in_l[l] * b->out_l[l] + b->out_l[l]);
  }
  b->mstride = (off + 63) / 64 * 64;
  const size_t E = c.ensemble, tot = E * (size_t)b->mstride;
  b->ldr = r16(c.max_batch);
  int rc = ILSX_OK;
  Slab s;
  s.add(&b->P, tot); s.add(&b->M, tot); s.add(&b->V, tot);
  s.add(&b->mean, b->KP0); s.add(&b->std, b->KP0);
  s.add(&b->xs, E * b->ldr * b->KP0);
  s.add(&b->pre, (size_t)c.n_hidden * E * b->ldr * b->HP);
  s.add(&b->hs, (size_t)c.n_hidden * E * b->ldr * b->HP);
  s.add(&b->dpre, (size_t)c.n_hidden * E * b->ldr * b->HP);
  s.add(&b->dhead, E * b->ldr * b->NOP);
  s.add(&b->loss, E);
  void* base = nullptr;
  rc = b->own.commit(s, &base);
  if (rc != ILSX_OK) { ilsx_bnn_destroy(b); return rc; }
  for (int k = 0; k < 256; ++k) { b->h_mean[k] = 0.f; b->h_std[k] = 1.0f + 1e-8f; }   // FixedNormalizer(mean=0, std=1): std + eps
  rc = ilsx_bnn_set_normalizer(b, b->h_mean, b->h_std);
  if (rc != ILSX_OK) { ilsx_bnn_destroy(b); return rc; }
  b->rng_stream = ctx->next_rng_stream++;
  *out = b;
  return ILSX_OK;
}

extern "C" int ilsx_bnn_destroy(ilsx_bnn* b) {
  if (!b) return ILSX_OK;
  hipSetDevice(b->ctx->device);
  hipStreamSynchronize(b->ctx->stream);
  b->own.release();
  delete b;
  return ILSX_OK;
}

extern "C" int ilsx_bnn_num_params(const ilsx_bnn* b, size_t* n) {
  if (!b || !n) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_num_params: NULL argument");
  *n = b->n_flat;
  return ILSX_OK;
}

// flat (named_parameters order: per layer weight[E,in,out] | bias[E,1,out]) <-> internal blocks (W, Wt and b per member)
static void bnn_flat_to_internal(const ilsx_bnn* b, const float* flat, float* in, bool transposed_too) {
  const int E = b->cfg.ensemble;
  size_t f = 0;
  for (int l = 0; l < b->nl; ++l) {
    const int I = b->in_l[l], O = b->out_l[l];
    for (int e = 0; e < E; ++e) {
      float* m = in + (size_t)e * b->mstride;
      for (int i = 0; i < I; ++i)
        for (int j = 0; j < O; ++j) {
          const float v = flat[f + ((size_t)e * I + i) * O + j];
          m[b->off_w[l] + (size_t)i * b->np[l] + j] = v;
          if (transposed_too) m[b->off_wt[l] + (size_t)j * b->kp[l] + i] = v;
        }
    }
    f += (size_t)E * I * O;
    for (int e = 0; e < E; ++e)
      for (int j = 0; j < O; ++j) in[(size_t)e * b->mstride + b->off_b[l] + j] = flat[f + (size_t)e * O + j];
    f += (size_t)E * O;
  }
}

static void bnn_internal_to_flat(const ilsx_bnn* b, const float* in, float* flat) {
  const int E = b->cfg.ensemble;
  size_t f = 0;
  for (int l = 0; l < b->nl; ++l) {
    const int I = b->in_l[l], O = b->out_l[l];
    for (int e = 0; e < E; ++e)
      for (int i = 0; i < I; ++i)
        for (int j = 0; j < O; ++j) flat[f + ((size_t)e * I + i) * O + j] = in[(size_t)e * b->mstride + b->off_w[l] + (size_t)i * b->np[l] + j];
    f += (size_t)E * I * O;
    for (int e = 0; e < E; ++e)
      for (int j = 0; j < O; ++j) flat[f + (size_t)e * O + j] = in[(size_t)e * b->mstride + b->off_b[l] + j];
    f += (size_t)E * O;
  }
}

static int bnn_upload(ilsx_bnn* b, float* dst, const float* flat, bool transposed_too) {
  std::vector<float> in((size_t)b->cfg.ensemble * b->mstride, 0.f);
  bnn_flat_to_internal(b, flat, in.data(), transposed_too);
  HIPCHK(hipMemcpyAsync(dst, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}

static int bnn_download(const ilsx_bnn* b, const float* src, float* flat) {
  std::vector<float> in((size_t)b->cfg.ensemble * b->mstride);
  HIPCHK(hipMemcpyAsync(in.data(), src, in.size() * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  bnn_internal_to_flat(b, in.data(), flat);
  return ILSX_OK;
}

extern "C" int ilsx_bnn_set_params(ilsx_bnn* b, const float* src, size_t n) {
  if (!b || !src) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_params: NULL argument");
  if (n != b->n_flat) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_params: n=%zu, the ensemble has %zu", n, b->n_flat);
  HIPCHK(hipSetDevice(b->ctx->device));
  return bnn_upload(b, b->P, src, true);
}

extern "C" int ilsx_bnn_get_params(const ilsx_bnn* b, float* dst, size_t n) {
  if (!b || !dst) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_get_params: NULL argument");
  if (n != b->n_flat) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_get_params: n=%zu, the ensemble has %zu", n, b->n_flat);
  HIPCHK(hipSetDevice(b->ctx->device));
  return bnn_download(b, b->P, dst);
}

extern "C" int ilsx_bnn_init(ilsx_bnn* b, uint64_t seed) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_init: NULL ensemble");
  // networks.py:200-229 + pytorch_util.py:20-29: fanin_init on an [E, in, out] weight takes fan-in = in * out; hidden biases 0.1;
  // the last layer's weight and bias U(+-init_w)
  std::mt19937_64 gen(seed);
  std::vector<float> flat(b->n_flat);
  const int E = b->cfg.ensemble;
  size_t f = 0;
  for (int l = 0; l < b->nl; ++l) {
    const size_t I = b->in_l[l], O = b->out_l[l];
    const bool last = l == b->nl - 1;
    const float bound = last ? b->cfg.init_w : (float)(1.0 / std::sqrt((double)(I * O)));
    std::uniform_real_distribution<float> u(-bound, bound);
    for (size_t i = 0; i < E * I * O; ++i) flat[f + i] = u(gen);
    f += E * I * O;
    for (size_t i = 0; i < E * O; ++i) flat[f + i] = last ? u(gen) : 0.1f;
    f += E * O;
  }
  return ilsx_bnn_set_params(b, flat.data(), flat.size());
}

extern "C" int ilsx_bnn_get_opt(const ilsx_bnn* b, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_get_opt: NULL ensemble");
  if ((m_host || v_host) && n != b->n_flat) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_get_opt: n=%zu, the ensemble has %zu", n, b->n_flat);
  HIPCHK(hipSetDevice(b->ctx->device));
  if (m_host) ILSX_TRY(bnn_download(b, b->M, m_host));
  if (v_host) ILSX_TRY(bnn_download(b, b->V, v_host));
  if (meta) { meta->t = b->t; meta->rng_step = b->rng_step; meta->n_train_steps = b->t; }
  return ILSX_OK;
}

extern "C" int ilsx_bnn_set_opt(ilsx_bnn* b, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta) {
  if (!b) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_opt: NULL ensemble");
  if ((m_host || v_host) && n != b->n_flat) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_opt: n=%zu, the ensemble has %zu", n, b->n_flat);
  HIPCHK(hipSetDevice(b->ctx->device));
  if (m_host) ILSX_TRY(bnn_upload(b, b->M, m_host, false));
  if (v_host) ILSX_TRY(bnn_upload(b, b->V, v_host, false));
  if (meta) { b->t = meta->t; b->rng_step = meta->rng_step; }
  return ILSX_OK;
}

extern "C" int ilsx_bnn_set_normalizer(ilsx_bnn* b, const float* mean_host, const float* std_host) {
  if (!b || !mean_host || !std_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_normalizer: NULL argument");
  const int K = b->cfg.in_dim;
  for (int k = 0; k < K; ++k) {
    if (!(std_host[k] != 0.f)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_set_normalizer: std[%d] is zero", k);
    b->h_mean[k] = mean_host[k]; b->h_std[k] = std_host[k];
  }
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipMemcpyAsync(b->mean, b->h_mean, K * sizeof(float), hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipMemcpyAsync(b->std, b->h_std, K * sizeof(float), hipMemcpyHostToDevice, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}

extern "C" int ilsx_bnn_get_normalizer(const ilsx_bnn* b, float* mean_host, float* std_host) {
  if (!b || !mean_host || !std_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_get_normalizer: NULL argument");
  HIPCHK(hipSetDevice(b->ctx->device));
  HIPCHK(hipMemcpyAsync(mean_host, b->mean, b->cfg.in_dim * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipMemcpyAsync(std_host, b->std, b->cfg.in_dim * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}

static int bnn_check_ring(const ilsx_bnn* b, const ilsx_replay* rb, const char* who) {
  if (!rb) ILSX_FAIL(ILSX_ERR_ARG, "%s: NULL replay ring", who);
  if (rb->ctx->device != b->ctx->device) ILSX_FAIL(ILSX_ERR_ARG, "%s: the ring lives on another device", who);
  if (rb->o + rb->a != b->cfg.in_dim || rb->o + 1 != b->cfg.out_dim)
    ILSX_FAIL(ILSX_ERR_ARG, "%s: ring rows (obs %d, act %d) do not match the ensemble (in %d, out %d)", who, rb->o, rb->a, b->cfg.in_dim,
              b->cfg.out_dim);
  return ILSX_OK;
}

extern "C" int ilsx_bnn_fit_stats(ilsx_bnn* b, ilsx_replay* rb, const int32_t* idx, int n) {
  if (!b || !idx || n < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_fit_stats: bad argument");
  ILSX_TRY(bnn_check_ring(b, rb, "ilsx_bnn_fit_stats"));
  HIPCHK(hipSetDevice(b->ctx->device));
  hipLaunchKernelGGL(k_bnn_stats, dim3(b->cfg.in_dim), dim3(256), 0, b->ctx->stream, rb->data, (long long)rb->cap, rb->rec, idx, n, b->mean,
                     b->std);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(b->h_mean, b->mean, b->cfg.in_dim * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipMemcpyAsync(b->h_std, b->std, b->cfg.in_dim * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return ILSX_OK;
}

static BnnFwdArgs bnn_fwd_args(const ilsx_bnn* b, const ilsx_replay* rb, const int32_t* idx, int64_t idx_ms, int rows) {
  BnnFwdArgs A{};
  A.net = bnn_net(b);
  if (rb) { A.ring = rb->data; A.cap = rb->cap; A.rec = rb->rec; A.o = rb->o; A.a = rb->a; }
  A.idx = idx; A.idx_ms = idx_ms;
  A.rows = rows; A.ntiles = (rows + 15) / 16;
  A.reward_scale = b->cfg.reward_scale;
  return A;
}

extern "C" int ilsx_bnn_train_batch(ilsx_bnn* b, ilsx_replay* rb, const int32_t* idx, int64_t idx_member_stride, int B, float* loss_host) {
  if (!b || !idx || B < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_train_batch: bad argument");
  if (B > b->cfg.max_batch) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_train_batch: B=%d > max_batch=%d", B, b->cfg.max_batch);
  ILSX_TRY(bnn_check_ring(b, rb, "ilsx_bnn_train_batch"));
  ilsx_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int E = b->cfg.ensemble;
  const int nt = (B + 15) / 16;
  ILSX_TRY(bnn_grow(b, &b->part, &b->part_n, (size_t)E * nt * 2));
  BnnFwdArgs A = bnn_fwd_args(b, rb, idx, idx_member_stride, B);
  A.xs = b->xs; A.pre = b->pre; A.hs = b->hs; A.dhead = b->dhead; A.dpre = b->dpre; A.ldr = b->ldr;
  A.gscale = (float)(1.0 / ((double)E * B * b->D));
  A.partial = b->part; A.add_var = 1;
  bnn_launch_fwd<BNN_TRAIN>(b, nt, A);
  HIPCHK(hipGetLastError());
  // torch Adam: t += 1; step_size = lr / (1 - b1^t); denom = sqrt(v) / sqrt(1 - b2^t) + eps (bnn_trainer.py:81-87,150-154)
  b->t += 1;
  const double b1 = 0.9, b2 = 0.999;
  BnnDwArgs W{};
  W.P = b->P; W.M = b->M; W.V = b->V; W.mstride = b->mstride;
  int ntask = 0;
  for (int l = 0; l < b->nl; ++l) {
    W.off_w[l] = b->off_w[l]; W.off_wt[l] = b->off_wt[l]; W.off_b[l] = b->off_b[l];
    W.kp[l] = b->kp[l]; W.np[l] = b->np[l]; W.in_l[l] = b->in_l[l]; W.out_l[l] = b->out_l[l];
    W.wd[l] = b->cfg.weight_decay[l];
    W.task0[l] = ntask;
    ntask += (b->kp[l] / 16) * (b->np[l] / 16) + b->np[l] / 16;
  }
  W.task0[b->nl] = ntask;
  W.nl = b->nl; W.HP = b->HP; W.NOP = b->NOP; W.rows = B; W.E = E;
  W.xs = b->xs; W.hs = b->hs; W.dpre = b->dpre; W.dhead = b->dhead; W.ldr = b->ldr;
  W.lr_bc1 = (float)((double)b->cfg.lr / (1.0 - std::pow(b1, (double)b->t)));
  W.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)b->t));
  W.b1 = (float)b1; W.b2 = (float)b2; W.eps = 1e-8f;
  hipLaunchKernelGGL(k_bnn_dw_adam, dim3((ntask + 3) / 4, E), dim3(256), 0, c->stream, W);
  HIPCHK(hipGetLastError());
  if (loss_host) {
    hipLaunchKernelGGL(k_bnn_reduce, dim3((E + 63) / 64), dim3(64), 0, c->stream, b->part, E, nt, (float)((double)B * b->D), b->loss);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(loss_host, b->loss, E * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return ILSX_OK;
}

extern "C" int ilsx_bnn_mse(ilsx_bnn* b, ilsx_replay* rb, const int32_t* idx, int64_t idx_member_stride, int n, int add_var, float* out_host) {
  if (!b || !idx || n < 1 || !out_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_mse: bad argument");
  ILSX_TRY(bnn_check_ring(b, rb, "ilsx_bnn_mse"));
  ilsx_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int E = b->cfg.ensemble, nt = (n + 15) / 16;
  ILSX_TRY(bnn_grow(b, &b->part, &b->part_n, (size_t)E * nt * 2));
  BnnFwdArgs A = bnn_fwd_args(b, rb, idx, idx_member_stride, n);
  A.partial = b->part; A.add_var = add_var ? 1 : 0;
  bnn_launch_fwd<BNN_MSE>(b, nt, A);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_bnn_reduce, dim3((E + 63) / 64), dim3(64), 0, c->stream, b->part, E, nt, (float)((double)n * b->D), b->loss);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_host, b->loss, E * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ILSX_OK;
}

static int bnn_forward_rows(ilsx_bnn* b, const float* x, int n, float* mean, float* lv, int out_var) {
  const int nt = (n + 15) / 16;
  BnnFwdArgs A = bnn_fwd_args(b, nullptr, nullptr, 0, n);
  A.x = x; A.out_mean = mean; A.out_lv = lv; A.out_var = out_var;
  bnn_launch_fwd<BNN_PREDICT>(b, nt, A);
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

extern "C" int ilsx_bnn_predict(ilsx_bnn* b, const float* x, int n, float* mean, float* var, int ret_log_var) {
  if (!b || !x || !mean || !var || n < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_predict: bad argument");
  if (n == 0) return ILSX_OK;
  HIPCHK(hipSetDevice(b->ctx->device));
  return bnn_forward_rows(b, x, n, mean, var, ret_log_var ? 0 : 1);
}

static int bnn_step_scratch(ilsx_bnn* b, int n, int o, int a) {
  if (n <= b->step_cap) return ILSX_OK;
  DevOwner& own = b->own;
  for (void** p : {(void**)&b->s_mean, (void**)&b->s_lv, (void**)&b->s_x, (void**)&b->s_act, (void**)&b->s_rew, (void**)&b->s_nobs, (void**)&b->s_done,
                   (void**)&b->s_midx}) {
    ILSX_TRY(own.free(*p));
    *p = nullptr;
  }
  b->step_cap = 0;
  const size_t E = b->cfg.ensemble, D = b->D;
  ILSX_TRY(own.alloc(&b->s_mean, E * n * D, false));
  ILSX_TRY(own.alloc(&b->s_lv, E * n * D, false));
  ILSX_TRY(own.alloc(&b->s_x, (size_t)n * b->cfg.in_dim, false));
  ILSX_TRY(own.alloc(&b->s_act, (size_t)n * a, false));
  ILSX_TRY(own.alloc(&b->s_rew, (size_t)n, false));
  ILSX_TRY(own.alloc(&b->s_nobs, (size_t)n * o, false));
  ILSX_TRY(own.alloc(&b->s_done, (size_t)n, false));
  ILSX_TRY(own.alloc(&b->s_midx, (size_t)n, false));
  if (!b->s_elites) ILSX_TRY(own.alloc(&b->s_elites, 256));
  if (!b->s_count) ILSX_TRY(own.alloc_bytes(&b->s_count, 64));
  b->step_cap = n;
  return ILSX_OK;
}

extern "C" int ilsx_mbpo_model_step(ilsx_bnn* b, ilsx_net* pi, ilsx_replay* model_rb, int term_kind, const float* obs, const float* act,
                                    int n, const int32_t* elites_host, int n_elites, int deterministic, const float* eps,
                                    const int32_t* model_idx, float* act_out, int32_t* model_idx_out, float* obs_next, int* n_survivors) {
  if (!b || !obs || !obs_next || !n_survivors || n < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_mbpo_model_step: bad argument");
  if (!act && !pi) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_mbpo_model_step: neither a policy nor actions");
  if (!model_idx && (!elites_host || n_elites < 1 || n_elites > 256)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_mbpo_model_step: no elite set");
  if (!model_idx)
    for (int q = 0; q < n_elites; ++q)
      if (elites_host[q] < 0 || elites_host[q] >= b->cfg.ensemble) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_mbpo_model_step: elite %d out of range", elites_host[q]);
  const int o = b->D - 1, a = b->cfg.in_dim - o;
  if (model_rb && (model_rb->o != o || model_rb->a != a)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_mbpo_model_step: model ring rows do not match");
  *n_survivors = 0;
  if (n == 0) return ILSX_OK;
  ilsx_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->device));
  ILSX_TRY(bnn_step_scratch(b, n, o, a));
  // actions: the SAC policy's stochastic get_actions (mbpo.py:249), or given
  const float* d_act = act;
  if (!d_act) {
    ILSX_TRY(ilsx_policy_act(pi, obs, n, 0, nullptr, b->s_act, nullptr));
    d_act = b->s_act;
  }
  // ensemble inputs [obs | act] (fake_env.py:40): the forward reads x[n][in_dim]
  float* x = b->s_x;
  HIPCHK(hipMemcpy2DAsync(x, (size_t)b->cfg.in_dim * 4, obs, (size_t)o * 4, (size_t)o * 4, n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpy2DAsync(x + o, (size_t)b->cfg.in_dim * 4, d_act, (size_t)a * 4, (size_t)a * 4, n, hipMemcpyDeviceToDevice, c->stream));
  ILSX_TRY(bnn_forward_rows(b, x, n, b->s_mean, b->s_lv, 0));
  if (!model_idx) HIPCHK(hipMemcpyAsync(b->s_elites, elites_host, n_elites * 4, hipMemcpyHostToDevice, c->stream));
  const uint64_t step = b->rng_step++;
  hipLaunchKernelGGL(k_mbpo_sample, dim3((n + 255) / 256), dim3(256), 0, c->stream, b->s_mean, b->s_lv, n, b->D, obs, b->s_elites, n_elites,
                     model_idx, deterministic, eps, c->seed, (unsigned long long)step, b->rng_stream, b->s_rew, b->s_nobs, b->s_midx);
  HIPCHK(hipGetLastError());
  ILSX_TRY(ilsx_is_terminal(c, term_kind, b->s_nobs, n, o, b->s_done));
  if (act_out && act_out != d_act) HIPCHK(hipMemcpyAsync(act_out, d_act, (size_t)n * a * 4, hipMemcpyDeviceToDevice, c->stream));
  if (model_idx_out) HIPCHK(hipMemcpyAsync(model_idx_out, b->s_midx, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  if (model_rb) {   // add_path: the step's rows in order, then terminate_episode (mbpo.py:251-258, simple_replay_buffer.py:134-160)
    std::vector<uint8_t> ep_end(n, 0);
    ep_end[n - 1] = 1;
    ILSX_TRY(ilsx_replay_add(model_rb, obs, d_act, b->s_rew, b->s_done, b->s_nobs, n, ep_end.data(), 1));
  }
  hipLaunchKernelGGL(k_mbpo_compact, dim3(1), dim3(1024), 0, c->stream, b->s_nobs, b->s_done, n, o, obs_next, b->s_count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(n_survivors, b->s_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return ILSX_OK;
}

extern "C" int ilsx_bnn_debug_padding(const ilsx_bnn* b, double* max_abs) {
  if (!b || !max_abs) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_bnn_debug_padding: NULL argument");
  HIPCHK(hipSetDevice(b->ctx->device));
  const size_t tot = (size_t)b->cfg.ensemble * b->mstride;
  std::vector<float> h(tot);
  double mx = 0.0;
  for (const float* src : {(const float*)b->P, (const float*)b->M, (const float*)b->V}) {
    HIPCHK(hipMemcpyAsync(h.data(), src, tot * sizeof(float), hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    for (int e = 0; e < b->cfg.ensemble; ++e) {
      const float* m = h.data() + (size_t)e * b->mstride;
      for (int l = 0; l < b->nl; ++l) {
        const bool is_p = src == b->P;   // Wt lives in the parameter block only
        for (int k = 0; k < b->kp[l]; ++k)
          for (int j = 0; j < b->np[l]; ++j) {
            if (k < b->in_l[l] && j < b->out_l[l]) continue;
            mx = std::max(mx, (double)std::fabs(m[b->off_w[l] + (size_t)k * b->np[l] + j]));
            if (is_p) mx = std::max(mx, (double)std::fabs(m[b->off_wt[l] + (size_t)j * b->kp[l] + k]));
          }
        for (int j = b->out_l[l]; j < b->np[l]; ++j) mx = std::max(mx, (double)std::fabs(m[b->off_b[l] + j]));
      }
    }
  }
  *max_abs = mx;
  return ILSX_OK;
}
