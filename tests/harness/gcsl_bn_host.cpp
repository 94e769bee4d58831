// TEST HARNESS, not product: compiles ilswiss_amd/csrc/gcsl.h (the horizon gather and the phases of the BatchNorm categorical policy's
// cross-entropy step, over the phases of disc_bn.h) for the HOST, every phase as a serial loop, so that the CPU suite can check them against the
// reference's vectors (tests/golden/g29_gcsl.npz) without a GPU.  Built by tests/test_gcsl_cpu.py into a temp dir; nothing in ilswiss_amd/
// loads it.
#define DBN_HOST_EMU 1
#include <cstring>
#include <vector>
#include "../../ilswiss_amd/csrc/gcsl.h"

struct HostLaunch {
  template <class F> void par(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
  template <class F> void col(int H, F f) { for (int j = 0; j < H; ++j) f(j, 0); }
  void gemm(const DbnGemm& g) { for (int i = 0; i < g.M; ++i) for (int j = 0; j < g.N; ++j) dbn_gemm_elem(g, i, j); }
  void gemm(const DbnGemm& g1, const DbnGemm& g2) { gemm(g1); gemm(g2); }
};

struct HostCat {
  GcslNet N;
  GcslWs W;
  std::vector<std::vector<float>> store;
  std::vector<int> labels;
  int rows, t = 0;
  float* buf(size_t n) { store.emplace_back(n, 0.0f); return store.back().data(); }
};

extern "C" void* gch_create(int D, int H, int nblk, int n, int rows) {
  if (nblk < 1 || nblk > GCSL_MAX_BLK || n < 1 || n > GCSL_MAX_NO) return nullptr;
  HostCat* d = new HostCat();
  GcslNet& N = d->N;
  N.D = D; N.H = H; N.nblk = nblk; N.n = n;
  const int np = N.n_params();
  N.P = d->buf(np); N.G = d->buf(np); N.M = d->buf(np); N.V = d->buf(np);
  N.rmean = d->buf((size_t)nblk * H); N.rvar = d->buf((size_t)nblk * H);
  for (int i = 0; i < nblk * H; ++i) N.rvar[i] = 1.0f;
  d->rows = rows;
  GcslWs& W = d->W;
  W.X = d->buf((size_t)rows * D);
  d->labels.assign(rows, 0);
  W.label = d->labels.data();
  for (int l = 0; l < nblk; ++l) {
    W.ch[l] = d->buf((size_t)rows * H); W.ah[l] = d->buf((size_t)rows * H); W.h[l] = d->buf((size_t)rows * H);
    W.p[l] = d->buf((size_t)rows * H); W.s[l] = d->buf(H);
  }
  W.t0 = d->buf((size_t)rows * H); W.t1 = d->buf((size_t)rows * H);
  W.logit = d->buf((size_t)rows * n); W.dlogit = d->buf((size_t)rows * n);
  W.ce_row = d->buf(rows); W.correct = d->buf(rows);
  W.bstat = d->buf((size_t)nblk * 2 * H);
  return d;
}
extern "C" void gch_destroy(void* h) { delete (HostCat*)h; }
extern "C" int gch_num_params(void* h) { return ((HostCat*)h)->N.n_params(); }
extern "C" void gch_set_params(void* h, const float* flat) { HostCat* d = (HostCat*)h; memcpy(d->N.P, flat, sizeof(float) * d->N.n_params()); }
extern "C" void gch_get(void* h, float* params, float* rmean, float* rvar) {
  HostCat* d = (HostCat*)h;
  const int np = d->N.n_params(), nb = d->N.nblk * d->N.H;
  if (params) memcpy(params, d->N.P, sizeof(float) * np);
  if (rmean) memcpy(rmean, d->N.rmean, sizeof(float) * nb);
  if (rvar) memcpy(rvar, d->N.rvar, sizeof(float) * nb);
}
// one CLASS-mode step on X [B][D] and integer labels; stats2 = {CE, accuracy}
extern "C" int gch_train_step(void* h, const float* X, const int* labels, int B, float lr, float* stats2) {
  HostCat* d = (HostCat*)h;
  if (B < 2 || B > d->rows) return -1;
  memcpy(d->W.X, X, sizeof(float) * (size_t)B * d->N.D);
  memcpy(d->W.label, labels, sizeof(int) * B);
  HostLaunch L;
  gcsl_cat_step(L, d->N, d->W, B, stats2, lr, ++d->t);
  return 0;
}
extern "C" int gch_eval(void* h, const float* x, int rows, float* probs, float* amax) {
  HostCat* d = (HostCat*)h;
  if (rows < 1 || rows > d->rows) return -1;
  HostLaunch L;
  gcsl_eval(L, d->N, d->W, x, rows, probs, amax);
  return 0;
}
// the horizon gather over a host copy of the ring's records
extern "C" void gch_gather(const float* data, int rec, const long long* idx, const long long* idx_rel, int B, int d_obs, int dg, int a, int T,
                           int mode, float* X, float* act, int* label) {
  HostLaunch L;
  L.par(B * (d_obs + dg + T), [=](int e) { gcsl_gather_elem(e, data, rec, idx, idx_rel, d_obs, dg, a, T, mode, X, act, label); });
}
