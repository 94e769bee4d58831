// bnn.h — gfx950 device code of the probabilistic network ensemble of MBPO (rlkit/torch/common/networks.py:149-279 BNN,
// rlkit/torch/algorithms/mbpo/bnn_trainer.py BNNTrainer, fake_env.py FakeEnv).  A kernel family of its own next to kernels.h:
// four hidden layers, SiLU, H = 200 (not a multiple of 16) and a head with a soft-clamped log-variance do not fit the SAC kernels'
// NetView / FwdTask descriptors, whose constant-memory blocks are tuned.
//
// Layout (per member, one contiguous block of `mstride` floats; members back to back):
//   layer l: W_l [KP_l][NP_l] row-major (k = input unit, n = output unit, the reference's weight[e] of shape [in, out]),
//            Wt_l [NP_l][KP_l] (the same matrix transposed, kept in step by the optimiser: the backward reads it n-contiguous),
//            b_l [NP_l].
//   KP_0 = in_dim rounded up to 16, every hidden width H rounded up to 16 (200 -> 208), NP of the head = 2*D rounded up to 16.
//   Padded rows / columns / biases are zero and stay zero: SiLU(0) = 0, so a padded unit's activation, its gradient, its weight
//   decay and its Adam moments are all zero (the optimiser also masks them, so "stay zero" holds bit for bit).
//
// One workgroup = 16 batch rows of ONE member (grid = row tiles x members: one launch covers the whole ensemble), HP/16 waves (13 for
// H = 200); wave w owns output columns [16w, 16w+16) of every layer.  Each layer is a chain of exact-fp32 MFMAs
// (v_mfma_f32_16x16x4_f32); the layer's input rows sit in LDS, the member's weights stream from L2.  Fragment maps (MI355X guide 3):
//   lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; lane l, register v receives D[row = 4*(l>>4) + v][col = l&15].
// Widths above 256 (up to 400, the reference's Humanoid spec) take the wide kernel k_bnn_wide further down: HP/16 would be up to 25 waves,
// so a wave owns TWO 16-column slices of a layer, w and w + nwaves (13 waves for H = 400; the last wave has one slice when the slice count
// is odd), two accumulators fed by one LDS read of the input fragment, and the two LDS tiles get a 404-float row stride (51.7 KB).  Same
// math, layout, fragment maps and MFMA chain per column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

#define ILSX_BNN_MAX_LAYERS 9       // hidden layers + head
#define ILSX_BNN_LDA 260            // LDS row stride of an activation tile (widths <= 256, +4 against bank conflicts)
#define ILSX_BNN_MAX_WAVES 16
#define ILSX_BNN_MAX_WIDE 400       // widest hidden layer (k_bnn_wide); in_dim and the head stay <= 256
#define ILSX_BNN_LDA_WIDE 404       // its row stride: 404 = 20 mod 64, so the 16 rows x 4 k of an A fragment fall in 64 distinct banks
#define ILSX_BNN_SPW_WIDE 2         // 16-column slices per wave of k_bnn_wide

enum { BNN_PREDICT = 0, BNN_TRAIN = 1, BNN_MSE = 2 };

struct BnnNet {
  const float* P;           // parameters, [E][mstride]
  long long mstride;
  int off_w[ILSX_BNN_MAX_LAYERS], off_wt[ILSX_BNN_MAX_LAYERS], off_b[ILSX_BNN_MAX_LAYERS];
  int kp[ILSX_BNN_MAX_LAYERS], np[ILSX_BNN_MAX_LAYERS];
  int nl, HP, NOP, D, in_dim;
  const float* mean;        // normaliser [in_dim]
  const float* std;         // (FixedNormalizer's std, its 1e-8 included)
};

struct BnnFwdArgs {
  BnnNet net;
  // rows: from replay records (ring != nullptr; slot = idx[e*idx_ms + row]) or from x[rows][in_dim]
  const float* ring; long long cap; int rec, o, a;
  const int32_t* idx; long long idx_ms;
  const float* x;
  int rows, ntiles;
  float reward_scale;
  // BNN_PREDICT
  float* out_mean; float* out_lv; int out_var;
  // BNN_TRAIN: saved activations ([e][ldr][.]) and the head gradient scale 1 / (E * rows * D)
  float* xs; float* pre; float* hs; float* dhead; float* dpre; long long ldr; float gscale;
  // BNN_TRAIN / BNN_MSE: per-(member, tile) partial sums [E][ntiles][2]
  float* partial; int add_var;
};

__device__ __forceinline__ float bnn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float bnn_silu(float x) { return x / (1.0f + expf(-x)); }   // torch's silu: x * sigmoid(x)
__device__ __forceinline__ float bnn_softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }   // beta 1, threshold 20

// Wave-level sum in a fixed lane order (deterministic run to run).
__device__ __forceinline__ float bnn_wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// One layer of one 16-row tile: out[16][NP] = in[16][KP] @ W (+ epilogue by the caller).  Returns the wave's accumulator.
__device__ __forceinline__ f32x4 bnn_tile_mm(const float (*in)[ILSX_BNN_LDA], const float* __restrict__ W, int kp, int ldw, int col0,
                                             int lane) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int i = lane & 15, kk = lane >> 4;
  const float* wp = W + (size_t)kk * ldw + col0 + i;
  for (int k0 = 0; k0 < kp; k0 += 4) {
    const float av = in[i][k0 + kk];
    const float bv = wp[(size_t)k0 * ldw];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
  return acc;
}

// Forward of the whole ensemble (and, for BNN_TRAIN, the loss gradient and the backward chain down to the first layer's
// pre-activation gradient).  grid (ntiles, E), block 64 * max(HP, KP_0, NOP) / 16.
// KEEP IN STEP with k_bnn_wide below: input staging, head split, loss gradient and partial sums are the same text in both kernels.
template <int MODE>
__global__ __launch_bounds__(1024) void k_bnn_fwd(const BnnFwdArgs A) {
  __shared__ float sbuf[2][16][ILSX_BNN_LDA];
  __shared__ float sred[ILSX_BNN_MAX_WAVES][2];
  const BnnNet& N = A.net;
  const int tile = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, w = tid >> 6;
  const int row0 = tile * 16;
  const float* Pm = N.P + (size_t)e * N.mstride;
  const int kp0 = N.kp[0], in_dim = N.in_dim, D = N.D;

  // ---- input tile, normalised on the load: (x - mean) / std, padded columns / rows zero
  for (int t = tid; t < 16 * kp0; t += nthr) {
    const int r = t / kp0, k = t - r * kp0, gr = row0 + r;
    float v = 0.f;
    if (gr < A.rows && k < in_dim) {
      float raw;
      if (A.ring) {
        long long slot = A.idx[(size_t)e * A.idx_ms + gr];
        if (slot < 0 || slot >= A.cap) slot = 0;
        raw = A.ring[(size_t)slot * A.rec + k];      // record: obs | act | ...
      } else {
        raw = A.x[(size_t)gr * in_dim + k];
      }
      v = (raw - N.mean[k]) / N.std[k];
    }
    sbuf[0][r][k] = v;
    if (MODE == BNN_TRAIN && gr < A.rows) A.xs[((size_t)e * A.ldr + gr) * kp0 + k] = v;
  }
  __syncthreads();

  int cur = 0;
  for (int l = 0; l < N.nl; ++l) {
    const int kp = N.kp[l], np = N.np[l];
    const bool head = (l == N.nl - 1);
    if (w < np / 16) {
      const f32x4 acc = bnn_tile_mm(sbuf[cur], Pm + N.off_w[l], kp, np, 16 * w, lane);
      const int col = 16 * w + (lane & 15);
      const float bias = Pm[N.off_b[l] + col];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 4 * (lane >> 4) + v, gr = row0 + r;
        const float x = acc[v] + bias;
        if (head) {
          sbuf[cur ^ 1][r][col] = x;
        } else {
          const float h = bnn_silu(x);
          sbuf[cur ^ 1][r][col] = h;
          if (MODE == BNN_TRAIN && gr < A.rows) {
            const size_t o_ = (((size_t)l * gridDim.y + e) * A.ldr + gr) * N.HP + col;
            A.pre[o_] = x;
            A.hs[o_] = h;
          }
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- head split (BNN.forward, networks.py:241-263): mean | log-var soft-clamped into [min_lv, max_lv]
  const float max_lv = 0.5f, min_lv = -10.0f;
  float s0 = 0.f, s1 = 0.f;
  for (int t = tid; t < 16 * N.NOP; t += nthr) {
    const int r = t / N.NOP, c = t - r * N.NOP, gr = row0 + r;
    if (c >= D) {
      if (MODE == BNN_TRAIN && c >= 2 * D) sbuf[cur ^ 1][r][c] = 0.f;
      continue;
    }
    const float mu = sbuf[cur][r][c], raw = sbuf[cur][r][D + c];
    const float lv1 = max_lv - bnn_softplus(max_lv - raw);
    const float lv = min_lv + bnn_softplus(lv1 - min_lv);
    if (MODE == BNN_PREDICT) {
      if (gr < A.rows) {
        const size_t o_ = ((size_t)e * A.rows + gr) * D + c;
        A.out_mean[o_] = mu;
        A.out_lv[o_] = A.out_var ? expf(lv) : lv;
      }
      continue;
    }
    float gmu = 0.f, graw = 0.f;
    if (gr < A.rows) {
      const long long slot0 = A.idx[(size_t)e * A.idx_ms + gr];
      const long long slot = (slot0 < 0 || slot0 >= A.cap) ? 0 : slot0;
      const float* R = A.ring + (size_t)slot * A.rec;
      // target [reward_scale * rew | next_obs - obs] (bnn_trainer.py:92-97)
      const float tg = c == 0 ? A.reward_scale * R[A.o + A.a] : R[A.o + A.a + 2 + (c - 1)] - R[c - 1];
      const float diff = mu - tg, sq = diff * diff;
      if (MODE == BNN_MSE && !A.add_var) {
        s0 += sq;
      } else {
        const float inv = expf(-lv);
        s0 += sq * inv;
        s1 += lv;
        if (MODE == BNN_TRAIN) {   // d/dmu, d/dlv of mean_e[ mean((mu - t)^2 e^-lv) + mean(lv) ]; lv = f(raw) through both softplus
          gmu = A.gscale * 2.0f * diff * inv;
          const float glv = A.gscale * (1.0f - sq * inv);
          graw = glv * bnn_sigmoid(lv1 - min_lv) * bnn_sigmoid(max_lv - raw);
        }
      }
    }
    if (MODE == BNN_TRAIN) {
      sbuf[cur ^ 1][r][c] = gmu;
      sbuf[cur ^ 1][r][D + c] = graw;
      if (gr < A.rows) {
        float* dh = A.dhead + ((size_t)e * A.ldr + gr) * N.NOP;
        dh[c] = gmu;
        dh[D + c] = graw;
      }
    }
  }
  if (MODE == BNN_PREDICT) return;
  // per-(member, tile) partial sums, fixed order
  s0 = bnn_wave_sum(s0);
  s1 = bnn_wave_sum(s1);
  if (lane == 0) { sred[w][0] = s0; sred[w][1] = s1; }
  __syncthreads();
  if (tid == 0) {
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < (nthr >> 6); ++q) { a0 += sred[q][0]; a1 += sred[q][1]; }
    A.partial[((size_t)e * A.ntiles + tile) * 2 + 0] = a0;
    A.partial[((size_t)e * A.ntiles + tile) * 2 + 1] = a1;
  }
  if (MODE != BNN_TRAIN) return;
  // padded head columns of the gradient tile (written above for c >= 2D) and columns [D, 2D) were set by the owners of c < D
  cur ^= 1;
  // ---- backward chain: dh_{l-1} = dpre_l @ W_l^T, dpre_{l-1} = dh_{l-1} * silu'(pre_{l-1})
  for (int l = N.nl - 1; l >= 1; --l) {
    const int kp = N.kp[l], np = N.np[l];
    if (w < kp / 16) {
      const f32x4 acc = bnn_tile_mm(sbuf[cur], Pm + N.off_wt[l], np, kp, 16 * w, lane);
      const int col = 16 * w + (lane & 15);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 4 * (lane >> 4) + v, gr = row0 + r;
        float dp = 0.f;
        if (gr < A.rows) {
          const size_t o_ = (((size_t)(l - 1) * gridDim.y + e) * A.ldr + gr) * N.HP + col;
          const float x = A.pre[o_];               // written by this very lane in the forward (same wave / column / row map)
          const float sg = bnn_sigmoid(x);
          dp = acc[v] * (sg * (1.0f + x * (1.0f - sg)));
          A.dpre[o_] = dp;
        }
        sbuf[cur ^ 1][r][col] = dp;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// ---- hidden widths 257..400: k_bnn_fwd with SPW = 2 slices per wave and 404-float LDS rows.  A kernel of its own rather than a
// template parameter of k_bnn_fwd: the narrow kernel's instruction stream is pinned (tests/test_pendulum_cpu.py compares every existing
// kernel with its earlier build), and sharing one body moves its schedule.  Everything outside the two matrix chains is k_bnn_fwd's text.
// The wide instantiation's bnn_tile_mm: one layer of one 16-row tile, the first NS slices of wave w: acc[j] is the
// 16-column slice w + j * nw (nw = waves of the workgroup).  One LDS read of the A fragment feeds every slice; each slice is its own
// k-ascending MFMA chain, so the sum order of a column does not depend on NS.
template <int NS, int SPW, int LDA>
__device__ __forceinline__ void bnn_wide_mm_n(const float (*in)[LDA], const float* __restrict__ W, int kp, int ldw, int w, int nw, int lane,
                                              f32x4 (&acc)[SPW]) {
  const int i = lane & 15, kk = lane >> 4;
  const float* wp = W + (size_t)kk * ldw + 16 * w + i;
  for (int k0 = 0; k0 < kp; k0 += 4) {
    const float av = in[i][k0 + kk];
    float bv[NS];                    // every slice's load in flight before the first MFMA; static register indices: no scratch
#pragma unroll
    for (int j = 0; j < NS; ++j) bv[j] = wp[(size_t)k0 * ldw + 16 * j * nw];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[j], 0, 0, 0);
  }
}

// The wave's slices of a layer with ns = NP / 16 slices (slice w exists; slice w + nw when it is below ns; w is wave-uniform).
template <int SPW, int LDA>
__device__ __forceinline__ void bnn_wide_mm(const float (*in)[LDA], const float* __restrict__ W, int kp, int ldw, int w, int nw, int ns,
                                            int lane, f32x4 (&acc)[SPW]) {
  static_assert(SPW == 1 || SPW == 2, "one or two slices per wave");
#pragma unroll
  for (int j = 0; j < SPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (SPW == 2 && w + nw < ns) bnn_wide_mm_n<SPW, SPW, LDA>(in, W, kp, ldw, w, nw, lane, acc);
  else bnn_wide_mm_n<1, SPW, LDA>(in, W, kp, ldw, w, nw, lane, acc);
}

// Forward of the whole ensemble, wide (and, for BNN_TRAIN, the loss gradient and the backward chain down to the first layer's
// pre-activation gradient).  grid (ntiles, E), block 64 * nw with nw = max(ceil(HP / 16 / SPW), KP_0 / 16, NOP / 16) <= 16 waves.
// Wave w owns slices w, w + nw, ... (SPW of them at most) of every layer, in the forward and in the backward chain alike.
// KEEP IN STEP with k_bnn_fwd above: input staging, head split, loss gradient and partial sums are the same text in both kernels; a fix
// to one is a fix to the other.
template <int MODE>
__global__ __launch_bounds__(1024) void k_bnn_wide(const BnnFwdArgs A) {
  constexpr int SPW = ILSX_BNN_SPW_WIDE, LDA = ILSX_BNN_LDA_WIDE;
  __shared__ float sbuf[2][16][LDA];
  __shared__ float sred[ILSX_BNN_MAX_WAVES][2];
  const BnnNet& N = A.net;
  const int tile = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, nw = nthr >> 6;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // decides which slices exist: kept in a scalar register
  const int row0 = tile * 16;
  const float* Pm = N.P + (size_t)e * N.mstride;
  const int kp0 = N.kp[0], in_dim = N.in_dim, D = N.D;

  // ---- input tile, normalised on the load: (x - mean) / std, padded columns / rows zero
  for (int t = tid; t < 16 * kp0; t += nthr) {
    const int r = t / kp0, k = t - r * kp0, gr = row0 + r;
    float v = 0.f;
    if (gr < A.rows && k < in_dim) {
      float raw;
      if (A.ring) {
        long long slot = A.idx[(size_t)e * A.idx_ms + gr];
        if (slot < 0 || slot >= A.cap) slot = 0;
        raw = A.ring[(size_t)slot * A.rec + k];      // record: obs | act | ...
      } else {
        raw = A.x[(size_t)gr * in_dim + k];
      }
      v = (raw - N.mean[k]) / N.std[k];
    }
    sbuf[0][r][k] = v;
    if (MODE == BNN_TRAIN && gr < A.rows) A.xs[((size_t)e * A.ldr + gr) * kp0 + k] = v;
  }
  __syncthreads();

  int cur = 0;
  for (int l = 0; l < N.nl; ++l) {
    const int kp = N.kp[l], np = N.np[l];
    const bool head = (l == N.nl - 1);
    if (w < np / 16) {
      f32x4 acc[SPW];
      bnn_wide_mm<SPW, LDA>(sbuf[cur], Pm + N.off_w[l], kp, np, w, nw, np / 16, lane, acc);
#pragma unroll
      for (int j = 0; j < SPW; ++j) {
        if (j == 0 || w + j * nw < np / 16) {
          const int col = 16 * (w + j * nw) + (lane & 15);
          const float bias = Pm[N.off_b[l] + col];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = 4 * (lane >> 4) + v, gr = row0 + r;
            const float x = acc[j][v] + bias;
            if (head) {
              sbuf[cur ^ 1][r][col] = x;
            } else {
              const float h = bnn_silu(x);
              sbuf[cur ^ 1][r][col] = h;
              if (MODE == BNN_TRAIN && gr < A.rows) {
                const size_t o_ = (((size_t)l * gridDim.y + e) * A.ldr + gr) * N.HP + col;
                A.pre[o_] = x;
                A.hs[o_] = h;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- head split (BNN.forward, networks.py:241-263): mean | log-var soft-clamped into [min_lv, max_lv]
  const float max_lv = 0.5f, min_lv = -10.0f;
  float s0 = 0.f, s1 = 0.f;
  for (int t = tid; t < 16 * N.NOP; t += nthr) {
    const int r = t / N.NOP, c = t - r * N.NOP, gr = row0 + r;
    if (c >= D) {
      if (MODE == BNN_TRAIN && c >= 2 * D) sbuf[cur ^ 1][r][c] = 0.f;
      continue;
    }
    const float mu = sbuf[cur][r][c], raw = sbuf[cur][r][D + c];
    const float lv1 = max_lv - bnn_softplus(max_lv - raw);
    const float lv = min_lv + bnn_softplus(lv1 - min_lv);
    if (MODE == BNN_PREDICT) {
      if (gr < A.rows) {
        const size_t o_ = ((size_t)e * A.rows + gr) * D + c;
        A.out_mean[o_] = mu;
        A.out_lv[o_] = A.out_var ? expf(lv) : lv;
      }
      continue;
    }
    float gmu = 0.f, graw = 0.f;
    if (gr < A.rows) {
      const long long slot0 = A.idx[(size_t)e * A.idx_ms + gr];
      const long long slot = (slot0 < 0 || slot0 >= A.cap) ? 0 : slot0;
      const float* R = A.ring + (size_t)slot * A.rec;
      // target [reward_scale * rew | next_obs - obs] (bnn_trainer.py:92-97)
      const float tg = c == 0 ? A.reward_scale * R[A.o + A.a] : R[A.o + A.a + 2 + (c - 1)] - R[c - 1];
      const float diff = mu - tg, sq = diff * diff;
      if (MODE == BNN_MSE && !A.add_var) {
        s0 += sq;
      } else {
        const float inv = expf(-lv);
        s0 += sq * inv;
        s1 += lv;
        if (MODE == BNN_TRAIN) {   // d/dmu, d/dlv of mean_e[ mean((mu - t)^2 e^-lv) + mean(lv) ]; lv = f(raw) through both softplus
          gmu = A.gscale * 2.0f * diff * inv;
          const float glv = A.gscale * (1.0f - sq * inv);
          graw = glv * bnn_sigmoid(lv1 - min_lv) * bnn_sigmoid(max_lv - raw);
        }
      }
    }
    if (MODE == BNN_TRAIN) {
      sbuf[cur ^ 1][r][c] = gmu;
      sbuf[cur ^ 1][r][D + c] = graw;
      if (gr < A.rows) {
        float* dh = A.dhead + ((size_t)e * A.ldr + gr) * N.NOP;
        dh[c] = gmu;
        dh[D + c] = graw;
      }
    }
  }
  if (MODE == BNN_PREDICT) return;
  // per-(member, tile) partial sums, fixed order
  s0 = bnn_wave_sum(s0);
  s1 = bnn_wave_sum(s1);
  if (lane == 0) { sred[w][0] = s0; sred[w][1] = s1; }
  __syncthreads();
  if (tid == 0) {
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < (nthr >> 6); ++q) { a0 += sred[q][0]; a1 += sred[q][1]; }
    A.partial[((size_t)e * A.ntiles + tile) * 2 + 0] = a0;
    A.partial[((size_t)e * A.ntiles + tile) * 2 + 1] = a1;
  }
  if (MODE != BNN_TRAIN) return;
  // padded head columns of the gradient tile (written above for c >= 2D) and columns [D, 2D) were set by the owners of c < D
  cur ^= 1;
  // ---- backward chain: dh_{l-1} = dpre_l @ W_l^T, dpre_{l-1} = dh_{l-1} * silu'(pre_{l-1})
  for (int l = N.nl - 1; l >= 1; --l) {
    const int kp = N.kp[l], np = N.np[l];
    if (w < kp / 16) {
      f32x4 acc[SPW];
      bnn_wide_mm<SPW, LDA>(sbuf[cur], Pm + N.off_wt[l], np, kp, w, nw, kp / 16, lane, acc);
#pragma unroll
      for (int j = 0; j < SPW; ++j) {
        if (j == 0 || w + j * nw < kp / 16) {
          const int col = 16 * (w + j * nw) + (lane & 15);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int r = 4 * (lane >> 4) + v, gr = row0 + r;
            float dp = 0.f;
            if (gr < A.rows) {
              const size_t o_ = (((size_t)(l - 1) * gridDim.y + e) * A.ldr + gr) * N.HP + col;
              const float x = A.pre[o_];           // written by this very lane in the forward (same wave / slice / column / row map)
              const float sg = bnn_sigmoid(x);
              dp = acc[j][v] * (sg * (1.0f + x * (1.0f - sg)));
              A.dpre[o_] = dp;
            }
            sbuf[cur ^ 1][r][col] = dp;
          }
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// Per-layer weight gradient + torch Adam with L2 weight decay, fused: wave = one 16x16 tile of dW_l (or 16 biases), the full row
// sum in-wave (no atomics, fixed order), then the optimiser step on exactly those parameters.  grid (ceil(ntasks / 4), E), block 256.
struct BnnDwArgs {
  float* P; float* M; float* V;
  long long mstride;
  int off_w[ILSX_BNN_MAX_LAYERS], off_wt[ILSX_BNN_MAX_LAYERS], off_b[ILSX_BNN_MAX_LAYERS];
  int kp[ILSX_BNN_MAX_LAYERS], np[ILSX_BNN_MAX_LAYERS], in_l[ILSX_BNN_MAX_LAYERS], out_l[ILSX_BNN_MAX_LAYERS];
  int task0[ILSX_BNN_MAX_LAYERS + 1];   // first task of layer l (weight tiles, then bias groups)
  float wd[ILSX_BNN_MAX_LAYERS];
  int nl, HP, NOP, rows, E;
  const float* xs; const float* hs; const float* dpre; const float* dhead; long long ldr;
  float lr_bc1, bc2_sqrt, b1, b2, eps;
};

__device__ __forceinline__ void bnn_adam(float* p, float* m, float* v, float g, float wd, const BnnDwArgs& A) {
  const float pv = *p;
  g = g + wd * pv;                                            // Adam(weight_decay): grad + wd * param
  float mv = *m;
  mv = mv + (1.0f - A.b1) * (g - mv);                         // exp_avg.lerp_(grad, 1 - beta1)
  const float vv = *v * A.b2 + (1.0f - A.b2) * g * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(vv) / A.bc2_sqrt + A.eps;
  *m = mv;
  *v = vv;
  *p = pv - A.lr_bc1 * (mv / denom);
}

__global__ __launch_bounds__(256) void k_bnn_dw_adam(const BnnDwArgs A) {
  const int lane = threadIdx.x & 63, e = blockIdx.y;
  const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= A.task0[A.nl]) return;
  int l = 0;
  while (task >= A.task0[l + 1]) ++l;
  const int local = task - A.task0[l];
  const int kp = A.kp[l], np = A.np[l];
  const int ntw = (kp / 16) * (np / 16);
  const bool head = (l == A.nl - 1);
  const float* Hin = l == 0 ? A.xs + (size_t)e * A.ldr * kp : A.hs + (((size_t)(l - 1) * A.E + e) * A.ldr) * A.HP;
  const int ldi = l == 0 ? kp : A.HP;
  const float* dP = head ? A.dhead + (size_t)e * A.ldr * A.NOP : A.dpre + (((size_t)l * A.E + e) * A.ldr) * A.HP;
  const int ldo = head ? A.NOP : A.HP;
  float* Pm = A.P + (size_t)e * A.mstride;
  float* Mm = A.M + (size_t)e * A.mstride;
  float* Vm = A.V + (size_t)e * A.mstride;
  const int R = A.rows;
  if (local < ntw) {
    const int ib = local / (np / 16), jb = local - ib * (np / 16);
    const int i = lane & 15, kk = lane >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < R; r0 += 4) {
      const int r = r0 + kk;
      const float av = r < R ? Hin[(size_t)r * ldi + 16 * ib + i] : 0.f;   // A[i][k] = h_{l-1}[row k][unit i]
      const float bv = r < R ? dP[(size_t)r * ldo + 16 * jb + i] : 0.f;    // B[k][j] = dpre_l[row k][unit j]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    const int jc = 16 * jb + (lane & 15);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int ir = 16 * ib + 4 * (lane >> 4) + v;
      if (ir < A.in_l[l] && jc < A.out_l[l]) {
        const size_t o_ = (size_t)A.off_w[l] + (size_t)ir * np + jc;
        bnn_adam(Pm + o_, Mm + o_, Vm + o_, acc[v], A.wd[l], A);
        Pm[(size_t)A.off_wt[l] + (size_t)jc * kp + ir] = Pm[o_];
      }
    }
  } else if (lane < 16) {
    const int jc = 16 * (local - ntw) + lane;
    if (jc < A.out_l[l]) {
      float g = 0.f;
      for (int r = 0; r < R; ++r) g += dP[(size_t)r * ldo + jc];
      const size_t o_ = (size_t)A.off_b[l] + jc;
      bnn_adam(Pm + o_, Mm + o_, Vm + o_, g, A.wd[l], A);
    }
  }
}

// partial sums [E][ntiles][2] -> out[E] = (s0 + s1) / denom, summed over tiles in order
__global__ void k_bnn_reduce(const float* __restrict__ partial, int E, int ntiles, float denom, float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float a0 = 0.f, a1 = 0.f;
  for (int t = 0; t < ntiles; ++t) { a0 += partial[((size_t)e * ntiles + t) * 2]; a1 += partial[((size_t)e * ntiles + t) * 2 + 1]; }
  out[e] = a0 / denom + a1 / denom;
}

// Normaliser statistics over ring rows idx[0..n) (bnn_trainer.py:113-118): column k per workgroup, double accumulators, fixed-order
// tree; mean, unbiased std (torch.std), std < 1e-12 -> 1, then FixedNormalizer's + 1e-8 (normalizer.py:101-103).
__global__ __launch_bounds__(256) void k_bnn_stats(const float* __restrict__ ring, long long cap, int rec, const int32_t* __restrict__ idx,
                                                   int n, float* __restrict__ mean, float* __restrict__ std) {
  __shared__ double red[256];
  __shared__ double mu_s;
  const int k = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int j = tid; j < n; j += 256) {
    long long slot = idx[j];
    if (slot < 0 || slot >= cap) slot = 0;
    s += (double)ring[(size_t)slot * rec + k];
  }
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) mu_s = red[0] / (double)n;
  __syncthreads();
  const float mu = (float)mu_s;
  s = 0.0;
  for (int j = tid; j < n; j += 256) {
    long long slot = idx[j];
    if (slot < 0 || slot >= cap) slot = 0;
    const double d = (double)ring[(size_t)slot * rec + k] - mu_s;
    s += d * d;
  }
  __syncthreads();
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    float sd = n > 1 ? (float)sqrt(red[0] / (double)(n - 1)) : __builtin_nanf("");
    if (sd < 1e-12f) sd = 1.0f;
    mean[k] = mu;
    std[k] = sd + 1e-8f;
  }
}

// FakeEnv.step + one step of MBPO._rollout_model (fake_env.py:30-75, mbpo.py:244-262), the part after the ensemble forward: the
// member of each row (uniform over the elites by Philox, or given), the Gaussian sample around its mean (explicit eps or Philox, or
// none when deterministic), next_obs = obs + mu[1:] + std * z, rew = mu[0] + std * z.
__global__ __launch_bounds__(256) void k_mbpo_sample(const float* __restrict__ mean, const float* __restrict__ lv, int n, int D,
                                                     const float* __restrict__ obs, const int32_t* __restrict__ elites, int n_elites,
                                                     const int32_t* __restrict__ midx_in, int deterministic, const float* __restrict__ eps,
                                                     uint64_t seed, uint64_t step, uint32_t stream, float* __restrict__ rew,
                                                     float* __restrict__ nobs, int32_t* __restrict__ midx_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int o = D - 1;
  int m;
  if (midx_in) {
    m = midx_in[r];
  } else {
    uint32_t c[4] = {(uint32_t)r, 0xFFFFFFFFu, (uint32_t)step, (uint32_t)(step >> 32) ^ (stream * 0x9E3779B9u)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ stream);
    int q = (int)(u01_open(c[0]) * (float)n_elites);
    if (q >= n_elites) q = n_elites - 1;
    m = elites[q];
  }
  if (midx_out) midx_out[r] = m;
  const float* mu = mean + ((size_t)m * n + r) * D;
  const float* lvr = lv + ((size_t)m * n + r) * D;
  for (int q = 0; 4 * q < D; ++q) {
    float z4[4] = {0.f, 0.f, 0.f, 0.f};
    if (!deterministic && !eps) philox_normal4(seed, step, stream, (uint32_t)r, (uint32_t)q, z4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // static register index: no scratch
      const int d = 4 * q + j;
      if (d < D) {
        float s = d == 0 ? mu[0] : mu[d] + obs[(size_t)r * o + d - 1];
        if (!deterministic) {
          const float z = eps ? eps[(size_t)r * D + d] : z4[j];
          s = s + sqrtf(expf(lvr[d])) * z;
        }
        if (d == 0) rew[r] = s;
        else nobs[(size_t)r * o + d - 1] = s;
      }
    }
  }
}

// Stable compaction of the non-terminal rows' next observations (obs = next_obs[~terminal], mbpo.py:268): one workgroup, 1024-row
// chunks, wave ballots.  *count receives the survivors.
__global__ __launch_bounds__(1024) void k_mbpo_compact(const float* __restrict__ nobs, const uint8_t* __restrict__ done, int n, int o,
                                                       float* __restrict__ out, int* __restrict__ count) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int i = c0 + tid;
    const bool f = i < n && !done[i];
    const unsigned long long mask = __ballot(f);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (f) {
      const float* src = nobs + (size_t)i * o;
      float* dst = out + (size_t)(off + pre) * o;
      for (int k = 0; k < o; ++k) dst[k] = src[k];
    }
    __syncthreads();
    if (tid == 0) {
      for (int q = 0; q < 16; ++q) base += wsum[q];
    }
    __syncthreads();
  }
  if (tid == 0) *count = base;
}
