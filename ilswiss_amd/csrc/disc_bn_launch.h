// disc_bn_launch.h — the device launcher of the BatchNorm phase code (disc_bn.h / disc_bn_step.h): k_dbn_par, k_dbn_col, the exact-fp32
// MFMA product k_dbn_gemm and `DbnLaunch`.  Included by ilsx_disc.hip at file scope and by ilsx_gcsl.hip inside a namespace of its own
// (each translation unit keeps its own kernel symbols).  Needs kernels.h (f32x4, MFMA16) and disc_bn.h in front of it.
#pragma once

// The phases of csrc/disc_bn.h in the order of csrc/disc_bn_step.h, every phase one launch on the ctx stream (the host test harness
// runs the same two headers as serial loops: tests/test_disc_bn_host.py).
template <class F> __global__ __launch_bounds__(256) void k_dbn_par(int n, F f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) f(i);
}
template <class F> __global__ __launch_bounds__(64) void k_dbn_col(F f) { f((int)blockIdx.x, (int)threadIdx.x); }   // one wavefront per feature column
// The matrix products of the step (DbnGemm, disc_bn.h): a 256-thread workgroup owns a 16 x 16 output tile; its four waves split the
// contraction into the four consecutive ranges of dbn_kq(Kd) terms, each wave staging its own 32-term chunks of both operands in its own
// LDS region (every global operand word is read once per tile, consecutive lanes along the operand's unit stride) and holding 2 x 2 outputs
// per lane; the four partial tiles are added in range order — the chain of dbn_gemm_elem, bit for bit.  Small tiles on purpose: the weight
// gradients contract over all rows into few outputs (128 x 128 outputs over 512 rows = 64 workgroups); 32 x 32 tiles without the split ran
// 23 us per launch (16 workgroups, 16 serial load -> LDS -> multiply rounds), one thread per element with a strided walk 50-100 us.
// Two independent products can share a launch.
struct DbnGemm2 { DbnGemm g[3]; int start[4], tn[3]; };   // start[i]: first workgroup of product i (start[3] = grid size)
struct DbnGemmLds { float red[4][256]; };   // the four waves' partial tiles
// One 16 x 16 output tile of one product, by the 256 threads of a workgroup: wave w contracts the w-th of the four consecutive ranges of
// dbn_kq(Kd) terms on the exact-fp32 matrix pipe — v_mfma_f32_16x16x4_f32 is an fmaf chain over its four k slots in ascending order
// (tools/ubench/mfma_32x32.hip checks it against a host fmaf chain), so a wave's partial is the chain dbn_gemm_elem states for its range, and
// the four partials are added in range order: the same bits as the host emulation (padding terms are 0 * 0 products: + 0.0f).  Operands go
// from memory straight into the fragment layout (lane = (row | column) + 16 x k slot): no LDS staging, no barrier inside the contraction —
// the round-5 form (every lane 2 x 2 outputs, both operands staged through 18 KB of LDS, two barriers per 32 terms) ran the single-XCD
// step's product phases twice as long.  Loads are issued DBN_GQ MFMAs ahead.
#define DBN_GQ 8
__device__ __forceinline__ void dbn_gemm_tile(const DbnGemm& g, int tile, int tn, DbnGemmLds& S) {
  const int i0 = (tile / tn) * 16, j0 = (tile % tn) * 16, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int lr = lane & 15, ks = lane >> 4;   // row of the A fragment / column of the B fragment ; k slot
  const int kq = dbn_kq(g.Kd), kbeg = wave * kq, kend = kbeg + kq < g.Kd ? kbeg + kq : g.Kd;
  const bool i_ok = i0 + lr < g.M, j_ok = j0 + lr < g.N;
  const float* pa = g.A + (size_t)(i0 + lr) * g.sai;
  const float* pb = g.B + (size_t)(j0 + lr) * g.sbj;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = kbeg; k0 < kend; k0 += 4 * DBN_GQ) {   // wave-uniform bounds
    float va[DBN_GQ], vb[DBN_GQ];
#pragma unroll
    for (int q = 0; q < DBN_GQ; ++q) {
      const int k = k0 + 4 * q + ks;
      va[q] = (i_ok && k < kend) ? pa[(size_t)k * g.sak] : 0.0f;
      vb[q] = (j_ok && k < kend) ? pb[(size_t)k * g.sbk] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < DBN_GQ; ++q)
      if (k0 + 4 * q < kend) acc = MFMA16(va[q], vb[q], acc);   // wave-uniform
  }
  __syncthreads();   // (the previous tile's reduction has been read)
#pragma unroll
  for (int v = 0; v < 4; ++v) S.red[wave][(4 * ks + v) * 16 + lr] = acc[v];   // accumulator layout: lane = column + 16 x (row / 4), register = row % 4
  __syncthreads();
  const int gi = i0 + (t >> 4), gj = j0 + (t & 15);
  if (gi < g.M && gj < g.N) {
    float v = ((S.red[0][t] + S.red[1][t]) + S.red[2][t]) + S.red[3][t];
    if (g.bias) v = v + g.bias[gj];
    float* c = g.C + (size_t)gi * g.ldc + gj;
    *c = g.acc ? *c + v : v;
  }
}
__global__ __launch_bounds__(256) void k_dbn_gemm(const DbnGemm2 G2) {
  __shared__ __attribute__((aligned(16))) DbnGemmLds S;
  const int which = (int)blockIdx.x >= G2.start[2] ? 2 : (int)blockIdx.x >= G2.start[1] ? 1 : 0;
  dbn_gemm_tile(G2.g[which], (int)blockIdx.x - G2.start[which], G2.tn[which], S);
}

struct DbnLaunch {
  hipStream_t st;
  template <class F> void par(int n, F f) { if (n > 0) hipLaunchKernelGGL(k_dbn_par<F>, dim3((n + 255) / 256), dim3(256), 0, st, n, f); }
  template <class F> void col(int H, F f) { if (H > 0) hipLaunchKernelGGL(k_dbn_col<F>, dim3(H), dim3(64), 0, st, f); }
  static int tiles(const DbnGemm& g, int* tn) { *tn = (g.N + 15) / 16; return g.Kd > 0 ? ((g.M + 15) / 16) * *tn : 0; }
  void launch(const DbnGemm* gs, int n) {   // up to three products nobody of which reads what another one writes
    DbnGemm2 G2;
    int at = 0;
    for (int i = 0; i < 3; ++i) {
      G2.g[i] = gs[i < n ? i : 0];
      G2.start[i] = at;
      G2.tn[i] = 1;
      if (i < n) at += tiles(gs[i], &G2.tn[i]);
    }
    G2.start[3] = at;
    if (at > 0) hipLaunchKernelGGL(k_dbn_gemm, dim3(at), dim3(256), 0, st, G2);
  }
  void gemm(const DbnGemm& g1) { launch(&g1, 1); }
  void gemm(const DbnGemm& g1, const DbnGemm& g2) { const DbnGemm gs[2] = {g1, g2}; launch(gs, 2); }
  void gemm(const DbnGemm& g1, const DbnGemm& g2, const DbnGemm& g3) { const DbnGemm gs[3] = {g1, g2, g3}; launch(gs, 3); }
};
