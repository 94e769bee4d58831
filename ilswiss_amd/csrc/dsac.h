// dsac.h — the categorical head and the two fused loss kernels of discrete SAC (included by ilsx_ac.hip).
//   k_categorical_act   DiscretePolicy.forward (rlkit/torch/common/policies.py:39-101): log_softmax of the last linear layer; stochastic =
//                       Gumbel-max argmax(z_j - log(-log u_j)), deterministic = first maximal log-probability; log pi(a|s) of the index taken
//   k_dsac_critic_grad  discrete_sac.py:77-104: target from pi(s') logits and the target critics, dL/dQ_i for both critics (column a only)
//   k_dsac_policy_grad  discrete_sac.py:131-143: dL/dz of -mean(alpha H(p) + sum_j p_j min(Q1, Q2)_j) on the post-update critics
// One lane per batch row; every per-row quantity is recomputed from global memory in each pass over the n outputs (n <= ILSX_MAX_NO),
// so nothing is indexed in registers and nothing spills.  Log-softmax is max-shifted.  The existing MLP kernels are not touched: the
// trunks run as HEAD_RAW forwards and LOSS_GIVEN backwards.
#pragma once

// a [rows][n] head output that may sit in cs column-slice partial slabs of `stride` rows (the column-split forward's `part`)
struct HeadSlabs {
  const float* p; int cs; int stride;
  __device__ __forceinline__ float get(int r, int j, int n) const {
    float s = p[(size_t)r * n + j];
    for (int c = 1; c < cs; ++c) s += p[((size_t)c * stride + r) * n + j];
    return s;
  }
};

// max-shifted log-sum-exp of row r: m = max_j z_j, returns m + log(sum_j exp(z_j - m)); *lse_s = log(sum) (log_softmax_j = (z_j - m) - lse_s)
__device__ __forceinline__ float head_logsumexp_parts(const HeadSlabs& z, int r, int n, float* m_out) {
  float m = -INFINITY;
  for (int j = 0; j < n; ++j) m = fmaxf(m, z.get(r, j, n));
  float s = 0.0f;
  for (int j = 0; j < n; ++j) s += expf(z.get(r, j, n) - m);
  *m_out = m;
  return logf(s);
}

__global__ __launch_bounds__(256) void k_categorical_act(const float* __restrict__ z, int rows, int n, int deterministic, uint64_t seed,
                                                         uint32_t stream, unsigned long long step, float* __restrict__ act,
                                                         float* __restrict__ logp) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const HeadSlabs Z{z, 1, rows};
  float m;
  const float ls = head_logsumexp_parts(Z, r, n, &m);
  int best = 0;
  float bv = -INFINITY;
  if (deterministic) {   // torch.max(log_probs, 1): the first maximal entry
    for (int j = 0; j < n; ++j) {
      const float l = (z[(size_t)r * n + j] - m) - ls;
      if (l > bv) { bv = l; best = j; }
    }
  } else {               // Gumbel-max on the pre-activations (policies.py:83-87); u_j from Philox (row, j / 4) of this call
    for (int j0 = 0; j0 < n; j0 += 4) {
      uint32_t c[4] = {(uint32_t)r, (uint32_t)(j0 >> 2), (uint32_t)step, (uint32_t)(step >> 32) ^ (stream * 0x9E3779B9u)};
      philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ stream);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        if (j < n) {
          const float u = u01_open(c[q]);
          const float v = z[(size_t)r * n + j] - logf(-logf(u));
          if (v > bv) { bv = v; best = j; }
        }
      }
    }
  }
  act[r] = (float)best;
  if (logp) logp[r] = (z[(size_t)r * n + best] - m) - ls;
}

// DiscretePolicy.get_log_pis (policies.py:99-100): log_softmax of the raw head z[rows][n], in place
__global__ __launch_bounds__(256) void k_categorical_log_softmax(float* __restrict__ z, int rows, int n) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const HeadSlabs Z{z, 1, rows};
  float m;
  const float ls = head_logsumexp_parts(Z, r, n, &m);
  for (int j = 0; j < n; ++j) z[(size_t)r * n + j] = (z[(size_t)r * n + j] - m) - ls;
}

struct DsacCriticArgs {
  HeadSlabs zn, tq1, tq2, q1, q2;   // pi(s') logits, target critics at s', critics at s: [B][n] each
  const float *act, *rew, *done;    // [B] (action index as float)
  float *g1, *g2;                   // dL/dQ_i [B][n] (LOSS_GIVEN inputs)
  float *y, *qa1, *qa2;             // per-row target and Q_i(s)[a] (statistics)
  int B, n;
  float alpha, gamma, reward_scale, inv_B;
};
__global__ __launch_bounds__(256) void k_dsac_critic_grad(const DsacCriticArgs A) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= A.B) return;
  const int n = A.n;
  float m;
  const float ls = head_logsumexp_parts(A.zn, r, n, &m);
  float ev = 0.0f, ent = 0.0f;   // sum_j p'_j min(TQ1, TQ2)_j ; H(p') = -sum_j p'_j l'_j
  for (int j = 0; j < n; ++j) {
    const float l = (A.zn.get(r, j, n) - m) - ls, p = expf(l);
    ev += p * fminf(A.tq1.get(r, j, n), A.tq2.get(r, j, n));
    ent -= p * l;
  }
  const float y = A.reward_scale * A.rew[r] + (1.0f - A.done[r]) * A.gamma * (ev + A.alpha * ent);
  // the sampled action column as a gather index (actions.long()): truncated toward zero and kept inside [0, n)
  int a = (int)A.act[r];
  a = a < 0 ? 0 : (a >= n ? n - 1 : a);
  const float q1 = A.q1.get(r, a, n), q2 = A.q2.get(r, a, n);
  for (int j = 0; j < n; ++j) {   // 0.5 * mean((Q_i[a] - y)^2): only column a receives gradient
    A.g1[(size_t)r * n + j] = j == a ? (q1 - y) * A.inv_B : 0.0f;
    A.g2[(size_t)r * n + j] = j == a ? (q2 - y) * A.inv_B : 0.0f;
  }
  A.y[r] = y; A.qa1[r] = q1; A.qa2[r] = q2;
}

struct DsacPolicyArgs {
  HeadSlabs z, q1, q2;   // pi(s) logits, post-update critics at s
  float* gz;             // dL/dz [B][n]
  float* ploss;          // per-row -(alpha H(p) + sum_j p_j Q_j)
  int B, n;
  float alpha, inv_B;
};
__global__ __launch_bounds__(256) void k_dsac_policy_grad(const DsacPolicyArgs A) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= A.B) return;
  const int n = A.n;
  float m;
  const float ls = head_logsumexp_parts(A.z, r, n, &m);
  // f_j = Q_j - alpha l_j ; E = sum_j p_j f_j = alpha H(p) + sum_j p_j Q_j ; dL/dz_k = -(1/B) p_k (f_k - E)
  float E = 0.0f;
  for (int j = 0; j < n; ++j) {
    const float l = (A.z.get(r, j, n) - m) - ls;
    E += expf(l) * (fminf(A.q1.get(r, j, n), A.q2.get(r, j, n)) - A.alpha * l);
  }
  for (int j = 0; j < n; ++j) {
    const float l = (A.z.get(r, j, n) - m) - ls;
    const float f = fminf(A.q1.get(r, j, n), A.q2.get(r, j, n)) - A.alpha * l;
    A.gz[(size_t)r * n + j] = -A.inv_B * expf(l) * (f - E);
  }
  A.ploss[r] = -E;
}
