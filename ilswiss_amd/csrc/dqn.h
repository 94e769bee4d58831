// dqn.h — the loss kernel of DQN / Double DQN and the epsilon-greedy argmax head (included by ilsx_ac.hip after dsac.h, whose HeadSlabs it reads through).
//   k_dqn_grad     dqn.py:79-84 / double_dqn.py:24-30: the bootstrap value from the target net at s' (its own max, or its entry at the online
//                  net's first maximal action), y = r + (1 - d) * discount * v, dL/dQ(s) of nn.MSELoss (column a only)
//   k_egreedy_act  ArgmaxDiscretePolicy (rlkit/policies/argmax.py) under EpsilonGreedy (exploration_strategies/epsilon_greedy.py:21-24)
// One lane per row; the n head outputs are re-read from global memory in each pass (n <= ILSX_MAX_NO), nothing is indexed in registers.
#pragma once

// first maximal entry of row r (numpy argmax / torch.max(1)[1])
__device__ __forceinline__ int head_argmax(const HeadSlabs& z, int r, int n, float* v_out) {
  int best = 0;
  float bv = z.get(r, 0, n);
  for (int j = 1; j < n; ++j) {
    const float v = z.get(r, j, n);
    if (v > bv) { bv = v; best = j; }
  }
  *v_out = bv;
  return best;
}

struct DqnGradArgs {
  HeadSlabs tq, qn, q;             // target net at s', online net at s' (Double DQN only), online net at s: [B][n] each
  const float *act, *rew, *done;   // [B] (action index as float)
  float* g;                        // dL/dQ(s) [B][n] (LOSS_GIVEN input)
  float *y, *qa;                   // per-row target and Q(s)[a] (statistics)
  int B, n, double_q;
  float gamma, inv_B;
};
__global__ __launch_bounds__(256) void k_dqn_grad(const DqnGradArgs A) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= A.B) return;
  const int n = A.n;
  float v;
  if (A.double_q) v = A.tq.get(r, head_argmax(A.qn, r, n, &v), n);   // double_dqn.py:24-25
  else head_argmax(A.tq, r, n, &v);                                  // dqn.py:79
  const float y = A.rew[r] + (1.0f - A.done[r]) * A.gamma * v;       // no reward scale in the reference's DQN
  // the one-hot action as a gather index: truncated toward zero and kept inside [0, n) (train_step refuses a non-index on the host)
  int a = (int)A.act[r];
  a = a < 0 ? 0 : (a >= n ? n - 1 : a);
  const float qa = A.q.get(r, a, n);
  for (int j = 0; j < n; ++j) A.g[(size_t)r * n + j] = j == a ? 2.0f * (qa - y) * A.inv_B : 0.0f;   // nn.MSELoss(): mean, no 0.5
  A.y[r] = y; A.qa[r] = qa;
}

// z[rows][n]: raw head outputs.  Stochastic: ONE Philox call per row keyed by (row, this call's counter); u0 <= epsilon takes the uniform
// action floor(u1 * n) (which may be the greedy one, as Discrete.sample() may), otherwise the first maximal entry.  The index is written as a float.
__global__ __launch_bounds__(256) void k_egreedy_act(const float* __restrict__ z, int rows, int n, int deterministic, float epsilon,
                                                     uint64_t seed, uint32_t stream, unsigned long long step, float* __restrict__ act) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  if (!deterministic) {
    uint32_t c[4] = {(uint32_t)r, 0u, (uint32_t)step, (uint32_t)(step >> 32) ^ (stream * 0x9E3779B9u)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ stream);
    if (u01_open(c[0]) <= epsilon) {
      const int k = (int)floorf(u01_open(c[1]) * (float)n);
      act[r] = (float)(k < n ? k : n - 1);
      return;
    }
  }
  float v;
  act[r] = (float)head_argmax(HeadSlabs{z, 1, rows}, r, n, &v);
}
