// ilsx_env.hip — HIP-resident batched planar articulated-body stepper + fused rollout step.
// Replaces the vec-env path of the reference: rlkit/envs/vecenvs.py:158-257 (reset/step protocol),
// rlkit/envs/worker/subproc.py:59-113 (one OS process + pipe per env), rlkit/envs/wrappers.py:342-352
// (NormalizedBoxEnv action map) and the MuJoCo call under gym's HopperEnv/Walker2dEnv.step
// (reward / termination formulas as restated in rlkit/envs/mujoco/hopper.py:11-40, walker2d.py:11-36).
//
// Sixteen lanes per env (env2d_group.h).  State is SoA float64 in HBM (qpos[d][env], qvel[d][env]); the per-env
// matrices (mass matrix / Cholesky factor, constraint Jacobian, the constraint-space matrix A) live in LDS.
// The model and its solver are stated in oracle/planar_env.py (the CPU oracle); physics parity with
// MuJoCo is UNPINNED (no MuJoCo here) — see DESIGN.md.
// Not a roofline kernel: ~160 B of HBM traffic and O(1e4) fp64 FLOP per env-step on a serial chain.
#include <algorithm>
#include <cmath>

#include "host_common.h"
#include "env3d.h"
#include "env3d_wave.h"

#define ENV_MAXB 8
#define ENV_MAXG 8

struct PlanarModelDev {
  int nb, ng, task, frame_skip, pgs_iters, max_rows, n_act, obs_dim;
  int parent[ENV_MAXB], limited[ENV_MAXB], act_body[ENV_MAXB], geom_body[ENV_MAXG], ancmask[ENV_MAXB];
  double anchor[ENV_MAXB][2], com[ENV_MAXB][2], mass[ENV_MAXB], inertia[ENV_MAXB], jsign[ENV_MAXB];
  double armature[ENV_MAXB], damping[ENV_MAXB], range[ENV_MAXB][2], gear[ENV_MAXB], stiffness[ENV_MAXB];
  double gp1[ENV_MAXG][2], gp2[ENV_MAXG][2], grad[ENV_MAXG], gfric[ENV_MAXG];
  double timestep, gravity, reset_noise, margin, reset_noise_vel_std, qvel_clip;
  double c_solref[2], c_solimp[3], l_solref[2], l_solimp[3];
  double ctrl_cost, alive, z_min, z_max, ang_max, state_max;
  double init_qpos[ENV_MAXB + 2];
  // ScaledEnv / MinmaxEnv (wrappers.py:53-203): every observation the env produces is (raw - shift) * inv_scale
  double obs_shift[2 * (ENV_MAXB + 2)], obs_inv_scale[2 * (ENV_MAXB + 2)];
};

struct EnvStepArgs;
struct ilsx_vecenv {
  ilsx_ctx* ctx = nullptr;
  DevOwner own;   // every device allocation of this handle, at creation or later: ilsx_vecenv_destroy gives all of it back
  // the step and reset kernels of this handle, chosen once at creation (env_select_planar / _spatial / _classic)
  int (*step_fn)(ilsx_vecenv*, ProfScope&, const EnvStepArgs&) = nullptr;
  int (*reset_fn)(ilsx_vecenv*, const int* ids_dev, int n_ids, float* obs, unsigned long long step) = nullptr;
  PlanarModelDev hm;
  PlanarModelDev* dm = nullptr;
  int n_env = 0, n = 0, o = 0, a = 0;
  double *qpos = nullptr, *qvel = nullptr;  // [n][n_env]
  float *obs_cur = nullptr, *act = nullptr, *nobs = nullptr, *rew = nullptr;
  uint8_t* done = nullptr;
  int* ep_len = nullptr;
  double* ep_ret = nullptr;
  double* stats = nullptr;  // [0] finished episodes, [1] sum of their returns, [2] env steps
  int* ids = nullptr;       // device scratch for id lists
  uint64_t seed = 0;
  uint32_t rng_stream = 0;
  unsigned long long step_ctr = 0;
  // running observation statistics (vecenvs.py:299-327, normalizer.py:128-152)
  struct ObsRms* rms = nullptr;
  float* obs_n = nullptr;   // [n_env][o] normalised policy input (norm_obs)
  // evaluation rollouts (ilsx_eval_rollout)
  float* act_label = nullptr;   // [n_env][a] expert labels (ilsx_rollout_step_relabel)
  unsigned char* ev_frozen = nullptr; double* ev_ret = nullptr; int* ev_len = nullptr; double* ev_stats = nullptr; int* ev_alive = nullptr;
  bool norm_obs = false, update_rms = false;
  // path mode (ilsx_vecenv_set_path_mode): whole episodes are staged and enter the ring when they end (base_algorithm.py:509-519)
  bool path_mode = false; float* stage = nullptr; int stage_len = 0, stage_rec = 0; int* flush_len = nullptr;
  int* flush_host = nullptr;            // pinned: the per-step read-back of the episode-end flags is a true asynchronous copy
  ilsx_replay* paths_pending = nullptr; // ilsx_rollout_step_begin enqueued a step whose finished episodes are not in the ring yet (ilsx_rollout_step_end)
  // run 0 of a lock-step group (ilsx_rollout_steps_lockstep): ONE array of episode-end flags for all K runs, so that a lock-step reads them back
  // with one copy instead of K (each a serialised 8 us on the stream)
  int* grp_flush_dev = nullptr; int* grp_flush_host = nullptr; int grp_flush_n = 0;
  // 3-D engine (Ant / Humanoid, env3d_wave.h): model and its device copy (the per-env working set lives in the stepping wave's LDS)
  int engine = 0, nq = 0, nv = 0;   // engine: 0 planar, 1 3-D, 2 classic control (classic_env.h)
  int classic = -1, discrete_n = 0;  // engine 2: ILSX_CLASSIC_* task and the size of its Discrete action space (0 = Box actions)
  struct CartChainDev* cc = nullptr; // engine 2, InvertedPendulum / InvertedDoublePendulum: the constants k_cartchain_step takes by value
  struct SwimmerDev* sw = nullptr;   // engine 2, classic == ILSX_SWIMMER_TASK: the constants k_swimmer_step takes by value (swimmer_env.h)
  struct LunarDev* ln = nullptr;     // engine 2, classic == ILSX_LUNAR_TASK: the constants k_lunar_step takes by value (lunar_env.h)
  struct GoalDev* gl = nullptr;      // engine 2, classic == ILSX_GOAL_TASK: the constants k_goal_step takes by value (goal_env.h)
  int goal_dobs = 0, goal_dg = 0;    // a goal env (> 0): the row is observation (goal_dobs) | desired_goal (goal_dg) | achieved_goal (goal_dg) and a
                                     // policy reads its first goal_dobs + goal_dg columns (env_policy_act)
  bool step_draws = false;           // the task draws random numbers on every step: ilsx_vecenv_step gives each step stream coordinates of its own
  Spatial3Dev* hm3 = nullptr; Spatial3Dev* dm3 = nullptr;
  // exploration strategy of a deterministic policy (ilsx_vecenv_set_exploration): one process per env, float64
  ilsx_explore_cfg explore = {0, 0, 0.0, 0.0, 0.0, 0.0, 1.0, -1.0, 1.0};
  double *ou_state = nullptr, *ou_sigma = nullptr;   // [n_env][a]: the OU state, and the sigma its next evolve uses (the previous call's)
  double explore_eps = 0.0;               // Gaussian kind: probability of a uniform action instead (ilsx_vecenv_set_exploration_epsilon)
  long long explore_t = 0;                // the t of the rollout's next steps (PolicyWrappedWithExplorationStrategy.set_num_steps_total)
  unsigned long long explore_calls = 0;   // Philox counter of k_explore (one draw per call)
  const float* policy_obs() const { return norm_obs ? obs_n : obs_cur; }
};

// RunningMeanStd (normalizer.py:128-152): float64, one owner workgroup per observation dimension (count is kept per
// dimension so that no workgroup depends on another's update).
#define ENV_MAX_OBS E3_MAXOBS
struct ObsRms { double mean[ENV_MAX_OBS], var[ENV_MAX_OBS], count[ENV_MAX_OBS]; };

// update(x) with x = the selected rows of src[n_rows][o]: batch mean / population variance in two passes (np.mean,
// np.var), then the parallel-variance merge.  flag != null: only rows whose flag is 0 (episodes that just ended).
__global__ __launch_bounds__(256) void k_obs_rms_update(const float* __restrict__ src, int n_rows, int o, const int* __restrict__ flag,
                                                        ObsRms* rms) {
  __shared__ double sh[4];
  __shared__ double bc;
  const int i = blockIdx.x, tid = threadIdx.x;
  auto bsum = [&](double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
  };
  double s = 0.0, n = 0.0;
  for (int r = tid; r < n_rows; r += 256)
    if (!flag || flag[r] == 0) { s += (double)src[(size_t)r * o + i]; n += 1.0; }
  s = bsum(s); n = bsum(n);
  if (n == 0.0) return;   // block-uniform
  const double bm = s / n;
  double ss = 0.0;
  for (int r = tid; r < n_rows; r += 256)
    if (!flag || flag[r] == 0) { const double d = (double)src[(size_t)r * o + i] - bm; ss += d * d; }
  ss = bsum(ss);
  if (tid == 0) {
    const double bv = ss / n, c = rms->count[i], mean = rms->mean[i], var = rms->var[i];
    const double delta = bm - mean, tot = c + n;
    const double m2 = var * c + bv * n + delta * delta * c * n / tot;
    rms->mean[i] = mean + delta * n / tot;
    rms->var[i] = m2 / tot;
    rms->count[i] = tot;
  }
  (void)bc;
}
// normalize_obs (vecenvs.py:299-327): clip((x - mean) / sqrt(var + eps), +-10), eps = np.finfo(float32).eps
__global__ __launch_bounds__(256) void k_obs_normalize(const float* src, float* dst, int n, int o, const ObsRms* __restrict__ rms) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int i = t % o;
  const double z = ((double)src[t] - rms->mean[i]) / sqrt(rms->var[i] + 1.1920928955078125e-07);
  dst[t] = (float)fmin(fmax(z, -10.0), 10.0);
}

// The tail of a fused rollout step of a normalising env that records into a ring (base_algorithm.py:183-277 over vecenvs.py:158-257): the ring
// holds what step() returned, i.e. normalised rows.  One workgroup owns observation dimension i and does, for its column, in the reference's
// order: update(nobs of all envs) — the arithmetic and reduction order of k_obs_rms_update, so the statistics are bit for bit that kernel's —,
// the record's observation segment = the policy input the step acted on, its next-observation segment = normalize(nobs) under the updated
// statistics, update(reset observations of the envs whose episode just ended, ep_len == 0), and the next policy input: reset rows normalised
// under the newest statistics, every other row THE SAME BITS as the record's next observation (never re-normalised).
// The record of env e is where the stepper put it: ring slot (top + e) mod cap, or with `stage` the staging row of the step just taken — the
// stepper wrote at the episode length before the step, which is ep_len - 1 now, or the flushed length - 1 when the episode ended.
struct NormRecordArgs {
  const float *nobs, *obs_cur;   // [n_env][o] raw: the step's observation (pre-reset), the env's current one (post auto-reset)
  float* obs_n;                  // [n_env][o] in: what the policy read; out: what it reads next
  const int* ep_len;             // [n_env] after the step: 0 = the episode ended in it
  const int* flush_len;          // path mode: length | terminal << 30 of the episodes that ended
  ObsRms* rms;
  float *ring, *stage;           // stage != null: path mode
  int n_env, o, a, rec, stage_len, update;
  long long cap, top;
};
// REG: up to 256 * NORM_REC_K envs — a thread's rows of the column (tid, tid + 256, ...) are read once, all loads in flight together, and
// every pass works on registers.  Otherwise every pass re-reads memory.  Both visit a thread's rows in the same order: the same sums.
#define NORM_REC_K 16
template <bool REG>
__global__ __launch_bounds__(256) void k_obs_norm_record(const NormRecordArgs A) {
  __shared__ double sh[4];
  constexpr int K = REG ? NORM_REC_K : 1;
  const int i = blockIdx.x, tid = threadIdx.x, o = A.o;
  auto rows = [&](auto f) {   // f(k, r) for this thread's rows r, k = the row's register slot
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (tid + 256 * k < A.n_env) f(k, tid + 256 * k);
    } else {
      for (int r = tid; r < A.n_env; r += 256) f(0, r);
    }
  };
  float x_next[K], x_cur[K], x_in[K];   // nobs, obs_cur and the policy input of the row
  int len[K];
  if constexpr (REG)
    rows([&](int k, int r) { const size_t at = (size_t)r * o + i; x_next[k] = A.nobs[at]; x_cur[k] = A.obs_cur[at]; x_in[k] = A.obs_n[at]; len[k] = A.ep_len[r]; });
  auto nobs_of = [&](int k, int r) { return REG ? x_next[k] : A.nobs[(size_t)r * o + i]; };
  auto cur_of = [&](int k, int r) { return REG ? x_cur[k] : A.obs_cur[(size_t)r * o + i]; };
  auto len_of = [&](int k, int r) { return REG ? len[k] : A.ep_len[r]; };
  auto bsum = [&](double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
  };
  // RunningMeanStd.update with the step's observations (ended == false) or with the reset observations of the envs whose episode ended;
  // every thread carries the column's statistics (all of them hold the same sums)
  double mean = A.rms->mean[i], var = A.rms->var[i], count = A.rms->count[i];
  auto update = [&](bool ended) {
    double s = 0.0, n = 0.0;
    rows([&](int k, int r) {
      if (!ended || len_of(k, r) == 0) { s += (double)(ended ? cur_of(k, r) : nobs_of(k, r)); n += 1.0; }
    });
    s = bsum(s); n = bsum(n);
    if (n == 0.0) return;   // block-uniform
    const double bm = s / n;
    double ss = 0.0;
    rows([&](int k, int r) {
      if (!ended || len_of(k, r) == 0) { const double d = (double)(ended ? cur_of(k, r) : nobs_of(k, r)) - bm; ss += d * d; }
    });
    ss = bsum(ss);
    const double bv = ss / n, delta = bm - mean, tot = count + n;
    const double m2 = var * count + bv * n + delta * delta * count * n / tot;
    mean = mean + delta * n / tot;
    var = m2 / tot;
    count = tot;
  };
  auto normalize = [](float x, double m, double v) {   // k_obs_normalize's expression
    const double z = ((double)x - m) / sqrt(v + 1.1920928955078125e-07);
    return (float)fmin(fmax(z, -10.0), 10.0);
  };
  if (A.update) update(false);
  const double mean1 = mean, var1 = var;
  const int next_off = o + A.a + 2;
  rows([&](int k, int r) {
    float* rec;
    if (A.stage) {
      const int l = len_of(k, r);
      const int row = (l ? l : (A.flush_len[r] & ((1 << 30) - 1))) - 1;
      if (row < 0 || row >= A.stage_len) return;   // (a stepper that flagged no length: nothing was staged)
      rec = A.stage + ((size_t)r * A.stage_len + row) * A.rec;
    } else {
      long long slot = A.top + r;
      if (slot >= A.cap) slot -= A.cap;
      rec = A.ring + (size_t)slot * A.rec;
    }
    rec[i] = REG ? x_in[k] : A.obs_n[(size_t)r * o + i];
    rec[next_off + i] = normalize(nobs_of(k, r), mean1, var1);
  });
  if (A.update) update(true);
  rows([&](int k, int r) {   // a row that goes on is normalised exactly as its record's next observation was: the same bits
    A.obs_n[(size_t)r * o + i] = len_of(k, r) == 0 ? normalize(cur_of(k, r), mean, var) : normalize(nobs_of(k, r), mean1, var1);
  });
  if (A.update && tid == 0) { A.rms->mean[i] = mean; A.rms->var[i] = var; A.rms->count[i] = count; }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double impedance_d(double r_abs, const double* solimp) {
  const double d0 = solimp[0], dmax = solimp[1], width = solimp[2];
  double x = width > 0.0 ? fmin(r_abs / width, 1.0) : 1.0;
  const double y = x < 0.5 ? 2.0 * x * x : 1.0 - 2.0 * (1.0 - x) * (1.0 - x);
  return d0 + y * (dmax - d0);
}

struct EnvStepArgs {
  const PlanarModelDev* m;
  double *qpos, *qvel;
  int n_env;
  const int* ids;         // nullable: step only these envs (compact i/o indexing)
  int n_ids;
  const float* act;       // [n_ids][a]
  float *obs, *rew;       // [n_ids][o], [n_ids]   (obs = observation AFTER the step, pre-reset)
  unsigned char* done;    // [n_ids]
  // fused-rollout extras (all nullable / 0)
  float* obs_cur;         // [n_env][o]: the policy's next input (post auto-reset)
  int auto_reset, max_path_length, no_terminal;
  float* stage; int stage_len; int* flush_len;   // path mode: records go to stage[env][step of the episode], flush_len[env] = length | terminal << 30 when the episode ends
  const float* rec_act;          // nullable: [n_ids][a] action written into the replay record instead of `act`
  const unsigned char* frozen;   // nullable: envs whose flag is set do not step (evaluation: one episode per env)
  int* ep_len; double* ep_ret; double* stats;
  float* replay; int rec; long long cap, top;   // transition record written at slot (top + env) % cap
  uint64_t seed; uint32_t stream; unsigned long long step;
};

template <int NB>
__device__ __forceinline__ void env_write_obs(const PlanarModelDev& m, const double (&q)[NB + 2], const double (&v)[NB + 2],
                                              float* dst) {
  constexpr int N = NB + 2;
#pragma unroll
  for (int i = 1; i < N; ++i) dst[i - 1] = (float)((q[i] - m.obs_shift[i - 1]) * m.obs_inv_scale[i - 1]);   // qpos[1:] (hopper.py:29-30)
#pragma unroll
  for (int i = 0; i < N; ++i)                                                                                // clip(qvel, +-10)
    dst[N - 1 + i] = (float)(((m.qvel_clip > 0.0 ? fmin(fmax(v[i], -m.qvel_clip), m.qvel_clip) : v[i]) - m.obs_shift[N - 1 + i]) *
                             m.obs_inv_scale[N - 1 + i]);
}

__device__ __forceinline__ double env_uniform(uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env,
                                              uint32_t k) {
  uint32_t c[4] = {env, k >> 2, (uint32_t)step, (uint32_t)(step >> 32) ^ (stream * 0x9E3779B9u)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ stream);
  return ((double)c[k & 3] + 0.5) * (1.0 / 4294967296.0);
}

template <int NB>
__device__ __forceinline__ void env_reset_state(const PlanarModelDev& m, uint64_t seed, uint32_t stream,
                                                unsigned long long step, uint32_t env, double (&q)[NB + 2],
                                                double (&v)[NB + 2]) {
  constexpr int N = NB + 2;  // hopper.py:32-40: init + U(+-reset_noise) on qpos and qvel
#pragma unroll
  for (int i = 0; i < N; ++i) {
    q[i] = m.init_qpos[i] + m.reset_noise * (2.0 * env_uniform(seed, stream, step, env, i) - 1.0);
    if (m.reset_noise_vel_std > 0.0) {   // HalfCheetahEnv.reset_model: qvel = init + 0.1 * randn (Box-Muller on two draws)
      const double u1 = env_uniform(seed, stream, step, env, N + 2 * i), u2 = env_uniform(seed, stream, step, env, N + 2 * i + 1);
      v[i] = m.reset_noise_vel_std * sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    } else {
      v[i] = m.reset_noise * (2.0 * env_uniform(seed, stream, step, env, N + i) - 1.0);
    }
  }
}

#include "env2d_group.h"
#include "classic_env.h"
#include "swimmer_env.h"
#include "lunar_env.h"
#include "goal_env.h"
#ifdef ILSX_EG_PROFILE
extern "C" int ilsx_debug_eg_prof(unsigned long long* out16, int reset) {   // measurement build only
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_eg_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_eg_prof), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#endif

template <int NB>
__global__ void k_env_reset(const PlanarModelDev* mp, double* qpos, double* qvel, int n_env, const int* ids, int n_ids,
                            float* obs, float* obs_cur, int* ep_len, double* ep_ret, uint64_t seed, uint32_t stream,
                            unsigned long long step) {
  constexpr int N = NB + 2;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_ids) return;
  const int env = ids ? ids[t] : t;
  const PlanarModelDev& m = *mp;
  double q[N], v[N];
  env_reset_state<NB>(m, seed, stream, step, (uint32_t)env, q, v);
  float ob[2 * N - 1];
  env_write_obs<NB>(m, q, v, ob);
  for (int i = 0; i < m.obs_dim; ++i) {
    if (obs) obs[(size_t)t * m.obs_dim + i] = ob[i];
    if (obs_cur) obs_cur[(size_t)env * m.obs_dim + i] = ob[i];
  }
  ep_len[env] = 0; ep_ret[env] = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) { qpos[(size_t)i * n_env + env] = q[i]; qvel[(size_t)i * n_env + env] = v[i]; }
}

// uniform(-1,1) actions: env.action_space.sample() per env while the replay is short (base_algorithm.py:369-380)
__global__ void k_random_actions(float* act, int n, uint64_t seed, uint32_t stream, unsigned long long step, int a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * a) return;
  const int env = t / a, k = t - env * a;
  act[t] = (float)(2.0 * env_uniform(seed, stream, step, (uint32_t)env, (uint32_t)k) - 1.0);
}

// Exploration strategies of a deterministic policy, one process per env (rlkit/exploration_strategies/gaussian_strategy.py:25-33,
// ou_strategy.py:46-60), float64 in the reference's order (FMA contraction is off for this file).  One thread per action component.
//   Gaussian: act = clip(act + N(0,1) * sigma(t), low, high)
//   OU      : x = state (mu at the first step of an episode: OUStrategy.reset) ; state = x + (theta * (mu - x) + sigma_prev * N(0,1)) ;
//             sigma_prev = sigma(t) — annealed AFTER the evolve, so a call uses the sigma of the call before it ; act = clip(act + state)
//   Gaussian with epsilon > 0 (MlpGaussianAndEpsilonPolicy, policies.py:537-552): an env whose uniform u0 < epsilon takes a uniform action
//             act_j = (float)(low + (high - low) * u_{1+j}) instead; u = the caller's [n_env][1 + a] or counters 0..a of a Philox stream of
//             its own.  One draw of u0 per ENV (the reference draws once per call for its whole batch: the same thing at one env).
struct ExploreArgs {
  int kind, n_env, a;
  double mu, theta, max_sigma, min_sigma, decay_period, low, high;
  long long t;
  double epsilon;
};
__global__ __launch_bounds__(256) void k_explore(const ExploreArgs X, float* __restrict__ act, const double* __restrict__ eps,
                                                 const double* __restrict__ u, double* __restrict__ state, double* __restrict__ sigma, const int* __restrict__ ep_len,
                                                 uint64_t seed, uint32_t stream, unsigned long long step) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n_env * X.a) return;
  const int env = i / X.a, j = i - env * X.a;
  if (X.kind == 1 && X.epsilon > 0.0) {
    const uint32_t ustream = stream ^ 0x00554E49u;   // 'UNI': apart from the stream of the normals
    const double u0 = u ? u[(size_t)env * (1 + X.a)] : env_uniform(seed, ustream, step, (uint32_t)env, 0);
    if (u0 < X.epsilon) {
      const double uj = u ? u[(size_t)env * (1 + X.a) + 1 + j] : env_uniform(seed, ustream, step, (uint32_t)env, (uint32_t)(1 + j));
      act[i] = (float)(X.low + (X.high - X.low) * uj);
      return;
    }
  }
  double e;
  if (eps) {
    e = eps[i];
  } else {
    float z4[4];
    philox_normal4(seed, step, stream, (uint32_t)env, (uint32_t)(j >> 2), z4);
    const int q = j & 3;
    e = (double)(q == 0 ? z4[0] : q == 1 ? z4[1] : q == 2 ? z4[2] : z4[3]);
  }
  const double sig_t = X.max_sigma - (X.max_sigma - X.min_sigma) * fmin(1.0, (double)X.t * 1.0 / X.decay_period);
  double noise;
  if (X.kind == 1) {
    noise = e * sig_t;
  } else {
    const double x = ep_len[env] == 0 ? X.mu : state[i];
    const double dx = X.theta * (X.mu - x) + sigma[i] * e;
    noise = x + dx;
    state[i] = noise;
    sigma[i] = sig_t;
  }
  act[i] = (float)fmin(fmax((double)act[i] + noise, X.low), X.high);
}

// ================================================================================================ 3-D engine kernels
// ---- wave-per-env form (env3d_wave.h): one 64-lane workgroup per env, working set in that wave's LDS (its reset draws; the kernels are
// in env3d_kernels.inc)
__device__ __forceinline__ void e3w_reset_state(e3w_lds* S, const Spatial3Dev& m, int lane, uint64_t seed, uint32_t stream, unsigned long long step,
                                                uint32_t envu) {
  // component i of qpos uses counter i, qvel nq + i (uniform) or nq + 2i, nq + 2i + 1 (Box-Muller)
  E3W_FOR(i, m.nq) S[E3WOff::Q0 + i] = m.init_qpos[i] + m.reset_noise * (2.0 * env_uniform(seed, stream, step, envu, i) - 1.0);
  E3W_FOR(i, m.nv) {
    if (m.reset_noise_vel_std > 0.0) {
      const double u1 = env_uniform(seed, stream, step, envu, m.nq + 2 * i), u2 = env_uniform(seed, stream, step, envu, m.nq + 2 * i + 1);
      S[E3WOff::V0 + i] = m.reset_noise_vel_std * sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    } else {
      S[E3WOff::V0 + i] = m.reset_noise * (2.0 * env_uniform(seed, stream, step, envu, m.nq + i) - 1.0);
    }
  }
  E3W_FOR(k, m.n_act) S[E3WOff::CTRL + k] = 0.0;   // qfrc_actuator of a freshly reset model is zero
  E3W_SYNC();
  const double qw = S[E3WOff::Q0 + 3], qx = S[E3WOff::Q0 + 4], qy = S[E3WOff::Q0 + 5], qz = S[E3WOff::Q0 + 6];
  const double nrm = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  E3W_SYNC();
  E3W_ONE { S[E3WOff::Q0 + 3] = qw * nrm; S[E3WOff::Q0 + 4] = qx * nrm; S[E3WOff::Q0 + 5] = qy * nrm; S[E3WOff::Q0 + 6] = qz * nrm; }
  E3W_SYNC();
}

#define E3K(name) name
#define E3K_TRUNC 0
#include "env3d_kernels.inc"
#undef E3K
#undef E3K_TRUNC
#define E3K(name) name##_trunc
#define E3K_TRUNC 1
#include "env3d_kernels.inc"
#undef E3K
#undef E3K_TRUNC

// ------------------------------------------------------------------------------------------------ host
// One launcher per kernel; a handle's two (step_fn, reset_fn) are chosen once, when it is created, by its engine's env_select_* below.
// launch_env_step / launch_env_reset own what is common: the empty call, the ProfScope, the step counter, the launch error.
// 16 lanes per env (env2d_group.h): one wavefront = one workgroup = 4 envs
template <int NB, int MR>
static int step_planar_group(ilsx_vecenv* e, ProfScope& ps, const EnvStepArgs& A) {
  const size_t lds = (((sizeof(PlanarModelDev) + 7) / 8) + (size_t)EG_ENVS * EgOff<NB, MR>::TOTAL) * sizeof(double);
  ILSX_LAUNCH(ps, (k_envg_step<NB, MR>), dim3((A.n_ids + EG_ENVS - 1) / EG_ENVS), dim3(64), lds, e->ctx->stream, A);
  return ILSX_OK;
}
#define ENV_STEP_FN(fn, kernel, grid, block, lds, ...)                                  \
  static int fn(ilsx_vecenv* e, ProfScope& ps, const EnvStepArgs& A) {                  \
    ILSX_LAUNCH(ps, kernel, grid, dim3(block), lds, e->ctx->stream, A, ##__VA_ARGS__);  \
    return ILSX_OK;                                                                     \
  }
#define ENV_RESET_FN(fn, kernel, grid, block, lds, ...)                                                      \
  static int fn(ilsx_vecenv* e, const int* ids_dev, int n_ids, float* obs, unsigned long long step) {        \
    hipLaunchKernelGGL(kernel, grid, dim3(block), lds, e->ctx->stream, __VA_ARGS__);                         \
    return ILSX_OK;                                                                                          \
  }
#define ENV_RESET_TAIL obs, e->obs_cur, e->ep_len, e->ep_ret, e->seed, e->rng_stream, step
#define LANES(n, per) dim3(((n) + (per) - 1) / (per))
// ---- planar engine
ENV_RESET_FN(reset_planar4, k_env_reset<4>, LANES(n_ids, 256), 256, 0, e->dm, e->qpos, e->qvel, e->n_env, ids_dev, n_ids, ENV_RESET_TAIL)
ENV_RESET_FN(reset_planar7, k_env_reset<7>, LANES(n_ids, 256), 256, 0, e->dm, e->qpos, e->qvel, e->n_env, ids_dev, n_ids, ENV_RESET_TAIL)
static int env_select_planar(ilsx_vecenv* e) {
  const int nb = e->hm.nb;
  const bool wide = e->hm.max_rows > 12;
  if (nb == 4) {
    e->step_fn = step_planar_group<4, 8>;
    e->reset_fn = reset_planar4;
  } else if (nb == 7) {
    e->step_fn = wide ? step_planar_group<7, 16> : step_planar_group<7, 12>;
    e->reset_fn = reset_planar7;
  } else {
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "vec-env kernels are instantiated for 4 (Hopper) and 7 (Walker2d) bodies, got %d", nb);
  }
  return ILSX_OK;
}
// ---- 3-D engine: wave per env (env3d_wave.h); *_trunc: the observation ends after qvel
#define E3W_LDS ((size_t)E3WOff::TOTAL * 8)
#define E3_DM (const Spatial3Dev*)e->dm3
ENV_STEP_FN(step_3dw_23, k_env3dw_step<23>, dim3(A.n_ids), 64, E3W_LDS, E3_DM)   // Humanoid
ENV_STEP_FN(step_3dw_14, k_env3dw_step<14>, dim3(A.n_ids), 64, E3W_LDS, E3_DM)   // Ant
ENV_STEP_FN(step_3dw_any, k_env3dw_step<0>, dim3(A.n_ids), 64, E3W_LDS, E3_DM)   // any other tree: run-time dof count
ENV_STEP_FN(step_3dw_23_trunc, k_env3dw_step_trunc<23>, dim3(A.n_ids), 64, E3W_LDS, E3_DM)
ENV_STEP_FN(step_3dw_14_trunc, k_env3dw_step_trunc<14>, dim3(A.n_ids), 64, E3W_LDS, E3_DM)
ENV_RESET_FN(reset_3dw, k_env3dw_reset, dim3(n_ids), 64, E3W_LDS, E3_DM, e->qpos, e->qvel, e->n_env, ids_dev, ENV_RESET_TAIL)
ENV_RESET_FN(reset_3dw_trunc, k_env3dw_reset_trunc, dim3(n_ids), 64, E3W_LDS, E3_DM, e->qpos, e->qvel, e->n_env, ids_dev, ENV_RESET_TAIL)
static void env_select_spatial(ilsx_vecenv* e) {   // obs_trunc comes with 14 or 23 dofs only (ilsx_vecenv_create_spatial)
  const bool trunc = e->hm3->obs_trunc != 0;
  if (e->nv == 23) e->step_fn = trunc ? step_3dw_23_trunc : step_3dw_23;
  else if (e->nv == 14) e->step_fn = trunc ? step_3dw_14_trunc : step_3dw_14;
  else e->step_fn = step_3dw_any;
  e->reset_fn = trunc ? reset_3dw_trunc : reset_3dw;
}
// ---- classic control, Swimmer and the lander: the lane-per-env frame (classic_env.h), one row per task
#define LANE_RESET_ARGS LaneResetArgs{e->qpos, e->qvel, e->n_env, ids_dev, n_ids, ENV_RESET_TAIL}
ENV_STEP_FN(step_cartpole, k_cartpole_step, LANES(A.n_ids, 256), 256, 0)
ENV_STEP_FN(step_pendulum, k_pendulum_step, LANES(A.n_ids, 256), 256, 0)
ENV_STEP_FN(step_cartchain1, k_cartchain_step<1>, LANES(A.n_ids, 256), 256, 0, *e->cc)
ENV_STEP_FN(step_cartchain2, k_cartchain_step<2>, LANES(A.n_ids, 256), 256, 0, *e->cc)
ENV_STEP_FN(step_swimmer, k_swimmer_step<3>, LANES(A.n_ids, 256), 256, 0, *e->sw)
ENV_STEP_FN(step_lunar, k_lunar_step, LANES(A.n_ids, 256), 256, 0, *e->ln)
ENV_STEP_FN(step_goal, k_goal_step, LANES(A.n_ids, 256), 256, 0, *e->gl)
ENV_STEP_FN(step_mountaincar_cont, k_mountaincar_cont_step, LANES(A.n_ids, 256), 256, 0)
ENV_STEP_FN(step_mountaincar, k_mountaincar_step, LANES(A.n_ids, 256), 256, 0)
ENV_STEP_FN(step_acrobot, k_acrobot_step, LANES(A.n_ids, 256), 256, 0)
ENV_RESET_FN(reset_cartpole, k_cartpole_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_pendulum, k_pendulum_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_cartchain1, k_cartchain_reset<1>, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_cartchain2, k_cartchain_reset<2>, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_swimmer, k_swimmer_reset<3>, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS, *e->sw)
ENV_RESET_FN(reset_lunar, k_lunar_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS, *e->ln)
ENV_RESET_FN(reset_goal, k_goal_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS, *e->gl)
ENV_RESET_FN(reset_mountaincar_cont, k_mountaincar_cont_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_mountaincar, k_mountaincar_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
ENV_RESET_FN(reset_acrobot, k_acrobot_reset, LANES(n_ids, 256), 256, 0, LANE_RESET_ARGS)
static const struct ClassicTask {
  int kind, n, o, a, discrete_n;   // n = degrees of freedom; discrete_n: the size of a Discrete action space, 0 = Box(-1, 1) actions
  decltype(ilsx_vecenv::step_fn) step;
  decltype(ilsx_vecenv::reset_fn) reset;
  int nq, nv;                      // widths of the state rows where they are not n (0: n)
} CLASSIC_TASKS[] = {
    {ILSX_CLASSIC_CARTPOLE, 2, 4, 1, 2, step_cartpole, reset_cartpole},
    {ILSX_CLASSIC_PENDULUM, 1, 3, 1, 0, step_pendulum, reset_pendulum},
    {ILSX_CLASSIC_INVERTED_PENDULUM, 2, 4, 1, 0, step_cartchain1, reset_cartchain1},
    {ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM, 3, 11, 1, 0, step_cartchain2, reset_cartchain2},
    {ILSX_CLASSIC_MOUNTAINCAR_CONT, 1, 2, 1, 0, step_mountaincar_cont, reset_mountaincar_cont},
    {ILSX_CLASSIC_MOUNTAINCAR, 1, 2, 1, 3, step_mountaincar, reset_mountaincar},
    {ILSX_CLASSIC_ACROBOT, 2, 6, 1, 3, step_acrobot, reset_acrobot},
    {ILSX_SWIMMER_TASK, 5, 8, 2, 0, step_swimmer, reset_swimmer},
    {ILSX_LUNAR_TASK, 3, 8, 2, 0, step_lunar, reset_lunar, 14, 4},   // qpos carries the terrain, qvel the sleep clock
    {ILSX_GOAL_TASK, 2, 8, 2, 0, step_goal, reset_goal, 4, 2},       // qpos carries the goal; the row is observation | desired_goal | achieved_goal
};
#undef ENV_STEP_FN
#undef ENV_RESET_FN
#undef ENV_RESET_TAIL
#undef LANE_RESET_ARGS
#undef LANES
#undef E3W_LDS
#undef E3_DM

static int launch_env_step(ilsx_vecenv* e, const EnvStepArgs& A) {
  if (A.n_ids <= 0) return ILSX_OK;
  ProfScope ps(e->ctx, ILSX_K_ENV_STEP);
  ILSX_TRY(e->step_fn(e, ps, A));
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}
static int launch_env_reset(ilsx_vecenv* e, const int* ids_dev, int n_ids, float* obs) {
  if (n_ids <= 0) return ILSX_OK;
  ILSX_TRY(e->reset_fn(e, ids_dev, n_ids, obs, ++e->step_ctr));
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// RunningMeanStd update with rows of `src` (all, or those whose flag is 0) then normalise src -> dst
static int env_obs_norm(ilsx_vecenv* e, const float* upd_src, int upd_rows, const int* flag, const float* src, float* dst, int rows) {
  if (!e->norm_obs) return ILSX_OK;
  hipStream_t st = e->ctx->stream;
  if (e->update_rms && upd_src && upd_rows > 0)
    hipLaunchKernelGGL(k_obs_rms_update, dim3(e->o), dim3(256), 0, st, upd_src, upd_rows, e->o, flag, e->rms);
  if (src && rows > 0)
    hipLaunchKernelGGL(k_obs_normalize, dim3((rows * e->o + 255) / 256), dim3(256), 0, st, src, dst, rows * e->o, e->o,
                       (const ObsRms*)e->rms);
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// A handle under construction: every early return of a creator gives back the handle, its host-side models and its device buffers
struct EnvGuard {
  ilsx_vecenv* e;
  ~EnvGuard() { if (e) ilsx_vecenv_destroy(e); }
};
static ilsx_vecenv* env_new(ilsx_ctx* ctx, int engine, int n_env, uint64_t seed) {
  ilsx_vecenv* e = new ilsx_vecenv();
  e->ctx = e->own.ctx = ctx; e->n_env = n_env; e->seed = seed; e->rng_stream = ctx->next_rng_stream++; e->engine = engine;
  return e;
}
// What every creator does once nq / nv / o / a and the kernels of the handle are known: the buffers all engines share, RunningMeanStd() and
// the first reset.  On success the handle is the caller's.
static int env_create_finish(EnvGuard& guard, ilsx_vecenv** out) {
  ilsx_vecenv* e = guard.e;
  const size_t N = (size_t)e->n_env;
  ILSX_TRY(e->own.alloc_bytes(&e->qpos, N * e->nq * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->qvel, N * e->nv * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->obs_cur, N * e->o * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->act, N * e->a * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->nobs, N * e->o * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->rew, N * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->done, N));
  ILSX_TRY(e->own.alloc_bytes(&e->ep_len, N * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->obs_n, N * e->o * 4));
  ILSX_TRY(e->own.alloc_bytes(&e->rms, sizeof(ObsRms)));
  ILSX_TRY(e->own.alloc_bytes(&e->ep_ret, N * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->stats, 4 * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->ids, N * 4));
  ObsRms h;   // RunningMeanStd(): mean 0, var 1, count 0 (normalizer.py:133-136)
  for (int i = 0; i < ENV_MAX_OBS; ++i) { h.mean[i] = 0.0; h.var[i] = 1.0; h.count[i] = 0.0; }
  HIPCHK(hipMemcpyAsync(e->rms, &h, sizeof h, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));   // h, and a model record a creator is uploading, are read by now
  ILSX_TRY(launch_env_reset(e, nullptr, e->n_env, nullptr));
  guard.e = nullptr;
  *out = e;
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_create(ilsx_ctx* ctx, const ilsx_planar_model* pm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !pm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create: bad argument");
  if (pm->n_body != 4 && pm->n_body != 7)
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "n_body=%d: kernels exist for 4 (Hopper) and 7 (Walker2d) bodies", pm->n_body);
  if (pm->n_geom < 1 || pm->n_geom > ENV_MAXG) ILSX_FAIL(ILSX_ERR_ARG, "n_geom=%d out of range", pm->n_geom);
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_vecenv* e = env_new(ctx, 0, n_env, seed);
  EnvGuard guard{e};
  PlanarModelDev& m = e->hm;
  memset(&m, 0, sizeof m);
  m.nb = pm->n_body; m.ng = pm->n_geom; m.task = pm->task; m.frame_skip = pm->frame_skip; m.pgs_iters = pm->pgs_iters;
  m.max_rows = pm->max_rows > 0 ? pm->max_rows : (pm->n_body == 4 ? 8 : 12);
  if (m.max_rows > 16) { ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "max_rows=%d: the kernels keep at most 16 constraint rows per env", m.max_rows); }
  int na = 0;
  for (int b = 0; b < m.nb; ++b) {
    m.parent[b] = pm->parent[b]; m.limited[b] = pm->limited[b];
    m.anchor[b][0] = pm->anchor[b][0]; m.anchor[b][1] = pm->anchor[b][1];
    m.com[b][0] = pm->com[b][0]; m.com[b][1] = pm->com[b][1];
    m.mass[b] = pm->mass[b]; m.inertia[b] = pm->inertia[b]; m.jsign[b] = pm->jsign[b];
    m.armature[b] = pm->armature[b]; m.damping[b] = pm->damping[b]; m.stiffness[b] = pm->stiffness[b];
    m.range[b][0] = pm->range[b][0]; m.range[b][1] = pm->range[b][1]; m.gear[b] = pm->gear[b];
    if (pm->gear[b] != 0.0) m.act_body[na++] = b;
    int mask = 0;
    for (int j = b; j >= 0; j = pm->parent[j]) mask |= 1 << j;
    m.ancmask[b] = mask;
    if (b > 0 && (pm->parent[b] < 0 || pm->parent[b] >= b)) ILSX_FAIL(ILSX_ERR_ARG, "parent[%d] must precede the body", b);
  }
  m.n_act = na;
  for (int g = 0; g < m.ng; ++g) {
    m.geom_body[g] = pm->geom_body[g];
    m.gp1[g][0] = pm->geom_p1[g][0]; m.gp1[g][1] = pm->geom_p1[g][1];
    m.gp2[g][0] = pm->geom_p2[g][0]; m.gp2[g][1] = pm->geom_p2[g][1];
    m.grad[g] = pm->geom_radius[g]; m.gfric[g] = pm->geom_friction[g];
  }
  m.timestep = pm->timestep; m.gravity = pm->gravity; m.reset_noise = pm->reset_noise; m.margin = pm->contact_margin;
  m.reset_noise_vel_std = pm->reset_noise_vel_std; m.qvel_clip = pm->qvel_clip;
  for (int i = 0; i < 2; ++i) { m.c_solref[i] = pm->contact_solref[i]; m.l_solref[i] = pm->limit_solref[i]; }
  for (int i = 0; i < 3; ++i) { m.c_solimp[i] = pm->contact_solimp[i]; m.l_solimp[i] = pm->limit_solimp[i]; }
  m.ctrl_cost = pm->ctrl_cost; m.alive = pm->alive_bonus; m.z_min = pm->z_min; m.z_max = pm->z_max;
  m.ang_max = pm->ang_max; m.state_max = pm->state_max;
  e->n = m.nb + 2; e->nq = e->nv = e->n; e->o = 2 * e->n - 1; e->a = na;
  m.obs_dim = e->o;
  for (int i = 0; i < e->n; ++i) m.init_qpos[i] = pm->init_qpos[i];
  for (int i = 0; i < 2 * (ENV_MAXB + 2); ++i) { m.obs_shift[i] = 0.0; m.obs_inv_scale[i] = 1.0; }
  ILSX_TRY(env_select_planar(e));
  ILSX_TRY(e->own.alloc_bytes(&e->dm, sizeof m));
  HIPCHK(hipMemcpyAsync(e->dm, &m, sizeof m, hipMemcpyHostToDevice, ctx->stream));
  return env_create_finish(guard, out);
}

// 3-D models (Ant / Humanoid): same handle type, same protocol entry points; the engine behind step / reset is env3d_wave.h
extern "C" int ilsx_vecenv_create_spatial(ilsx_ctx* ctx, const ilsx_spatial_model* sm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !sm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_spatial: bad argument");
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_vecenv* e = env_new(ctx, 1, n_env, seed);
  EnvGuard guard{e};
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_step<23>, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_step<14>, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_step<0>, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_reset, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_step_trunc<23>, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_step_trunc<14>, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  HIPCHK(hipFuncSetAttribute((const void*)k_env3dw_reset_trunc, hipFuncAttributeMaxDynamicSharedMemorySize, E3WOff::TOTAL * 8));
  e->hm3 = new Spatial3Dev();
  Spatial3Dev& m = *e->hm3;
  if (const char* why = e3_build_model(sm, m)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_spatial: %s", why);
  if (m.obs_trunc && m.nv != 23 && m.nv != 14)   // the truncated wave kernel is built for the Humanoid's and the Ant's dof counts only
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_vecenv_create_spatial: obs_trunc is available for the Ant (14 dofs) and the Humanoid (23), not for %d dofs", m.nv);
  e->n = m.nq; e->nq = m.nq; e->nv = m.nv; e->o = m.obs_dim; e->a = m.n_act;
  env_select_spatial(e);
  ILSX_TRY(e->own.alloc_bytes(&e->dm3, sizeof m));
  HIPCHK(hipMemcpyAsync(e->dm3, &m, sizeof m, hipMemcpyHostToDevice, ctx->stream));
  return env_create_finish(guard, out);
}
// Classic control (classic_env.h): CartPole, Pendulum and the cart-and-poles tasks, one lane per env, the same handle and protocol entry
// points as the other engines.  cc != null: InvertedPendulum / InvertedDoublePendulum with these constants; sw != null: Swimmer with these;
// ln != null: the lander with these; gl != null: the goal env with these.
static int create_classic(ilsx_ctx* ctx, int kind, const CartChainDev* cc, int n_env, uint64_t seed, ilsx_vecenv** out,
                          const SwimmerDev* sw = nullptr, const LunarDev* ln = nullptr, const GoalDev* gl = nullptr) {
  HIPCHK(hipSetDevice(ctx->device));
  ilsx_vecenv* e = env_new(ctx, 2, n_env, seed);
  EnvGuard guard{e};
  const ClassicTask* task = nullptr;
  for (const ClassicTask& t : CLASSIC_TASKS)
    if (t.kind == kind) task = &t;
  if (!task) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "classic control: unknown kind %d", kind);
  e->classic = kind; e->discrete_n = task->discrete_n;
  e->n = task->n; e->nq = task->nq ? task->nq : task->n; e->nv = task->nv ? task->nv : task->n; e->o = task->o; e->a = task->a;
  e->step_fn = task->step; e->reset_fn = task->reset;
  if (cc) e->cc = new CartChainDev(*cc);
  if (sw) e->sw = new SwimmerDev(*sw);
  if (ln) { e->ln = new LunarDev(*ln); e->step_draws = true; }
  if (gl) { e->gl = new GoalDev(*gl); e->goal_dobs = PointReachTask::D_OBS; e->goal_dg = PointReachTask::D_GOAL; }
  return env_create_finish(guard, out);
}

// MuJoCo's capsule rule as ilswiss_amd/envs/models.py states it (capsule_mass_inertia): m = rho pi r^2 (L + r), inertia about the COM
static void cartchain_capsule(double L, double r, double* mass, double* inertia) {
  const double rho = 1000.0, pi = 3.141592653589793;
  const double m_c = rho * pi * r * r * L, m_s = rho * pi * (r * r * r);
  *mass = m_c + m_s;
  *inertia = m_c * (L * L / 12.0 + r * r / 4.0) + m_s * (2.0 * r * r / 5.0 + L * L / 4.0 + 3.0 * L * r / 8.0);
}

// The built-in constants: the values of ilswiss_amd/envs/models_cartchain.py (gym 0.22's inverted_pendulum.xml / inverted_double_pendulum.xml
// as authored there, UNVERIFIED against MuJoCo)
static void cartchain_defaults(int n_pole, ilsx_cartchain_model* m) {
  memset(m, 0, sizeof *m);
  const double pi = 3.141592653589793;
  m->n_pole = n_pole; m->pgs_iters = 30; m->gravity = 9.81; m->jsign = -1.0;
  m->limit_solref[0] = 0.02; m->limit_solref[1] = 1.0;
  m->limit_solimp[0] = 0.9; m->limit_solimp[1] = 0.95; m->limit_solimp[2] = 0.001;
  cartchain_capsule(0.2, 0.1, &m->mass[0], &m->inertia[0]);   // cart: capsule of radius 0.1, half-length 0.1 along x, COM at its origin
  m->limited[0] = 1; m->range[0][0] = -1.0; m->range[0][1] = 1.0;
  if (n_pole == 1) {
    m->timestep = 0.02; m->frame_skip = 2; m->gear = 100.0; m->ctrl_range[0] = -3.0; m->ctrl_range[1] = 3.0;
    cartchain_capsule(hypot(0.001, 0.6), 0.049, &m->mass[1], &m->inertia[1]);
    m->com[1][0] = 0.5 * 0.001; m->com[1][1] = 0.5 * 0.6;
    m->tip[0] = 0.001; m->tip[1] = 0.6;
    m->damping[0] = m->damping[1] = 1.0;
    m->limited[1] = 1; m->range[1][0] = -90.0 * (pi / 180.0); m->range[1][1] = 90.0 * (pi / 180.0);
  } else {
    m->timestep = 0.01; m->frame_skip = 5; m->gear = 500.0; m->ctrl_range[0] = -1.0; m->ctrl_range[1] = 1.0;
    for (int k = 1; k <= 2; ++k) {
      cartchain_capsule(0.6, 0.045, &m->mass[k], &m->inertia[k]);
      m->com[k][0] = 0.0; m->com[k][1] = 0.5 * 0.6;
    }
    m->anchor[2][0] = 0.0; m->anchor[2][1] = 0.6;
    m->tip[0] = 0.0; m->tip[1] = 0.6;
    m->damping[0] = m->damping[1] = m->damping[2] = 0.05;
  }
}

extern "C" int ilsx_vecenv_create_cartchain(ilsx_ctx* ctx, const ilsx_cartchain_model* pm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !pm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_cartchain: bad argument");
  if (pm->n_pole != 1 && pm->n_pole != 2) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "n_pole=%d: kernels exist for 1 and 2 poles", pm->n_pole);
  const int n = pm->n_pole + 1;
  if (pm->frame_skip < 1 || pm->pgs_iters < 1 || !(pm->timestep > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "cartchain: frame_skip, pgs_iters and timestep must be positive");
  if (pm->n_pole == 2 && pm->limited[2]) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "cartchain: the kernel solves limit rows on DoF 0 and DoF 1 only");
  if (!(pm->ctrl_range[0] < pm->ctrl_range[1])) ILSX_FAIL(ILSX_ERR_ARG, "cartchain: empty ctrl_range");
  if (!(pm->limit_solref[0] > 0.0) || !(pm->limit_solref[1] > 0.0) || !(pm->limit_solimp[0] > 0.0) || !(pm->limit_solimp[1] > 0.0))
    ILSX_FAIL(ILSX_ERR_ARG, "cartchain: limit_solref and the impedances of limit_solimp must be positive");
  CartChainDev d;
  memset(&d, 0, sizeof d);
  d.frame_skip = pm->frame_skip; d.pgs_iters = pm->pgs_iters;
  for (int i = 0; i < n; ++i) {
    if (!(pm->mass[i] > 0.0) || pm->inertia[i] < 0.0 || pm->armature[i] < 0.0) ILSX_FAIL(ILSX_ERR_ARG, "cartchain: body %d needs mass > 0, inertia >= 0, armature >= 0", i);
    d.mass[i] = pm->mass[i]; d.inertia[i] = pm->inertia[i]; d.armature[i] = pm->armature[i]; d.damping[i] = pm->damping[i];
    for (int k = 0; k < 2; ++k) { d.com[i][k] = pm->com[i][k]; d.anchor[i][k] = pm->anchor[i][k]; }
    if (i < 2) {
      d.limited[i] = pm->limited[i] != 0;
      d.range[i][0] = pm->range[i][0]; d.range[i][1] = pm->range[i][1];
      if (d.limited[i] && !(d.range[i][0] < d.range[i][1])) ILSX_FAIL(ILSX_ERR_ARG, "cartchain: DoF %d is limited to an empty range", i);
    }
  }
  if (pm->anchor[1][0] != 0.0 || pm->anchor[1][1] != 0.0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "cartchain: hinge 1 sits at the cart's origin");
  d.tip[0] = pm->tip[0]; d.tip[1] = pm->tip[1];
  d.gear = pm->gear; d.jsign = pm->jsign; d.timestep = pm->timestep; d.gravity = pm->gravity;
  for (int k = 0; k < 3; ++k) d.solimp[k] = pm->limit_solimp[k];
  const double tc = pm->limit_solref[0], dr = pm->limit_solref[1], dmax = pm->limit_solimp[1];
  d.lim_b = 2.0 / (dmax * tc);
  d.lim_k = 1.0 / (dmax * dmax * tc * tc * dr * dr);
  d.ctrl_lo = (float)pm->ctrl_range[0]; d.ctrl_hi = (float)pm->ctrl_range[1];
  return create_classic(ctx, pm->n_pole == 1 ? ILSX_CLASSIC_INVERTED_PENDULUM : ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM, &d, n_env, seed, out);
}

// Swimmer (swimmer_env.h): the caller's model is the one source of the constants.  Every field is checked before anything is allocated;
// create_classic gives back whatever it allocated when it fails.
extern "C" int ilsx_vecenv_create_swimmer(ilsx_ctx* ctx, const ilsx_swimmer_model* pm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !pm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_swimmer: bad argument");
  if (pm->n_link != 3) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "n_link=%d: the swimmer kernels exist for 3 links", pm->n_link);
  const int nl = pm->n_link, n = nl + 2;
  if (pm->frame_skip < 1 || pm->pgs_iters < 1 || !(pm->timestep > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: frame_skip, pgs_iters and timestep must be positive");
  if (!(pm->ctrl_range[0] < pm->ctrl_range[1])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: empty ctrl_range");
  if (!(pm->limit_solref[0] > 0.0) || !(pm->limit_solref[1] > 0.0) || !(pm->limit_solimp[0] > 0.0) || !(pm->limit_solimp[1] > 0.0))
    ILSX_FAIL(ILSX_ERR_ARG, "swimmer: limit_solref and the impedances of limit_solimp must be positive");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(pm->limit_solimp[k]) || (k < 2 && !std::isfinite(pm->limit_solref[k])) || (k < 2 && !std::isfinite(pm->ctrl_range[k])))
      ILSX_FAIL(ILSX_ERR_ARG, "swimmer: limit_solref, limit_solimp and ctrl_range must be finite");
  if (!std::isfinite(pm->timestep) || pm->limit_solimp[2] < 0.0) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: the time step must be finite and the impedance width not negative");
  if (!(pm->density >= 0.0) || !(pm->viscosity >= 0.0) || !std::isfinite(pm->density) || !std::isfinite(pm->viscosity))
    ILSX_FAIL(ILSX_ERR_ARG, "swimmer: the medium's density and viscosity must be finite and not negative");
  SwimmerDev d;
  memset(&d, 0, sizeof d);
  d.frame_skip = pm->frame_skip; d.pgs_iters = pm->pgs_iters;
  const double pi = 3.141592653589793, rho = pm->density, beta = pm->viscosity;
  for (int b = 0; b < nl; ++b) {
    if (!(pm->mass[b] > 0.0) || !std::isfinite(pm->mass[b])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: link %d needs a finite mass > 0", b);
    for (int k = 0; k < 3; ++k) {
      if (!(pm->inertia[b][k] >= 0.0) || !std::isfinite(pm->inertia[b][k])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: link %d needs finite inertias >= 0", b);
      if (!(pm->box[b][k] > 0.0) || !std::isfinite(pm->box[b][k])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: link %d needs finite box sides > 0", b);
    }
    d.mass[b] = pm->mass[b]; d.inertia[b] = pm->inertia[b][2];
    for (int k = 0; k < 2; ++k) {
      if (!std::isfinite(pm->com[b][k]) || !std::isfinite(pm->anchor[b][k])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: link %d needs a finite com and anchor", b);
      d.com[b][k] = pm->com[b][k]; d.anchor[b][k] = pm->anchor[b][k];
    }
    const double bx = pm->box[b][0], by = pm->box[b][1], bz = pm->box[b][2], dd = (bx + by + bz) / 3.0;
    d.drag[b][0] = 3.0 * pi * beta * dd;
    d.drag[b][1] = 0.5 * rho * by * bz;
    d.drag[b][2] = 0.5 * rho * bx * bz;
    d.drag[b][3] = pi * beta * (dd * dd * dd);
    d.drag[b][4] = rho * bz * (bx * bx * bx * bx + by * by * by * by) / 64.0;
  }
  if (pm->anchor[0][0] != 0.0 || pm->anchor[0][1] != 0.0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "swimmer: the root joints sit at the first link's origin");
  for (int i = 0; i < n; ++i) {
    if (!(pm->armature[i] >= 0.0) || !(pm->damping[i] >= 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: DoF %d needs armature >= 0 and damping >= 0", i);
    if (i < 3 && pm->limited[i]) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "swimmer: DoF %d is a root joint; only the hinges between links may be limited", i);
    if (i < 3 && pm->gear[i] != 0.0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "swimmer: DoF %d is a root joint; the actuators drive the hinges between links", i);
    if (!std::isfinite(pm->gear[i]) || !std::isfinite(pm->init_qpos[i])) ILSX_FAIL(ILSX_ERR_ARG, "swimmer: DoF %d needs a finite gear and init_qpos", i);
    d.armature[i] = pm->armature[i]; d.damping[i] = pm->damping[i]; d.init_qpos[i] = pm->init_qpos[i];
    if (i >= 3) {
      const int j = i - 3;
      d.limited[j] = pm->limited[i] != 0; d.gear[j] = pm->gear[i];
      d.range[j][0] = pm->range[i][0]; d.range[j][1] = pm->range[i][1];
      if (d.limited[j] && (!std::isfinite(d.range[j][0]) || !std::isfinite(d.range[j][1]) || !(d.range[j][0] < d.range[j][1])))
        ILSX_FAIL(ILSX_ERR_ARG, "swimmer: DoF %d is limited to an empty or non-finite range", i);
    }
  }
  d.timestep = pm->timestep;
  for (int k = 0; k < 3; ++k) d.solimp[k] = pm->limit_solimp[k];
  const double tc = pm->limit_solref[0], dr = pm->limit_solref[1], dmax = pm->limit_solimp[1];
  d.lim_b = 2.0 / (dmax * tc);
  d.lim_k = 1.0 / (dmax * dmax * tc * tc * dr * dr);
  d.ctrl_lo = (float)pm->ctrl_range[0]; d.ctrl_hi = (float)pm->ctrl_range[1];
  return create_classic(ctx, ILSX_SWIMMER_TASK, nullptr, n_env, seed, out, &d);
}

// The lander (lunar_env.h): the caller's model is the one source of the constants.  Every field is checked before anything is allocated;
// create_classic gives back whatever it allocated when it fails.
extern "C" int ilsx_vecenv_create_lunar(ilsx_ctx* ctx, const ilsx_lunar_model* pm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !pm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_lunar: bad argument");
  if (pm->frame_skip < 1 || pm->pgs_iters < 1) ILSX_FAIL(ILSX_ERR_ARG, "lunar: frame_skip and pgs_iters must be positive");
  const double all[] = {pm->fps, pm->scale, pm->w, pm->h, pm->gravity, pm->main_engine_power, pm->side_engine_power, pm->initial_random,
                        pm->side_engine_height, pm->side_engine_away, pm->leg_down, pm->helipad_y, pm->mass, pm->inertia, pm->com[0], pm->com[1],
                        pm->foot[0][0], pm->foot[0][1], pm->foot[1][0], pm->foot[1][1], pm->friction, pm->contact_solref[0], pm->contact_solref[1],
                        pm->contact_solimp[0], pm->contact_solimp[1], pm->contact_solimp[2], pm->sleep_lin_tol, pm->sleep_ang_tol, pm->sleep_time};
  for (double x : all)
    if (!std::isfinite(x)) ILSX_FAIL(ILSX_ERR_ARG, "lunar: every constant must be finite");
  if (!(pm->mass > 0.0) || !(pm->inertia > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "lunar: mass and inertia must be positive");
  if (!(pm->fps > 0.0) || !(pm->scale > 0.0) || !(pm->w > 0.0) || !(pm->h > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "lunar: fps, scale, w and h must be positive");
  if (!(pm->contact_solref[0] > 0.0) || !(pm->contact_solref[1] > 0.0) || !(pm->contact_solimp[0] > 0.0) || !(pm->contact_solimp[1] > 0.0))
    ILSX_FAIL(ILSX_ERR_ARG, "lunar: contact_solref and the impedances of contact_solimp must be positive");
  if (pm->contact_solimp[2] < 0.0 || pm->friction < 0.0) ILSX_FAIL(ILSX_ERR_ARG, "lunar: the impedance width and the friction must not be negative");
  if (!(pm->sleep_lin_tol > 0.0) || !(pm->sleep_ang_tol > 0.0) || !(pm->sleep_time > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "lunar: the sleep tolerances must be positive");
  double bottom = pm->hull[0][1];
  for (int k = 0; k < 6; ++k) {
    if (!std::isfinite(pm->hull[k][0]) || !std::isfinite(pm->hull[k][1])) ILSX_FAIL(ILSX_ERR_ARG, "lunar: every constant must be finite");
    bottom = std::fmin(bottom, pm->hull[k][1]);
  }
  for (int i = 0; i < 2; ++i)
    if (!(pm->foot[i][1] < bottom)) ILSX_FAIL(ILSX_ERR_ARG, "lunar: foot %d must lie below the hull's bottom (the hull has no contact response)", i);
  LunarDev d;
  memset(&d, 0, sizeof d);
  d.frame_skip = pm->frame_skip; d.pgs_iters = pm->pgs_iters;
  d.fps = pm->fps; d.scale = pm->scale; d.w = pm->w; d.h = pm->h; d.gravity = pm->gravity;
  d.main_power = pm->main_engine_power; d.side_power = pm->side_engine_power; d.initial_random = pm->initial_random;
  d.side_height = pm->side_engine_height; d.side_away = pm->side_engine_away; d.leg_down = pm->leg_down; d.helipad_y = pm->helipad_y;
  d.mass = pm->mass; d.inertia = pm->inertia;
  for (int k = 0; k < 2; ++k) { d.com[k] = pm->com[k]; d.foot[0][k] = pm->foot[0][k]; d.foot[1][k] = pm->foot[1][k]; }
  for (int k = 0; k < 6; ++k) { d.hull[k][0] = pm->hull[k][0]; d.hull[k][1] = pm->hull[k][1]; }
  d.friction = pm->friction;
  for (int k = 0; k < 3; ++k) d.solimp[k] = pm->contact_solimp[k];
  const double tc = pm->contact_solref[0], dr = pm->contact_solref[1], dmax = pm->contact_solimp[1];
  d.con_b = 2.0 / (dmax * tc);
  d.con_k = 1.0 / (dmax * dmax * tc * tc * dr * dr);
  d.sleep_lin2 = pm->sleep_lin_tol * pm->sleep_lin_tol; d.sleep_ang2 = pm->sleep_ang_tol * pm->sleep_ang_tol; d.sleep_time = pm->sleep_time;
  d.chunk_dx = pm->w / 10.0;
  return create_classic(ctx, ILSX_LUNAR_TASK, nullptr, n_env, seed, out, nullptr, &d);
}

// The goal env (goal_env.h): the caller's model is the one source of the constants, refused before anything is allocated unless every one
// is finite and positive.
extern "C" int ilsx_vecenv_create_goal(ilsx_ctx* ctx, const ilsx_goal_model* pm, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !pm || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_goal: bad argument");
  for (double x : {pm->tol, pm->step_scale, pm->p_range, pm->g_range})
    if (!std::isfinite(x) || !(x > 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "goal env: tol, step_scale, p_range and g_range must be finite and positive");
  if (pm->p_range > 1.0 || pm->g_range > 1.0) ILSX_FAIL(ILSX_ERR_ARG, "goal env: p_range and g_range lie inside the arena [-1, 1]");
  if (pm->reward_kind < 0 || pm->reward_kind > 1) ILSX_FAIL(ILSX_ERR_ARG, "goal env: reward_kind must be 0 (sparse) or 1 (dense)");
  GoalDev d;
  memset(&d, 0, sizeof d);
  d.tol = pm->tol; d.p_range = pm->p_range; d.g_range = pm->g_range; d.step_scale = (float)pm->step_scale; d.reward_kind = pm->reward_kind;
  return create_classic(ctx, ILSX_GOAL_TASK, nullptr, n_env, seed, out, nullptr, nullptr, &d);
}
extern "C" int ilsx_vecenv_goal_dims(const ilsx_vecenv* e, int* d_obs, int* d_goal) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  if (e->goal_dobs <= 0) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_vecenv_goal_dims: not a goal env");
  if (d_obs) *d_obs = e->goal_dobs;
  if (d_goal) *d_goal = e->goal_dg;
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_create_classic(ilsx_ctx* ctx, int kind, int n_env, uint64_t seed, ilsx_vecenv** out) {
  if (!ctx || !out || n_env < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_create_classic: bad argument");
  if (kind == ILSX_CLASSIC_INVERTED_PENDULUM || kind == ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM) {
    ilsx_cartchain_model m;
    cartchain_defaults(kind == ILSX_CLASSIC_INVERTED_PENDULUM ? 1 : 2, &m);
    return ilsx_vecenv_create_cartchain(ctx, &m, n_env, seed, out);
  }
  if (kind != ILSX_CLASSIC_CARTPOLE && kind != ILSX_CLASSIC_PENDULUM && kind != ILSX_CLASSIC_MOUNTAINCAR_CONT &&
      kind != ILSX_CLASSIC_MOUNTAINCAR && kind != ILSX_CLASSIC_ACROBOT)
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_vecenv_create_classic: unknown kind %d", kind);
  return create_classic(ctx, kind, nullptr, n_env, seed, out);
}
extern "C" int ilsx_vecenv_action_space(const ilsx_vecenv* e, int* discrete_n) {
  if (!e || !discrete_n) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_action_space: NULL argument");
  *discrete_n = e->discrete_n;
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_set_path_mode(ilsx_vecenv* e, int on) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  e->path_mode = on != 0;
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_state_dims(const ilsx_vecenv* e, int* nq, int* nv) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  if (nq) *nq = e->nq;
  if (nv) *nv = e->nv;
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_destroy(ilsx_vecenv* e) {
  if (!e) return ILSX_OK;
  hipSetDevice(e->ctx->device);
  hipStreamSynchronize(e->ctx->stream);
  e->own.release();
  if (e->flush_host) hipHostFree(e->flush_host);
  if (e->grp_flush_host) hipHostFree(e->grp_flush_host);
  delete e->hm3;
  delete e->cc;
  delete e->sw;
  delete e->ln;
  delete e->gl;
  delete e;
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_dims(const ilsx_vecenv* e, int* obs_dim, int* act_dim, int* n_dof, int* n_env) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  if (obs_dim) *obs_dim = e->o;
  if (act_dim) *act_dim = e->a;
  if (n_dof) *n_dof = e->n;
  if (n_env) *n_env = e->n_env;
  return ILSX_OK;
}

static int env_upload_ids(ilsx_vecenv* e, const int32_t* ids_host, int n_ids, const int** dev) {
  *dev = nullptr;
  if (!ids_host) return ILSX_OK;
  for (int i = 0; i < n_ids; ++i)
    if (ids_host[i] < 0 || ids_host[i] >= e->n_env) ILSX_FAIL(ILSX_ERR_ARG, "env id %d out of range", ids_host[i]);
  HIPCHK(hipMemcpyAsync(e->ids, ids_host, (size_t)n_ids * 4, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  *dev = e->ids;
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_reset(ilsx_vecenv* e, const int32_t* ids_host, int n_ids, float* obs) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  HIPCHK(hipSetDevice(e->ctx->device));
  if (!ids_host) n_ids = e->n_env;
  if (n_ids < 0 || n_ids > e->n_env) ILSX_FAIL(ILSX_ERR_ARG, "n_ids=%d out of range", n_ids);
  const int* dev = nullptr;
  ILSX_TRY(env_upload_ids(e, ids_host, n_ids, &dev));
  if (!e->norm_obs) return launch_env_reset(e, dev, n_ids, obs);
  // reset(id) returns normalised observations and feeds the running statistics (vecenvs.py:173-181)
  float* raw = obs ? obs : e->nobs;   // compact [n_ids][o]
  ILSX_TRY(launch_env_reset(e, dev, n_ids, raw));
  ILSX_TRY(env_obs_norm(e, raw, n_ids, nullptr, obs, obs, obs ? n_ids : 0));
  return env_obs_norm(e, nullptr, 0, nullptr, e->obs_cur, e->obs_n, e->n_env);
}

extern "C" int ilsx_vecenv_step(ilsx_vecenv* e, const float* act, const int32_t* ids_host, int n_ids, float* obs,
                                float* rew, uint8_t* done) {
  if (!e || !act) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_step: NULL argument");
  HIPCHK(hipSetDevice(e->ctx->device));
  if (!ids_host) n_ids = e->n_env;
  if (n_ids < 0 || n_ids > e->n_env) ILSX_FAIL(ILSX_ERR_ARG, "n_ids=%d out of range", n_ids);
  const int* dev = nullptr;
  ILSX_TRY(env_upload_ids(e, ids_host, n_ids, &dev));
  EnvStepArgs A;
  memset(&A, 0, sizeof A);
  A.m = e->dm; A.qpos = e->qpos; A.qvel = e->qvel; A.n_env = e->n_env;
  A.ids = dev; A.n_ids = n_ids; A.act = act; A.obs = obs; A.rew = rew; A.done = done;
  A.obs_cur = e->obs_cur;
  if (e->step_draws) { A.seed = e->seed; A.stream = e->rng_stream; A.step = ++e->step_ctr; }   // no auto-reset here: only advance draws
  if (!e->norm_obs) return launch_env_step(e, A);
  if (!obs) A.obs = e->nobs;
  ILSX_TRY(launch_env_step(e, A));   // step() returns normalised observations (vecenvs.py:251-257)
  ILSX_TRY(env_obs_norm(e, A.obs, n_ids, nullptr, obs, obs, obs ? n_ids : 0));
  return env_obs_norm(e, nullptr, 0, nullptr, e->obs_cur, e->obs_n, e->n_env);
}

extern "C" int ilsx_vecenv_get_state(ilsx_vecenv* e, double* qpos_host, double* qvel_host) {
  if (!e || !qpos_host || !qvel_host) ILSX_FAIL(ILSX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t N = e->n_env, nq = e->nq, nv = e->nv;
  std::vector<double> tq(N * nq), tv(N * nv);
  HIPCHK(hipMemcpyAsync(tq.data(), e->qpos, N * nq * 8, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipMemcpyAsync(tv.data(), e->qvel, N * nv * 8, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  for (size_t j = 0; j < N; ++j) {
    for (size_t i = 0; i < nq; ++i) qpos_host[j * nq + i] = tq[i * N + j];
    for (size_t i = 0; i < nv; ++i) qvel_host[j * nv + i] = tv[i * N + j];
  }
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_set_state(ilsx_vecenv* e, const double* qpos_host, const double* qvel_host) {
  if (!e || !qpos_host || !qvel_host) ILSX_FAIL(ILSX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(e->ctx->device));
  const size_t N = e->n_env, nq = e->nq, nv = e->nv;
  std::vector<double> tq(N * nq), tv(N * nv);
  for (size_t j = 0; j < N; ++j) {
    for (size_t i = 0; i < nq; ++i) tq[i * N + j] = qpos_host[j * nq + i];
    for (size_t i = 0; i < nv; ++i) tv[i * N + j] = qvel_host[j * nv + i];
  }
  HIPCHK(hipMemcpyAsync(e->qpos, tq.data(), N * nq * 8, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipMemcpyAsync(e->qvel, tv.data(), N * nv * 8, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return ILSX_OK;
}

extern "C" int ilsx_vecenv_cur_obs(ilsx_vecenv* e, float** dev_ptr) {
  if (!e || !dev_ptr) ILSX_FAIL(ILSX_ERR_ARG, "NULL argument");
  *dev_ptr = const_cast<float*>(e->policy_obs());
  return ILSX_OK;
}

// ------------------------------------------------------------------------------------------------ terminals.py
// One wave per row: lanes stride the row for the all-finite / all-below-100 scans, lane 0 applies the task's thresholds.
__global__ __launch_bounds__(256) void k_is_terminal(int kind, const float* __restrict__ x, int n, int o, unsigned char* done) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* r = x + (size_t)row * o;
  bool fin = true, below = true;
  if (kind == ILSX_TERM_INVERTED_PENDULUM || kind == ILSX_TERM_HOPPER || kind == ILSX_TERM_ANT)
    for (int i = lane; i < o; i += 64) {
      const float v = r[i];
      fin = fin && isfinite(v);
      if (i >= 1) below = below && (v < 100.0f);   // terminals.py:61: abs() wraps the comparison, so only an upper bound
    }
  fin = __all(fin); below = __all(below);
  if (lane != 0) return;
  bool d = false;
  if (kind == ILSX_TERM_INVERTED_PENDULUM) {
    d = !(fin && fabsf(r[1]) <= 0.2f);
  } else if (kind == ILSX_TERM_INVERTED_DOUBLE_PENDULUM) {
    const float th1 = atan2f(r[1], r[3]), th2 = atan2f(r[2], r[4]);
    d = 0.6f * (r[3] + cosf(th1 + th2)) <= 1.0f;
  } else if (kind == ILSX_TERM_HOPPER) {
    d = !(fin && below && r[0] > 0.7f && fabsf(r[1]) < 0.2f);
  } else if (kind == ILSX_TERM_WALKER2D) {
    d = !(r[0] > 0.8f && r[0] < 2.0f && r[1] > -1.0f && r[1] < 1.0f);
  } else if (kind == ILSX_TERM_HUMANOID) {
    d = r[0] < 1.0f || r[0] > 2.0f;
  } else if (kind == ILSX_TERM_ANT) {
    d = !(fin && r[0] >= 0.2f && r[0] <= 1.0f);
  }
  done[row] = d ? 1 : 0;
}

extern "C" int ilsx_is_terminal(ilsx_ctx* ctx, int kind, const float* next_obs, int n, int obs_dim, uint8_t* done) {
  if (!ctx || !next_obs || !done || n < 0) ILSX_FAIL(ILSX_ERR_ARG, "is_terminal: null argument or n < 0");
  static const int min_dim[7] = {2, 5, 2, 2, 1, 1, 1};
  if (kind < 0 || kind > ILSX_TERM_ANT) ILSX_FAIL(ILSX_ERR_ARG, "is_terminal: unknown kind %d", kind);
  if (obs_dim < min_dim[kind]) ILSX_FAIL(ILSX_ERR_ARG, "is_terminal: kind %d reads %d observation columns, got %d", kind, min_dim[kind], obs_dim);
  if (n == 0) return ILSX_OK;
  hipLaunchKernelGGL(k_is_terminal, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, kind, next_obs, n, obs_dim, done);
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// ScaledEnv (obs - mean)/(std + EPS) and MinmaxEnv (obs - min)/(max - min + EPS) (wrappers.py:53-203): a fixed affine map of
// every observation the env hands out or records; shift / scale are HOST float64 [obs_dim] (scale already includes EPS).
// The envs are reset so that the observations they currently show follow the new map.
extern "C" int ilsx_vecenv_set_obs_affine(ilsx_vecenv* e, const double* shift_host, const double* scale_host) {
  if (!e || !shift_host || !scale_host) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_set_obs_affine: NULL argument");
  if (e->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_vecenv_set_obs_affine: not available for goal envs (dictionary observations)");
  if (e->engine == 2) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_vecenv_set_obs_affine: not available for classic-control envs");
  HIPCHK(hipSetDevice(e->ctx->device));
  for (int i = 0; i < e->o; ++i) {
    if (!(scale_host[i] != 0.0)) ILSX_FAIL(ILSX_ERR_ARG, "observation scale %d is zero", i);
    if (e->engine == 1) { e->hm3->obs_shift[i] = shift_host[i]; e->hm3->obs_inv_scale[i] = 1.0 / scale_host[i]; }
    else { e->hm.obs_shift[i] = shift_host[i]; e->hm.obs_inv_scale[i] = 1.0 / scale_host[i]; }
  }
  if (e->engine == 1) HIPCHK(hipMemcpyAsync(e->dm3, e->hm3, sizeof(Spatial3Dev), hipMemcpyHostToDevice, e->ctx->stream));
  else HIPCHK(hipMemcpyAsync(e->dm, &e->hm, sizeof e->hm, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  ILSX_TRY(launch_env_reset(e, nullptr, e->n_env, nullptr));
  return env_obs_norm(e, nullptr, 0, nullptr, e->obs_cur, e->obs_n, e->n_env);
}

// vecenvs.py:104-113 (obs_rms / norm_obs / update_obs_rms attributes of BaseVectorEnv)
extern "C" int ilsx_vecenv_obs_norm(ilsx_vecenv* e, int norm_obs, int update_obs_rms) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  if (e->o > ENV_MAX_OBS) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "obs_dim %d > %d", e->o, ENV_MAX_OBS);
  if (norm_obs && e->goal_dobs > 0)
    ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_vecenv_obs_norm: norm_obs=1 is not available for goal envs (the reference's RunningMeanStd takes flat observations)");
  HIPCHK(hipSetDevice(e->ctx->device));
  e->norm_obs = norm_obs != 0; e->update_rms = update_obs_rms != 0;
  // the observations the envs currently show become the first batch, like the reset() that follows construction
  return env_obs_norm(e, e->obs_cur, e->n_env, nullptr, e->obs_cur, e->obs_n, e->n_env);
}
extern "C" int ilsx_vecenv_get_obs_rms(ilsx_vecenv* e, double* mean, double* var, double* count) {
  if (!e || !mean || !var || !count) ILSX_FAIL(ILSX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(e->ctx->device));
  ObsRms h;
  HIPCHK(hipMemcpyAsync(&h, e->rms, sizeof h, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  for (int i = 0; i < e->o; ++i) { mean[i] = h.mean[i]; var[i] = h.var[i]; }
  *count = h.count[0];
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_set_obs_rms(ilsx_vecenv* e, const double* mean, const double* var, double count) {
  if (!e || !mean || !var) ILSX_FAIL(ILSX_ERR_ARG, "NULL argument");
  HIPCHK(hipSetDevice(e->ctx->device));
  ObsRms h;
  for (int i = 0; i < ENV_MAX_OBS; ++i) { h.mean[i] = i < e->o ? mean[i] : 0.0; h.var[i] = i < e->o ? var[i] : 1.0; h.count[i] = count; }
  HIPCHK(hipMemcpyAsync(e->rms, &h, sizeof h, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return env_obs_norm(e, nullptr, 0, nullptr, e->obs_cur, e->obs_n, e->n_env);
}

// after an auto-resetting step: statistics see the step's observations, then the reset observations of the envs whose
// episode just ended (the reference's step() followed by reset(ids)), and the policy input is re-normalised
static int env_after_step_norm(ilsx_vecenv* e) {
  if (!e->norm_obs) return ILSX_OK;
  ILSX_TRY(env_obs_norm(e, e->nobs, e->n_env, nullptr, nullptr, nullptr, 0));
  return env_obs_norm(e, e->obs_cur, e->n_env, e->ep_len, e->obs_cur, e->obs_n, e->n_env);
}
// the same after a step that recorded into a ring (A: the stepper's arguments): statistics, the records' normalised observation segments and
// the next policy input in one launch (k_obs_norm_record)
#ifdef ILSX_NORM_RECORD_CHAIN
// Measurement build only (make VAR=chain VARFLAGS=-DILSX_NORM_RECORD_CHAIN, tools/bench_norm_rollout.py): the same step as four launches —
// the two existing statistics updates around an element-parallel record fix-up, then the reset rows.  Timed against the single launch in
// profiles/norm_rollout_bench.json; not part of the shipped library.
__global__ __launch_bounds__(256) void k_norm_chain_fix(const NormRecordArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_env * A.o) return;
  const int r = t / A.o, i = t - r * A.o;
  float* rec;
  if (A.stage) {
    const int len = A.ep_len[r];
    const int row = (len ? len : (A.flush_len[r] & ((1 << 30) - 1))) - 1;
    if (row < 0 || row >= A.stage_len) return;
    rec = A.stage + ((size_t)r * A.stage_len + row) * A.rec;
  } else {
    long long slot = A.top + r;
    if (slot >= A.cap) slot -= A.cap;
    rec = A.ring + (size_t)slot * A.rec;
  }
  const double z = ((double)A.nobs[t] - A.rms->mean[i]) / sqrt(A.rms->var[i] + 1.1920928955078125e-07);
  const float nn = (float)fmin(fmax(z, -10.0), 10.0);
  rec[i] = A.obs_n[t];
  rec[A.o + A.a + 2 + i] = nn;
  A.obs_n[t] = nn;
}
__global__ __launch_bounds__(256) void k_norm_chain_reset(const NormRecordArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_env * A.o) return;
  const int r = t / A.o, i = t - r * A.o;
  if (A.ep_len[r] != 0) return;
  const double z = ((double)A.obs_cur[t] - A.rms->mean[i]) / sqrt(A.rms->var[i] + 1.1920928955078125e-07);
  A.obs_n[t] = (float)fmin(fmax(z, -10.0), 10.0);
}
#endif
static int env_norm_record(ilsx_vecenv* e, const EnvStepArgs& A) {
  NormRecordArgs N;
  N.nobs = e->nobs; N.obs_cur = e->obs_cur; N.obs_n = e->obs_n; N.ep_len = e->ep_len; N.flush_len = A.flush_len; N.rms = e->rms;
  N.ring = A.replay; N.stage = A.stage; N.n_env = e->n_env; N.o = e->o; N.a = e->a; N.rec = A.rec; N.stage_len = A.stage_len;
  N.update = e->update_rms ? 1 : 0; N.cap = A.cap; N.top = A.top;
#ifdef ILSX_NORM_RECORD_CHAIN
  const dim3 grid((e->n_env * e->o + 255) / 256);
  if (N.update) hipLaunchKernelGGL(k_obs_rms_update, dim3(e->o), dim3(256), 0, e->ctx->stream, (const float*)e->nobs, e->n_env, e->o, (const int*)nullptr, e->rms);
  hipLaunchKernelGGL(k_norm_chain_fix, grid, dim3(256), 0, e->ctx->stream, N);
  if (N.update) hipLaunchKernelGGL(k_obs_rms_update, dim3(e->o), dim3(256), 0, e->ctx->stream, (const float*)e->obs_cur, e->n_env, e->o, (const int*)e->ep_len, e->rms);
  hipLaunchKernelGGL(k_norm_chain_reset, grid, dim3(256), 0, e->ctx->stream, N);
#else
  if (e->n_env <= 256 * NORM_REC_K) hipLaunchKernelGGL(k_obs_norm_record<true>, dim3(e->o), dim3(256), 0, e->ctx->stream, N);
  else hipLaunchKernelGGL(k_obs_norm_record<false>, dim3(e->o), dim3(256), 0, e->ctx->stream, N);
#endif
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}

// One iteration of BaseAlgorithm's sampling loop (base_algorithm.py:183-277) for ALL envs, on the device:
// actions (policy or uniform random) -> physics -> transition record into the replay ring -> auto-reset.
// The stepper's arguments for one fused rollout step of `e` (auto-reset, record into `rb`'s ring — or, with path mode on, into the per-env
// episode staging area, allocated on first use).
static int rollout_env_args(ilsx_vecenv* e, ilsx_replay* rb, int max_path_length, int no_terminal, unsigned long long step, EnvStepArgs* out) {
  EnvStepArgs& A = *out;
  memset(&A, 0, sizeof A);
  A.m = e->dm; A.qpos = e->qpos; A.qvel = e->qvel; A.n_env = e->n_env;
  A.ids = nullptr; A.n_ids = e->n_env; A.act = e->act;
  A.obs = e->nobs; A.rew = e->rew; A.done = e->done;
  A.obs_cur = e->obs_cur; A.auto_reset = 1; A.max_path_length = max_path_length;
  A.ep_len = e->ep_len; A.ep_ret = e->ep_ret; A.stats = e->stats;
  if (rb) { A.replay = rb->data; A.rec = rb->rec; A.cap = rb->cap; A.top = rb->top; }
  A.seed = e->seed; A.stream = e->rng_stream; A.step = step; A.no_terminal = no_terminal;
  if (rb && e->path_mode) {
    if (e->stage && (e->stage_rec != rb->rec || e->stage_len < max_path_length))
      ILSX_FAIL(ILSX_ERR_ARG, "path mode: staging holds %d-step episodes of %d-float records, asked for %d / %d", e->stage_len, e->stage_rec,
                max_path_length, rb->rec);
    if (!e->stage) {
      if (max_path_length < 1 || max_path_length >= rb->cap) ILSX_FAIL(ILSX_ERR_ARG, "path mode needs 1 <= max_path_length < replay capacity");
      ILSX_TRY(e->own.alloc_bytes(&e->stage, (size_t)e->n_env * max_path_length * rb->rec * 4));
      ILSX_TRY(e->own.alloc_bytes(&e->flush_len, (size_t)e->n_env * 4));
      e->stage_len = max_path_length; e->stage_rec = rb->rec;
      HIPCHK(hipHostMalloc((void**)&e->flush_host, (size_t)e->n_env * sizeof(int), hipHostMallocDefault));
    }
    A.stage = e->stage; A.stage_len = e->stage_len; A.flush_len = e->flush_len;
  }
  return ILSX_OK;
}
// path mode, second half of a step: wait for the step, move the episodes that ended in it from the staging area into the ring
// synced: the caller has already waited for the stream the step ran on; flags: where the step's episode-end flags were read back to (default: the env's own buffer)
static int rollout_paths_finish(ilsx_vecenv* e, bool synced = false, const int* flags = nullptr) {
  ilsx_replay* rb = e->paths_pending;
  if (!rb) return ILSX_OK;
  e->paths_pending = nullptr;
  if (!synced) HIPCHK(hipStreamSynchronize(e->ctx->stream));
  if (!flags) flags = e->flush_host;
  std::vector<int> envs, lens; std::vector<uint8_t> term;
  for (int i = 0; i < e->n_env; ++i)
    if (flags[i]) { envs.push_back(i); lens.push_back(flags[i] & ((1 << 30) - 1)); term.push_back((flags[i] >> 30) & 1); }
  return replay_insert_paths(rb, e->stage, e->stage_len, envs.data(), lens.data(), term.data(), (int)envs.size());
}
// ---- exploration strategies (k_explore)
static int env_explore(ilsx_vecenv* e, float* act, const double* eps, long long t, const double* u = nullptr) {
  const ilsx_explore_cfg& c = e->explore;
  ExploreArgs X;
  X.kind = c.kind; X.n_env = e->n_env; X.a = e->a;
  X.mu = c.mu; X.theta = c.theta; X.max_sigma = c.max_sigma; X.min_sigma = c.min_sigma; X.decay_period = c.decay_period;
  X.low = c.low; X.high = c.high; X.t = t; X.epsilon = c.kind == 1 ? e->explore_eps : 0.0;
  const int tot = e->n_env * e->a;
  hipLaunchKernelGGL(k_explore, dim3((tot + 255) / 256), dim3(256), 0, e->ctx->stream, X, act, eps, u, e->ou_state, e->ou_sigma, (const int*)e->ep_len,
                     e->seed, e->rng_stream ^ 0x45585000u, ++e->explore_calls);   // 'EXP': a Philox stream of its own
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_set_exploration(ilsx_vecenv* e, const ilsx_explore_cfg* cfg) {
  if (!e || !cfg) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_set_exploration: NULL argument");
  if (cfg->kind < 0 || cfg->kind > 2) ILSX_FAIL(ILSX_ERR_ARG, "exploration kind %d: 0 none, 1 Gaussian, 2 OU", cfg->kind);
  if (cfg->kind && e->discrete_n > 0) ILSX_FAIL(ILSX_ERR_ARG, "exploration strategies add noise to Box actions; this env's action space is Discrete");
  if (cfg->kind && (!(cfg->decay_period > 0.0) || !(cfg->low <= cfg->high))) ILSX_FAIL(ILSX_ERR_ARG, "exploration: decay_period must be > 0 and low <= high");
  HIPCHK(hipSetDevice(e->ctx->device));
  e->explore = *cfg;
  e->explore_eps = 0.0;   // a strategy starts without the epsilon branch (ilsx_vecenv_set_exploration_epsilon)
  if (!cfg->kind) return ILSX_OK;
  const size_t n = (size_t)e->n_env * e->a;
  if (!e->ou_state) { ILSX_TRY(e->own.alloc_bytes(&e->ou_state, n * 8)); ILSX_TRY(e->own.alloc_bytes(&e->ou_sigma, n * 8)); }
  std::vector<double> h(n, cfg->mu);   // OUStrategy.__init__: state = mu, sigma = max_sigma
  HIPCHK(hipMemcpyAsync(e->ou_state, h.data(), n * 8, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  h.assign(n, cfg->max_sigma);
  HIPCHK(hipMemcpyAsync(e->ou_sigma, h.data(), n * 8, hipMemcpyHostToDevice, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_set_exploration_t(ilsx_vecenv* e, int64_t t) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_set_exploration_t: NULL env");
  e->explore_t = (long long)t;
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_set_exploration_epsilon(ilsx_vecenv* e, double epsilon) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_set_exploration_epsilon: NULL env");
  if (!(epsilon >= 0.0 && epsilon <= 1.0)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_set_exploration_epsilon: epsilon %g is not in [0, 1]", epsilon);
  if (e->explore.kind != 1) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_vecenv_set_exploration_epsilon: the epsilon branch belongs to the Gaussian strategy (kind 1)");
  e->explore_eps = epsilon;
  return ILSX_OK;
}
extern "C" int ilsx_vecenv_explore_u(ilsx_vecenv* e, float* act, const double* eps, const double* u, int64_t t) {
  if (!e || !act) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_explore_u: NULL argument");
  if (!e->explore.kind) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_vecenv_explore_u: no exploration strategy set (ilsx_vecenv_set_exploration)");
  HIPCHK(hipSetDevice(e->ctx->device));
  return env_explore(e, act, eps, (long long)t, u);
}
extern "C" int ilsx_vecenv_explore(ilsx_vecenv* e, float* act, const double* eps, int64_t t) {
  if (!e || !act) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_vecenv_explore: NULL argument");
  if (!e->explore.kind) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_vecenv_explore: no exploration strategy set (ilsx_vecenv_set_exploration)");
  HIPCHK(hipSetDevice(e->ctx->device));
  return env_explore(e, act, eps, (long long)t);
}

// A policy acts in the env's kind of action space: a categorical or epsilon-greedy policy writes indices (Discrete envs), every other policy writes
// continuous actions (Box envs).  Crossed, either the stepper reads an index as a force or an index lands in a continuous column.
static int env_policy_kind_check(const ilsx_vecenv* e, const ilsx_net* pi, const char* who) {
  if (pi && pi->discrete() != (e->discrete_n > 0))
    ILSX_FAIL(ILSX_ERR_ARG, "%s: a %s policy on an env with a %s action space", who,
              pi->categorical ? "categorical" : pi->egreedy ? "epsilon-greedy" : "continuous",
              e->discrete_n > 0 ? "Discrete" : "Box");
  return ILSX_OK;
}
// The env's policy acts on what the env shows.  A goal env's rows are observation | desired_goal | achieved_goal and its networks take the
// first two segments: the forward reads that prefix of obs_cur in place (row stride o, width in_dim); any other width is refused.
static int env_policy_act(ilsx_vecenv* e, ilsx_net* pi, int deterministic, float* act) {
  if (e->goal_dobs > 0) {
    if (pi->lay.cfg.in_dim != e->goal_dobs + e->goal_dg)
      ILSX_FAIL(ILSX_ERR_ARG, "a goal env's policy reads observation | desired_goal = %d columns, this one takes %d", e->goal_dobs + e->goal_dg,
                pi->lay.cfg.in_dim);
    return policy_act_strided(pi, e->obs_cur, e->o, e->n_env, deterministic, nullptr, act, nullptr);
  }
  return ilsx_policy_act(pi, e->policy_obs(), e->n_env, deterministic, nullptr, act, nullptr);
}
static int rollout_step_impl(ilsx_vecenv* e, ilsx_net* pi, ilsx_net* label_pi, int label_deterministic, ilsx_replay* rb,
                             int max_path_length, int random_actions, int deterministic, int no_terminal, bool defer_paths = false) {
  if (!e || (!pi && !random_actions)) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_step: need a policy or random_actions");
  ILSX_TRY(env_policy_kind_check(e, pi, "ilsx_rollout_step"));
  ILSX_TRY(env_policy_kind_check(e, label_pi, "ilsx_rollout_step_relabel"));
  if (e->paths_pending) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_rollout_step: the previous step was begun with ilsx_rollout_step_begin and never ended (ilsx_rollout_step_end)");
  ilsx_ctx* ctx = e->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  if (rb && (rb->o != e->o || rb->a != e->a)) ILSX_FAIL(ILSX_ERR_ARG, "replay dims (%d,%d) != env dims (%d,%d)", rb->o, rb->a, e->o, e->a);
  if (rb && e->n_env > rb->cap) ILSX_FAIL(ILSX_ERR_ARG, "n_env exceeds the replay capacity");
  // The stepper's fused insert records the env's RAW observations while the policy acts on the normalised ones (policy_obs()).  The reference
  // stores what step() returned, i.e. normalised observations (vecenvs.py:251-257): with a ring, env_norm_record rewrites the two observation
  // segments of the step's records after the stepper.  (A goal env cannot have norm_obs on: ilsx_vecenv_obs_norm refuses it.)
  const bool norm_record = rb && e->norm_obs;
  if (norm_record && e->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_rollout_step: norm_obs=1 with a replay ring is not available for goal envs");
  const unsigned long long step = ++e->step_ctr;
  if (random_actions && e->discrete_n > 0) {   // Discrete(n).sample()
    hipLaunchKernelGGL(k_random_discrete_actions, dim3((e->n_env + 255) / 256), dim3(256), 0, ctx->stream, e->act, e->n_env, e->discrete_n,
                       e->seed, e->rng_stream ^ 0x5A5A5A5Au, step);
    HIPCHK(hipGetLastError());
  } else if (random_actions) {
    const int tot = e->n_env * e->a;
    hipLaunchKernelGGL(k_random_actions, dim3((tot + 255) / 256), dim3(256), 0, ctx->stream, e->act, e->n_env, e->seed,
                       e->rng_stream ^ 0x5A5A5A5Au, step, e->a);
    HIPCHK(hipGetLastError());
  } else {
    ILSX_TRY(env_policy_act(e, pi, deterministic, e->act));
    if (e->explore.kind && !deterministic) ILSX_TRY(env_explore(e, e->act, nullptr, e->explore_t));
  }
  EnvStepArgs A;
  ILSX_TRY(rollout_env_args(e, rb, max_path_length, no_terminal, step, &A));
  if (label_pi) {   // DAgger._handle_step (dagger.py:45-71): the stored action is the expert's for the observation acted on
    if (!e->act_label) ILSX_TRY(e->own.alloc_bytes(&e->act_label, (size_t)e->n_env * e->a * 4));
    ILSX_TRY(env_policy_act(e, label_pi, label_deterministic, e->act_label));
    A.rec_act = e->act_label;
  }
  const bool paths = rb && e->path_mode;
  ILSX_TRY(launch_env_step(e, A));
  if (norm_record) ILSX_TRY(env_norm_record(e, A));   // before finished episodes move from the staging area into the ring
  if (paths) {
    HIPCHK(hipMemcpyAsync(e->flush_host, e->flush_len, (size_t)e->n_env * 4, hipMemcpyDeviceToHost, ctx->stream));
    e->paths_pending = rb;
    if (!defer_paths) ILSX_TRY(rollout_paths_finish(e));
  } else if (rb) {
    ILSX_TRY(replay_advance_device_rows(rb, e->n_env));
  }
  return norm_record ? ILSX_OK : env_after_step_norm(e);
}

extern "C" int ilsx_rollout_step(ilsx_vecenv* e, ilsx_net* pi, ilsx_replay* rb, int max_path_length, int random_actions,
                                 int deterministic, int no_terminal) {
  return rollout_step_impl(e, pi, nullptr, 0, rb, max_path_length, random_actions, deterministic, no_terminal);
}
// The same step in two halves, for a host that advances several runs side by side (each on its own ctx / stream): _begin only ENQUEUES
// (actions, physics, record, and in path mode the read-back of the episode-end flags), _end does what needs the host — in path mode it waits
// for the step and inserts the finished episodes (base_algorithm.py:509-519); otherwise nothing.  begin(all runs) ; end(all runs) lets the
// runs' launches overlap on the GPU instead of serialising on one host wait per run.
extern "C" int ilsx_rollout_step_begin(ilsx_vecenv* e, ilsx_net* pi, ilsx_replay* rb, int max_path_length, int random_actions,
                                       int deterministic, int no_terminal) {
  return rollout_step_impl(e, pi, nullptr, 0, rb, max_path_length, random_actions, deterministic, no_terminal, /*defer_paths=*/true);
}
extern "C" int ilsx_rollout_step_end(ilsx_vecenv* e) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_step_end: NULL env");
  HIPCHK(hipSetDevice(e->ctx->device));
  return rollout_paths_finish(e);
}
// n_steps lock-step sampling iterations of K runs (the inner loop of DeviceRLAlgorithmGroup between two train triggers): per iteration every
// run's step is enqueued on its own stream, then every run's host part is done — K x n_steps x 2 calls through the binding become one.
// Run k acts at random while its ring holds fewer than min_steps_before_training[k] samples (base_algorithm.py:186-188), exactly as the
// per-step form decides it.
// Can the K runs' steps go out as ONE launch per stage?  Planar steppers of one kernel instantiation with the same env count, plain
// observations, policies of one shape (the generic forward takes up to four tasks per launch), everything on one device.
static bool rollout_runs_groupable(ilsx_vecenv* const* envs, ilsx_net* const* pis, int n_runs) {
  if (sw::ILSX_ROLLOUT_NO_GROUP() || n_runs < 2) return false;
  const ilsx_vecenv* e0 = envs[0];
  const ilsx_net* p0 = pis[0];
  if (e0->engine != 0 || e0->ctx->prof_on) return false;
  for (int k = 0; k < n_runs; ++k) {
    const ilsx_vecenv* e = envs[k];
    const ilsx_net* p = pis[k];
    if (e->explore.kind) return false;   // a strategy's kernel runs between inference and the stepper: such runs step one by one
    if (e->engine != 0 || e->norm_obs || e->n_env != e0->n_env || e->hm.nb != e0->hm.nb || (e->hm.max_rows > 12) != (e0->hm.max_rows > 12) ||
        e->o != e0->o || e->a != e0->a || e->ctx->device != e0->ctx->device)
      return false;
    if (memcmp(&p->lay.cfg, &p0->lay.cfg, sizeof p->lay.cfg) || p->noise_policy != p0->noise_policy || p->out_linear != p0->out_linear ||
        (p->lay.cfg.n_heads != 2 && !p->noise_policy) || p->discrete())   // the grouped forward has no categorical / argmax head
      return false;
  }
  return true;
}
template <int NB, int MR>
static int launch_envg_step_runs_t(ilsx_ctx* ctx, const EnvStepGroupArgs& G, int n, int n_env) {
  const size_t lds = (((sizeof(PlanarModelDev) + 7) / 8) + (size_t)EG_ENVS * EgOff<NB, MR>::TOTAL) * sizeof(double);
  hipLaunchKernelGGL((k_envg_step_runs<NB, MR>), dim3((n_env + EG_ENVS - 1) / EG_ENVS, n), dim3(64), lds, ctx->stream, G);
  HIPCHK(hipGetLastError());
  return ILSX_OK;
}
// One lock-step iteration of K groupable runs on ONE stream (run 0's): the runs' actions — policy inference as launches of up to four tasks,
// each task on its run's Philox key and call counter, or uniform draws while a run is still filling its ring —, ONE stepper launch whose grid
// rows are the runs (k_envg_step_runs), the read-back of the episode-end flags with path mode on.  Per run the launches do exactly what its own
// ilsx_rollout_step would do: same arithmetic, same draws.
static int rollout_lockstep_grouped(ilsx_vecenv* const* envs, ilsx_net* const* pis, ilsx_replay* const* rbs, int n_runs, int max_path_length,
                                    const int64_t* min_steps, int deterministic, int no_terminal) {
  ilsx_ctx* gctx = envs[0]->ctx;
  hipStream_t gs = gctx->stream;
  std::vector<int> pol;   // runs that act through their policy this step
  for (int k = 0; k < n_runs; ++k) {
    ilsx_vecenv* e = envs[k];
    if (e->paths_pending) ILSX_FAIL(ILSX_ERR_STATE, "ilsx_rollout_steps_lockstep: run %d has an unfinished step (ilsx_rollout_step_end)", k);
    if (rbs[k]->o != e->o || rbs[k]->a != e->a || e->n_env > rbs[k]->cap) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_steps_lockstep: replay %d does not match its env", k);
    if (rbs[k]->size < min_steps[k]) {
      const int tot = e->n_env * e->a;
      hipLaunchKernelGGL(k_random_actions, dim3((tot + 255) / 256), dim3(256), 0, gs, e->act, e->n_env, e->seed, e->rng_stream ^ 0x5A5A5A5Au,
                         e->step_ctr + 1, e->a);
    } else pol.push_back(k);
  }
  for (size_t i = 0; i < pol.size(); i += 4) {
    FwdArgs A;
    memset(&A, 0, sizeof A);
    const int nt = (int)std::min<size_t>(4, pol.size() - i);
    for (int j = 0; j < nt; ++j) {
      ilsx_vecenv* e = envs[pol[i + j]];
      ilsx_net* pi = pis[pol[i + j]];
      FwdTask& t = A.t[j];
      t.net = net_view(pi->lay, pi->base);
      t.x0 = e->policy_obs(); t.d0 = pi->lay.cfg.in_dim; t.s0 = pi->lay.cfg.in_dim;
      t.head = deterministic ? HEAD_TANH_DET : HEAD_TANH_SAMPLE;
      if (pi->noise_policy) {
        t.head = pi->out_linear ? HEAD_DET_LIN_NOISE : HEAD_DET_TANH_NOISE;
        t.noise = deterministic ? 0.0f : pi->noise; t.noise_clip = pi->noise_clip; t.max_act = pi->max_act;
      }
      t.action = e->act;
      t.rng_stream = 0x41435400u;  // 'ACT' (ilsx_policy_act)
      t.seed_t = pi->ctx->seed; t.step_t = ++pi->ctx->act_calls;   // (>= 1: the task's own key)
    }
    A.rows = envs[0]->n_env; A.ntasks = nt; A.seed = gctx->seed;
    ILSX_TRY(launch_fwd(gctx, A, pis[0]->lay.cfg.hidden, pis[0]->lay.cfg.act, pis[0]->lay.KP));
  }
  ilsx_vecenv* e0m = envs[0];
  bool all_paths = true;
  for (int k = 0; k < n_runs; ++k) all_paths = all_paths && envs[k]->path_mode;
  const int ne = e0m->n_env;
  if (all_paths && e0m->grp_flush_n < n_runs * ne) {   // the group's flag array (owned by run 0's env, freed with it)
    if (e0m->grp_flush_dev) ILSX_TRY(e0m->own.free(e0m->grp_flush_dev));
    if (e0m->grp_flush_host) HIPCHK(hipHostFree(e0m->grp_flush_host));
    e0m->grp_flush_dev = nullptr; e0m->grp_flush_host = nullptr; e0m->grp_flush_n = 0;
    ILSX_TRY(e0m->own.alloc_bytes(&e0m->grp_flush_dev, (size_t)n_runs * ne * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&e0m->grp_flush_host, (size_t)n_runs * ne * sizeof(int), hipHostMallocDefault));
    e0m->grp_flush_n = n_runs * ne;
  }
  for (int k0 = 0; k0 < n_runs; k0 += ENVG_MAX_RUNS) {
    EnvStepGroupArgs G;
    const int n = std::min(ENVG_MAX_RUNS, n_runs - k0);
    for (int j = 0; j < n; ++j) {
      ilsx_vecenv* e = envs[k0 + j];
      ILSX_TRY(rollout_env_args(e, rbs[k0 + j], max_path_length, no_terminal, ++e->step_ctr, &G.a[j]));
      if (all_paths) G.a[j].flush_len = e0m->grp_flush_dev + (size_t)(k0 + j) * ne;
    }
    const ilsx_vecenv* e0 = envs[0];
    if (e0->hm.nb == 4) ILSX_TRY((launch_envg_step_runs_t<4, 8>(gctx, G, n, e0->n_env)));
    else if (e0->hm.max_rows > 12) ILSX_TRY((launch_envg_step_runs_t<7, 16>(gctx, G, n, e0->n_env)));
    else ILSX_TRY((launch_envg_step_runs_t<7, 12>(gctx, G, n, e0->n_env)));
  }
  bool any_paths = false;
  if (all_paths) {
    HIPCHK(hipMemcpyAsync(e0m->grp_flush_host, e0m->grp_flush_dev, (size_t)n_runs * ne * sizeof(int), hipMemcpyDeviceToHost, gs));
    for (int k = 0; k < n_runs; ++k) envs[k]->paths_pending = rbs[k];
    any_paths = true;
  } else {
    for (int k = 0; k < n_runs; ++k) {
      ilsx_vecenv* e = envs[k];
      if (e->path_mode) {
        HIPCHK(hipMemcpyAsync(e->flush_host, e->flush_len, (size_t)e->n_env * 4, hipMemcpyDeviceToHost, gs));
        e->paths_pending = rbs[k];
        any_paths = true;
      } else ILSX_TRY(replay_advance_device_rows(rbs[k], e->n_env));
    }
  }
  if (any_paths) {
    HIPCHK(hipStreamSynchronize(gs));
    for (int k = 0; k < n_runs; ++k)
      ILSX_TRY(rollout_paths_finish(envs[k], /*synced=*/true, all_paths ? e0m->grp_flush_host + (size_t)k * ne : nullptr));
  }
  return ILSX_OK;
}
// n_steps lock-step sampling iterations of K runs (the inner loop of DeviceRLAlgorithmGroup between two train triggers): K x n_steps x 2 calls
// through the binding become one.  Run k acts at random while its ring holds fewer than min_steps_before_training[k] samples
// (base_algorithm.py:186-188), exactly as the per-step form decides it.  Runs of one shape (rollout_runs_groupable: the reference's regime of a
// few envs per run and many seeds) go out as one launch per stage on run 0's stream; otherwise every run's step is enqueued on its own stream
// and then every run's host part is done.
extern "C" int ilsx_rollout_steps_lockstep(ilsx_vecenv* const* envs, ilsx_net* const* pis, ilsx_replay* const* rbs, int n_runs, int n_steps,
                                           int max_path_length, const int64_t* min_steps_before_training, int deterministic, int no_terminal) {
  if (!envs || !pis || !rbs || !min_steps_before_training || n_runs < 1 || n_steps < 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_steps_lockstep: bad argument");
  for (int k = 0; k < n_runs; ++k)
    if (!envs[k] || !pis[k] || !rbs[k]) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_steps_lockstep: run %d has a NULL env / policy / replay", k);
  for (int k = 0; k < n_runs; ++k)
    if (envs[k]->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_rollout_steps_lockstep: run %d is a goal env (grouped seeds are not available for goal envs)", k);
  if (rollout_runs_groupable(envs, pis, n_runs)) {
    HIPCHK(hipSetDevice(envs[0]->ctx->device));
    // everything the runs' own streams still hold (an evaluation, a train call, a ring insert) happens before the grouped launches, and they
    // are complete when this call returns: host waits (an event wait would slow the stream's later graph launches, profiles/r06_grp_streams.txt)
    for (int k = 1; k < n_runs; ++k)
      if (envs[k]->ctx->stream != envs[0]->ctx->stream) HIPCHK(hipStreamSynchronize(envs[k]->ctx->stream));
    for (int t = 0; t < n_steps; ++t)
      ILSX_TRY(rollout_lockstep_grouped(envs, pis, rbs, n_runs, max_path_length, min_steps_before_training, deterministic, no_terminal));
    HIPCHK(hipStreamSynchronize(envs[0]->ctx->stream));
    return ILSX_OK;
  }
  for (int t = 0; t < n_steps; ++t) {
    for (int k = 0; k < n_runs; ++k)
      ILSX_TRY(rollout_step_impl(envs[k], pis[k], nullptr, 0, rbs[k], max_path_length, rbs[k]->size < min_steps_before_training[k] ? 1 : 0,
                                 deterministic, no_terminal, /*defer_paths=*/true));
    for (int k = 0; k < n_runs; ++k) {
      HIPCHK(hipSetDevice(envs[k]->ctx->device));
      ILSX_TRY(rollout_paths_finish(envs[k]));
    }
  }
  return ILSX_OK;
}
extern "C" int ilsx_rollout_step_relabel(ilsx_vecenv* e, ilsx_net* pi, ilsx_net* expert, int expert_deterministic, ilsx_replay* rb,
                                         int max_path_length, int no_terminal) {
  if (!expert) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_rollout_step_relabel: NULL expert policy");
  return rollout_step_impl(e, pi, expert, expert_deterministic, rb, max_path_length, 0, 0, no_terminal);
}

// ---- on-policy rollout into env-major buffers (sample (env, t) lives at row env*T + t)
__global__ void k_onpolicy_record_pre(const float* __restrict__ obs, const float* __restrict__ act, int n_env, int o, int a, int t,
                                      int T, float* __restrict__ obs_buf, float* __restrict__ act_buf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, w = o + a;
  if (i >= n_env * w) return;
  const int env = i / w, j = i - env * w;
  const size_t row = (size_t)env * T + t;
  if (j < o) obs_buf[row * o + j] = obs[(size_t)env * o + j];
  else act_buf[row * a + (j - o)] = act[(size_t)env * a + (j - o)];
}
__global__ void k_onpolicy_record_post(const float* __restrict__ rew, const int* __restrict__ ep_len, int n_env, int t, int T,
                                       float* __restrict__ rew_buf, uint8_t* __restrict__ ends_buf) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_env) return;
  const size_t row = (size_t)env * T + t;
  rew_buf[row] = rew[env];
  ends_buf[row] = ep_len[env] == 0 ? 1 : 0;   // the env was just reset: terminal or time limit
}

// PPO's sampling phase (torch_rl_algorithm.py:30-32 over base_algorithm.py:183-277) for ALL envs on the device: T vec steps
// with the Gaussian policy of `ppo`; env-major buffers obs[n_env*T,o] (what the policy saw: normalised when norm_obs),
// act[n_env*T,a] (un-clipped policy output; the env clips), rew[n_env*T], ends[n_env*T] (1 = episode ended after this
// sample).  last_values[n_env] (nullable) = V(observation after the last step) for bootstrapping unfinished segments.
extern "C" int ilsx_ppo_rollout(ilsx_ppo* ppo, ilsx_vecenv* e, int T, int max_path_length, float* obs, float* act, float* rew,
                                uint8_t* ends, float* last_values) {
  if (!ppo || !e || !obs || !act || !rew || !ends || T < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_ppo_rollout: bad argument");
  if (e->discrete_n > 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_ppo_rollout: PPO's Gaussian policy on an env with a Discrete action space");
  if (e->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_ppo_rollout: not available for goal envs (dictionary observations)");
  ilsx_ctx* ctx = e->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const int n = e->n_env, w = e->o + e->a;
  for (int t = 0; t < T; ++t) {
    const unsigned long long step = ++e->step_ctr;
    ILSX_TRY(ilsx_ppo_policy_act(ppo, e->policy_obs(), n, 0, nullptr, e->act, nullptr));
    hipLaunchKernelGGL(k_onpolicy_record_pre, dim3((n * w + 255) / 256), dim3(256), 0, ctx->stream, e->policy_obs(), (const float*)e->act,
                       n, e->o, e->a, t, T, obs, act);
    EnvStepArgs A;
    memset(&A, 0, sizeof A);
    A.m = e->dm; A.qpos = e->qpos; A.qvel = e->qvel; A.n_env = n;
    A.ids = nullptr; A.n_ids = n; A.act = e->act;
    A.obs = e->nobs; A.rew = e->rew; A.done = e->done;
    A.obs_cur = e->obs_cur; A.auto_reset = 1; A.max_path_length = max_path_length;
    A.ep_len = e->ep_len; A.ep_ret = e->ep_ret; A.stats = e->stats;
    A.seed = e->seed; A.stream = e->rng_stream; A.step = step;
    ILSX_TRY(launch_env_step(e, A));
    hipLaunchKernelGGL(k_onpolicy_record_post, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float*)e->rew,
                       (const int*)e->ep_len, n, t, T, rew, ends);
    HIPCHK(hipGetLastError());
    ILSX_TRY(env_after_step_norm(e));
  }
  if (last_values) ILSX_TRY(ilsx_ppo_values(ppo, e->policy_obs(), n, last_values));
  return ILSX_OK;
}

// ---- evaluation: VecPathSampler.obtain_samples / rollout (samplers/vec_sampler.py:5-93,124-142) on the device.
// Every env plays ONE episode (envs that end are frozen, not reset); the statistics of
// eval_util.get_generic_path_information (:15-80) are accumulated as sums / extrema.
enum { EV_PATHS = 0, EV_STEPS, EV_RET_S, EV_RET_SS, EV_RET_MAX, EV_RET_MIN, EV_LEN_S, EV_LEN_SS, EV_LEN_MAX, EV_LEN_MIN, EV_REW_S,
       EV_REW_SS, EV_REW_MAX, EV_REW_MIN, EV_ACT_S, EV_ACT_SS, EV_ACT_MAX, EV_ACT_MIN, EV_N };
__device__ __forceinline__ void atomic_max_d(double* p, double v) {
  unsigned long long old = __double_as_longlong(*p);
  while (v > __longlong_as_double(old)) {
    const unsigned long long prev = atomicCAS((unsigned long long*)p, old, (unsigned long long)__double_as_longlong(v));
    if (prev == old) break;
    old = prev;
  }
}
__device__ __forceinline__ void atomic_min_d(double* p, double v) {
  unsigned long long old = __double_as_longlong(*p);
  while (v < __longlong_as_double(old)) {
    const unsigned long long prev = atomicCAS((unsigned long long*)p, old, (unsigned long long)__double_as_longlong(v));
    if (prev == old) break;
    old = prev;
  }
}
__global__ void k_eval_begin(unsigned char* frozen, double* ret, int* len, int n, int* alive) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) { frozen[e] = 0; ret[e] = 0.0; len[e] = 0; }
  if (e == 0) *alive = n;
}
__global__ void k_eval_accum(const float* __restrict__ rew, const unsigned char* __restrict__ done, const float* __restrict__ act,
                             int n, int a, int max_path_length, unsigned char* frozen, double* ret, int* len, double* st, int* alive) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n || frozen[e]) return;
  const double r = (double)rew[e];
  const double R = ret[e] + r;
  const int L = len[e] + 1;
  ret[e] = R; len[e] = L;
  atomicAdd(&st[EV_STEPS], 1.0);
  atomicAdd(&st[EV_REW_S], r); atomicAdd(&st[EV_REW_SS], r * r); atomic_max_d(&st[EV_REW_MAX], r); atomic_min_d(&st[EV_REW_MIN], r);
  for (int k = 0; k < a; ++k) {
    const double x = (double)act[(size_t)e * a + k];
    atomicAdd(&st[EV_ACT_S], x); atomicAdd(&st[EV_ACT_SS], x * x); atomic_max_d(&st[EV_ACT_MAX], x); atomic_min_d(&st[EV_ACT_MIN], x);
  }
  if (done[e] || L >= max_path_length) {   // the path ends at its first terminal or at the horizon (vec_sampler.py:61-77)
    frozen[e] = 1;
    atomicAdd(&st[EV_PATHS], 1.0);
    atomicAdd(&st[EV_RET_S], R); atomicAdd(&st[EV_RET_SS], R * R); atomic_max_d(&st[EV_RET_MAX], R); atomic_min_d(&st[EV_RET_MIN], R);
    const double l = (double)L;
    atomicAdd(&st[EV_LEN_S], l); atomicAdd(&st[EV_LEN_SS], l * l); atomic_max_d(&st[EV_LEN_MAX], l); atomic_min_d(&st[EV_LEN_MIN], l);
    atomicSub(alive, 1);
  }
}

static int eval_buffers(ilsx_vecenv* e) {   // allocated by the env's first evaluation rollout
  if (e->ev_frozen) return ILSX_OK;
  const int n = e->n_env;
  ILSX_TRY(e->own.alloc_bytes(&e->ev_frozen, n)); ILSX_TRY(e->own.alloc_bytes(&e->ev_ret, (size_t)n * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->ev_len, (size_t)n * 4)); ILSX_TRY(e->own.alloc_bytes(&e->ev_stats, EV_N * 8));
  ILSX_TRY(e->own.alloc_bytes(&e->ev_alive, 4));
  return ILSX_OK;
}

extern "C" int ilsx_eval_rollout(ilsx_vecenv* e, ilsx_net* pi, ilsx_ppo* ppo, int max_path_length, int deterministic, int reset_stats,
                                 double* stats_host) {
  if (!e || (!pi && !ppo) || max_path_length < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_eval_rollout: bad argument");
  ILSX_TRY(env_policy_kind_check(e, pi, "ilsx_eval_rollout"));
  if (!pi && e->discrete_n > 0) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_eval_rollout: PPO's Gaussian policy on an env with a Discrete action space");
  if (!pi && e->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_eval_rollout: PPO's policy on a goal env (dictionary observations)");
  ilsx_ctx* ctx = e->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const int n = e->n_env;
  if (!e->ev_frozen) {
    ILSX_TRY(eval_buffers(e));
    reset_stats = 1;
  }
  hipStream_t st = ctx->stream;
  if (reset_stats) {
    double h[EV_N];
    for (int i = 0; i < EV_N; ++i) h[i] = 0.0;
    h[EV_RET_MAX] = h[EV_LEN_MAX] = h[EV_REW_MAX] = h[EV_ACT_MAX] = -INFINITY;
    h[EV_RET_MIN] = h[EV_LEN_MIN] = h[EV_REW_MIN] = h[EV_ACT_MIN] = INFINITY;
    HIPCHK(hipMemcpyAsync(e->ev_stats, h, sizeof h, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  ILSX_TRY(ilsx_vecenv_reset(e, nullptr, n, nullptr));   // rollout() starts with env.reset(ready_env_ids) (vec_sampler.py:33)
  hipLaunchKernelGGL(k_eval_begin, dim3((n + 255) / 256), dim3(256), 0, st, e->ev_frozen, e->ev_ret, e->ev_len, n, e->ev_alive);
  for (int t = 0; t < max_path_length; ++t) {
    const unsigned long long step = ++e->step_ctr;
    if (pi) ILSX_TRY(env_policy_act(e, pi, deterministic, e->act));
    else ILSX_TRY(ilsx_ppo_policy_act(ppo, e->policy_obs(), n, deterministic, nullptr, e->act, nullptr));
    EnvStepArgs A;
    memset(&A, 0, sizeof A);
    A.m = e->dm; A.qpos = e->qpos; A.qvel = e->qvel; A.n_env = n;
    A.ids = nullptr; A.n_ids = n; A.act = e->act;
    A.obs = e->nobs; A.rew = e->rew; A.done = e->done; A.obs_cur = e->obs_cur; A.frozen = e->ev_frozen;
    A.seed = e->seed; A.stream = e->rng_stream; A.step = step;
    ILSX_TRY(launch_env_step(e, A));
    hipLaunchKernelGGL(k_eval_accum, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)e->rew, (const unsigned char*)e->done,
                       (const float*)e->act, n, e->a, max_path_length, e->ev_frozen, e->ev_ret, e->ev_len, e->ev_stats, e->ev_alive);
    HIPCHK(hipGetLastError());
    if (e->norm_obs) {   // step() hands out normalised observations and (training envs only) feeds the statistics
      ILSX_TRY(env_obs_norm(e, e->nobs, n, nullptr, nullptr, nullptr, 0));
      ILSX_TRY(env_obs_norm(e, nullptr, 0, nullptr, e->obs_cur, e->obs_n, n));
    }
    if ((t & 31) == 31) {   // every env done? (one 4-byte read-back per 32 vec steps)
      int alive = 0;
      HIPCHK(hipMemcpyAsync(&alive, e->ev_alive, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (alive <= 0) break;
    }
  }
  if (stats_host) {
    HIPCHK(hipMemcpyAsync(stats_host, e->ev_stats, EV_N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return ILSX_OK;
}

// ---- the evaluation rollouts of K runs in lock-step (DeviceRLAlgorithmGroup: K small eval envs, one per run)
struct EvalAccumRun { const float* rew; const unsigned char* done; const float* act; unsigned char* frozen; double* ret; int* len; double* st; int* alive; };
struct EvalAccumRuns { EvalAccumRun r[ENVG_MAX_RUNS]; int n, a, max_path_length; };
__global__ void k_eval_accum_runs(const EvalAccumRuns G) {   // blockIdx.y = run; a row of the grid is that run's k_eval_accum launch
  const EvalAccumRun& R = G.r[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= G.n || R.frozen[e]) return;
  const double r = (double)R.rew[e];
  const double Rt = R.ret[e] + r;
  const int L = R.len[e] + 1;
  R.ret[e] = Rt; R.len[e] = L;
  double* st = R.st;
  atomicAdd(&st[EV_STEPS], 1.0);
  atomicAdd(&st[EV_REW_S], r); atomicAdd(&st[EV_REW_SS], r * r); atomic_max_d(&st[EV_REW_MAX], r); atomic_min_d(&st[EV_REW_MIN], r);
  for (int k = 0; k < G.a; ++k) {
    const double x = (double)R.act[(size_t)e * G.a + k];
    atomicAdd(&st[EV_ACT_S], x); atomicAdd(&st[EV_ACT_SS], x * x); atomic_max_d(&st[EV_ACT_MAX], x); atomic_min_d(&st[EV_ACT_MIN], x);
  }
  if (R.done[e] || L >= G.max_path_length) {
    R.frozen[e] = 1;
    atomicAdd(&st[EV_PATHS], 1.0);
    atomicAdd(&st[EV_RET_S], Rt); atomicAdd(&st[EV_RET_SS], Rt * Rt); atomic_max_d(&st[EV_RET_MAX], Rt); atomic_min_d(&st[EV_RET_MIN], Rt);
    const double l = (double)L;
    atomicAdd(&st[EV_LEN_S], l); atomicAdd(&st[EV_LEN_SS], l * l); atomic_max_d(&st[EV_LEN_MAX], l); atomic_min_d(&st[EV_LEN_MIN], l);
    atomicSub(R.alive, 1);
  }
}
// VecPathSampler.obtain_samples (vec_sampler.py:126-146) of K runs at once: every run rolls whole rounds (one episode per env, frozen at its
// end) until ITS statistics hold >= num_steps steps; the runs of one shape step in lock-step as one launch per stage on run 0's stream — a run
// leaves a round at the very check (every 32 vec steps) at which its own ilsx_eval_rollout would, so its policy-call counter, env step counter
// and statistics are those of evaluating it alone.  stats_host: [K][18] doubles (the layout ilsx_eval_rollout fills).  ILSX_ERR_UNSUPPORTED when
// the runs cannot share launches (the caller evaluates them one by one).
extern "C" int ilsx_eval_rollouts_lockstep(ilsx_vecenv* const* envs, ilsx_net* const* pis, int n_runs, int max_path_length, int deterministic,
                                           int64_t num_steps, double* stats_host) {
  if (!envs || !pis || !stats_host || n_runs < 1 || max_path_length < 1) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_eval_rollouts_lockstep: bad argument");
  for (int k = 0; k < n_runs; ++k)
    if (!envs[k] || !pis[k]) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_eval_rollouts_lockstep: run %d has a NULL env / policy", k);
  for (int k = 0; k < n_runs; ++k)
    if (envs[k]->goal_dobs > 0) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_eval_rollouts_lockstep: run %d is a goal env (grouped seeds are not available for goal envs)", k);
  if (n_runs > ENVG_MAX_RUNS || !rollout_runs_groupable(envs, pis, n_runs)) ILSX_FAIL(ILSX_ERR_UNSUPPORTED, "ilsx_eval_rollouts_lockstep: the runs cannot share launches");
  ilsx_vecenv* e0 = envs[0];
  ilsx_ctx* gctx = e0->ctx;
  hipStream_t gs = gctx->stream;
  HIPCHK(hipSetDevice(gctx->device));
  const int ne = e0->n_env;
  for (int k = 0; k < n_runs; ++k) {
    ILSX_TRY(eval_buffers(envs[k]));
    if (envs[k]->ctx->stream != gs) HIPCHK(hipStreamSynchronize(envs[k]->ctx->stream));
  }
  if (e0->grp_flush_n < n_runs) {   // the group's small int array (alive counters here, episode-end flags in the training rollouts)
    if (e0->grp_flush_dev) ILSX_TRY(e0->own.free(e0->grp_flush_dev));
    if (e0->grp_flush_host) HIPCHK(hipHostFree(e0->grp_flush_host));
    e0->grp_flush_dev = nullptr; e0->grp_flush_host = nullptr; e0->grp_flush_n = 0;
    const int cnt = std::max(n_runs, n_runs * ne);
    ILSX_TRY(e0->own.alloc_bytes(&e0->grp_flush_dev, (size_t)cnt * sizeof(int)));
    HIPCHK(hipHostMalloc((void**)&e0->grp_flush_host, (size_t)cnt * sizeof(int), hipHostMallocDefault));
    e0->grp_flush_n = cnt;
  }
  int* alive_dev = e0->grp_flush_dev;
  int* alive_host = e0->grp_flush_host;
  std::vector<int> active(n_runs);
  for (int k = 0; k < n_runs; ++k) active[k] = k;
  {   // fresh statistics for every run
    double h[EV_N];
    for (int i = 0; i < EV_N; ++i) h[i] = 0.0;
    h[EV_RET_MAX] = h[EV_LEN_MAX] = h[EV_REW_MAX] = h[EV_ACT_MAX] = -INFINITY;
    h[EV_RET_MIN] = h[EV_LEN_MIN] = h[EV_REW_MIN] = h[EV_ACT_MIN] = INFINITY;
    for (int k = 0; k < n_runs; ++k) HIPCHK(hipMemcpyAsync(envs[k]->ev_stats, h, sizeof h, hipMemcpyHostToDevice, gs));
    HIPCHK(hipStreamSynchronize(gs));
  }
  while (!active.empty()) {
    for (int k : active) {   // rollout() starts with env.reset(ready_env_ids) (vec_sampler.py:33): on the run's own stream, waited for below
      ilsx_vecenv* e = envs[k];
      ILSX_TRY(ilsx_vecenv_reset(e, nullptr, e->n_env, nullptr));
      if (e->ctx->stream != gs) HIPCHK(hipStreamSynchronize(e->ctx->stream));
      hipLaunchKernelGGL(k_eval_begin, dim3((ne + 255) / 256), dim3(256), 0, gs, e->ev_frozen, e->ev_ret, e->ev_len, ne, alive_dev + k);
    }
    std::vector<int> live = active;
    for (int t = 0; t < max_path_length && !live.empty(); ++t) {
      for (size_t i = 0; i < live.size(); i += 4) {
        FwdArgs A;
        memset(&A, 0, sizeof A);
        const int nt = (int)std::min<size_t>(4, live.size() - i);
        for (int j = 0; j < nt; ++j) {
          ilsx_vecenv* e = envs[live[i + j]];
          ilsx_net* pi = pis[live[i + j]];
          FwdTask& ft = A.t[j];
          ft.net = net_view(pi->lay, pi->base);
          ft.x0 = e->policy_obs(); ft.d0 = pi->lay.cfg.in_dim; ft.s0 = pi->lay.cfg.in_dim;
          ft.head = deterministic ? HEAD_TANH_DET : HEAD_TANH_SAMPLE;
          if (pi->noise_policy) {
            ft.head = pi->out_linear ? HEAD_DET_LIN_NOISE : HEAD_DET_TANH_NOISE;
            ft.noise = deterministic ? 0.0f : pi->noise; ft.noise_clip = pi->noise_clip; ft.max_act = pi->max_act;
          }
          ft.action = e->act;
          ft.rng_stream = 0x41435400u;
          ft.seed_t = pi->ctx->seed; ft.step_t = ++pi->ctx->act_calls;
        }
        A.rows = ne; A.ntasks = nt; A.seed = gctx->seed;
        ILSX_TRY(launch_fwd(gctx, A, pis[0]->lay.cfg.hidden, pis[0]->lay.cfg.act, pis[0]->lay.KP));
      }
      EnvStepGroupArgs G;
      EvalAccumRuns Q;
      memset(&Q, 0, sizeof Q);
      Q.n = ne; Q.a = e0->a; Q.max_path_length = max_path_length;
      const int n = (int)live.size();
      for (int j = 0; j < n; ++j) {
        ilsx_vecenv* e = envs[live[j]];
        EnvStepArgs& A = G.a[j];
        memset(&A, 0, sizeof A);
        A.m = e->dm; A.qpos = e->qpos; A.qvel = e->qvel; A.n_env = ne;
        A.ids = nullptr; A.n_ids = ne; A.act = e->act;
        A.obs = e->nobs; A.rew = e->rew; A.done = e->done; A.obs_cur = e->obs_cur; A.frozen = e->ev_frozen;
        A.seed = e->seed; A.stream = e->rng_stream; A.step = ++e->step_ctr;
        Q.r[j] = EvalAccumRun{e->rew, e->done, e->act, e->ev_frozen, e->ev_ret, e->ev_len, e->ev_stats, alive_dev + live[j]};
      }
      if (e0->hm.nb == 4) ILSX_TRY((launch_envg_step_runs_t<4, 8>(gctx, G, n, ne)));
      else if (e0->hm.max_rows > 12) ILSX_TRY((launch_envg_step_runs_t<7, 16>(gctx, G, n, ne)));
      else ILSX_TRY((launch_envg_step_runs_t<7, 12>(gctx, G, n, ne)));
      hipLaunchKernelGGL(k_eval_accum_runs, dim3((ne + 255) / 256, n), dim3(256), 0, gs, Q);
      HIPCHK(hipGetLastError());
      if ((t & 31) == 31) {   // every env of a run done? (ilsx_eval_rollout's check, for all runs in one read-back)
        HIPCHK(hipMemcpyAsync(alive_host, alive_dev, (size_t)n_runs * sizeof(int), hipMemcpyDeviceToHost, gs));
        HIPCHK(hipStreamSynchronize(gs));
        std::vector<int> still;
        for (int k : live) if (alive_host[k] > 0) still.push_back(k);
        live.swap(still);
      }
    }
    for (int k : active) HIPCHK(hipMemcpyAsync(stats_host + (size_t)k * EV_N, envs[k]->ev_stats, EV_N * 8, hipMemcpyDeviceToHost, gs));
    HIPCHK(hipStreamSynchronize(gs));
    std::vector<int> more;
    for (int k : active) if (stats_host[(size_t)k * EV_N + EV_STEPS] < (double)num_steps) more.push_back(k);
    active.swap(more);
  }
  return ILSX_OK;
}

extern "C" int ilsx_rollout_stats(ilsx_vecenv* e, double* episodes, double* return_sum, int reset) {
  if (!e) ILSX_FAIL(ILSX_ERR_ARG, "env is NULL");
  HIPCHK(hipSetDevice(e->ctx->device));
  double h[4];
  HIPCHK(hipMemcpyAsync(h, e->stats, sizeof h, hipMemcpyDeviceToHost, e->ctx->stream));
  HIPCHK(hipStreamSynchronize(e->ctx->stream));
  if (episodes) *episodes = h[0];
  if (return_sum) *return_sum = h[1];
  if (reset) HIPCHK(hipMemsetAsync(e->stats, 0, sizeof h, e->ctx->stream));
  return ILSX_OK;
}

extern "C" int ilsx_debug_ctx_allocs(ilsx_ctx* ctx, size_t* count) {
  if (!ctx || !count) ILSX_FAIL(ILSX_ERR_ARG, "ilsx_debug_ctx_allocs: NULL argument");
  *count = ctx->allocs.size();
  return ILSX_OK;
}
