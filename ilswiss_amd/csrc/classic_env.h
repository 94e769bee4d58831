// classic_env.h — classic-control engine of ilsx_vecenv (engine 2), included by ilsx_env.hip after EnvStepArgs / env_uniform.
//
// CartPole: gym 0.22's closed-form CartPoleEnv (gym/envs/classic_control/cartpole.py, which rlkit/envs/envs_dict.py:2 maps `cartpole`
// to): Euler integration of the cart-pole equations, float64 throughout in gym's order and constants (the Makefile keeps FMA contraction
// off, so every product and sum rounds as Python's does).  One lane per env; the state (x, x_dot, theta, theta_dot) sits in qpos = (x,
// theta), qvel = (x_dot, theta_dot), SoA like the planar engine.  The action is a float holding the index (1-wide action column, the
// reference's get_dim(Discrete) == 1, env_replay_buffer.py:40): 1 pushes right, anything else left.  Reward 1.0 on every step including the
// one that ends the episode (steps_beyond_done is None then); the observation is the float32 cast of the state.
//
// Pendulum: gym 0.22's PendulumEnv (gym/envs/classic_control/pendulum.py, envs_dict.py `pendulum`) behind the reference's NormalizedBoxEnv
// (rlkit/envs/wrappers.py:342-346), which every training script wraps Box envs in and which is folded into the stepper here as it is for
// the MuJoCo tasks.  Box(-1, 1) actions of width 1; qpos = (theta), qvel = (theta_dot), float64; theta is never wrapped in the state.
// Never done (the reference builds PendulumEnv directly, with no TimeLimit): max_path_length ends episodes.
#pragma once

enum { CLASSIC_CARTPOLE = 0, CLASSIC_PENDULUM = 1 };

struct CartPoleC {
  static constexpr double gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5, force_mag = 10.0, tau = 0.02;
  static constexpr double x_threshold = 2.4;
};

__device__ __forceinline__ void cartpole_write_obs(double x, double xd, double th, double thd, float* dst) {
  dst[0] = (float)x; dst[1] = (float)xd; dst[2] = (float)th; dst[3] = (float)thd;
}

// reset(): np_random.uniform(low=-0.05, high=0.05, size=(4,)) — component k from counter k of the env's Philox stream
__device__ __forceinline__ void cartpole_reset_state(uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, double (&s)[4]) {
  s[0] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 0);
  s[1] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 1);
  s[2] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 2);
  s[3] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 3);
}

__global__ __launch_bounds__(256) void k_cartpole_step(const EnvStepArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_ids) return;
  const int env = A.ids ? A.ids[t] : t;
  if (A.frozen && A.frozen[env]) return;
  const size_t ne = (size_t)A.n_env;
  double x = A.qpos[env], th = A.qpos[ne + env], xd = A.qvel[env], thd = A.qvel[ne + env];
  float obs_before[4];
  if (A.replay) cartpole_write_obs(x, xd, th, thd, obs_before);
  const float av = A.act[t];
  // cartpole.py step(): constants derived exactly as __init__ derives them
  const double total_mass = CartPoleC::masspole + CartPoleC::masscart;
  const double polemass_length = CartPoleC::masspole * CartPoleC::length;
  const double theta_threshold = 12.0 * 2.0 * 3.141592653589793 / 360.0;
  const double force = av == 1.0f ? CartPoleC::force_mag : -CartPoleC::force_mag;
  const double costheta = cos(th), sintheta = sin(th);
  const double temp = (force + polemass_length * (thd * thd) * sintheta) / total_mass;
  const double thetaacc = (CartPoleC::gravity * sintheta - costheta * temp) /
                          (CartPoleC::length * (4.0 / 3.0 - CartPoleC::masspole * (costheta * costheta) / total_mass));
  const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
  x = x + CartPoleC::tau * xd;
  xd = xd + CartPoleC::tau * xacc;
  th = th + CartPoleC::tau * thd;
  thd = thd + CartPoleC::tau * thetaacc;
  const bool done = x < -CartPoleC::x_threshold || x > CartPoleC::x_threshold || th < -theta_threshold || th > theta_threshold;
  const double reward = 1.0;
  float ob[4];
  cartpole_write_obs(x, xd, th, thd, ob);
  if (A.obs) for (int i = 0; i < 4; ++i) A.obs[(size_t)t * 4 + i] = ob[i];
  if (A.rew) A.rew[t] = (float)reward;
  if (A.done) A.done[t] = done ? 1 : 0;
  if (A.replay) {   // fused replay insert (k_env_step's record layout with a 1-wide action column)
    long long slot = A.top + env;
    if (slot >= A.cap) slot -= A.cap;
    float* rec = A.stage ? A.stage + ((size_t)env * A.stage_len + A.ep_len[env]) * A.rec : A.replay + (size_t)slot * A.rec;
    for (int i = 0; i < 4; ++i) rec[i] = obs_before[i];
    rec[4] = A.rec_act ? A.rec_act[t] : av;
    rec[5] = (float)reward;
    rec[6] = (done && !A.no_terminal) ? 1.0f : 0.0f;
    for (int i = 0; i < 4; ++i) rec[7 + i] = ob[i];
    rec[11] = 0.0f; rec[12] = 0.0f;   // absorbing = [0, 0]
  }
  if (A.auto_reset) {
    const int len = A.ep_len[env] + 1;
    const double ret = A.ep_ret[env] + reward;
    const bool finite = isfinite(x) && isfinite(xd) && isfinite(th) && isfinite(thd);
    const bool end = (done && !A.no_terminal) || len >= A.max_path_length || !finite;   // as k_env_step
    if (end) {
      atomicAdd(&A.stats[0], 1.0);
      atomicAdd(&A.stats[1], ret);
      double s[4];
      cartpole_reset_state(A.seed, A.stream, A.step, (uint32_t)env, s);
      x = s[0]; xd = s[1]; th = s[2]; thd = s[3];
      cartpole_write_obs(x, xd, th, thd, ob);
    }
    A.ep_len[env] = end ? 0 : len;
    A.ep_ret[env] = end ? 0.0 : ret;
    if (A.flush_len) A.flush_len[env] = end ? (len | ((done && !A.no_terminal) ? (1 << 30) : 0)) : 0;
  }
  if (A.obs_cur) for (int i = 0; i < 4; ++i) A.obs_cur[(size_t)env * 4 + i] = ob[i];
  A.qpos[env] = x; A.qpos[ne + env] = th; A.qvel[env] = xd; A.qvel[ne + env] = thd;
}

__global__ __launch_bounds__(256) void k_cartpole_reset(double* qpos, double* qvel, int n_env, const int* ids, int n_ids, float* obs,
                                                       float* obs_cur, int* ep_len, double* ep_ret, uint64_t seed, uint32_t stream,
                                                       unsigned long long step) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_ids) return;
  const int env = ids ? ids[t] : t;
  double s[4];
  cartpole_reset_state(seed, stream, step, (uint32_t)env, s);
  float ob[4];
  cartpole_write_obs(s[0], s[1], s[2], s[3], ob);
  for (int i = 0; i < 4; ++i) {
    if (obs) obs[(size_t)t * 4 + i] = ob[i];
    if (obs_cur) obs_cur[(size_t)env * 4 + i] = ob[i];
  }
  ep_len[env] = 0; ep_ret[env] = 0.0;
  const size_t ne = (size_t)n_env;
  qpos[env] = s[0]; qpos[ne + env] = s[2]; qvel[env] = s[1]; qvel[ne + env] = s[3];
}

// env.action_space.sample() of a Discrete(n) space per env while the replay is short (base_algorithm.py:369-380): a uniform index in
// [0, n) as a float, one Philox draw per env (floor(u * n) with u in (0, 1); u * n < n for every u the draw can take, n <= 2^20)
__global__ __launch_bounds__(256) void k_random_discrete_actions(float* act, int n_env, int n_act, uint64_t seed, uint32_t stream,
                                                                unsigned long long step) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_env) return;
  const int k = (int)floor(env_uniform(seed, stream, step, (uint32_t)t, 0) * (double)n_act);
  act[t] = (float)(k < n_act ? k : n_act - 1);
}

// ------------------------------------------------------------------------------------------------ Pendulum
struct PendulumC {
  static constexpr double max_speed = 8.0, dt = 0.05;
  static constexpr double k_sin = 15.0, k_u = 3.0;   // 3 g / (2 l) and 3 / (m l^2) with g = 10, m = l = 1: exact in float64
  static constexpr double two_pi = 2.0 * 3.141592653589793, pi = 3.141592653589793;
};

// NormalizedBoxEnv.step as numpy evaluates it on float32 arrays (lb = -2, ub = 2): lb + (a + 1.0) * 0.5 * (ub - lb), each operation
// rounded to float32, then np.clip to [lb, ub] (which is also PendulumEnv's own clip to +-max_torque).  The comparisons keep a NaN a NaN,
// as np.clip does.
__device__ __forceinline__ float pendulum_torque(float a) {
  const float t = ((a + 1.0f) * 0.5f) * 4.0f;
  const float s = -2.0f + t;
  return s < -2.0f ? -2.0f : (s > 2.0f ? 2.0f : s);
}

// angle_normalize(x) = ((x + pi) % (2 pi)) - pi with numpy's float64 %: r = fmod(x, 2 pi) (exact), r += 2 pi when r < 0, and a zero
// remainder is +0.0 (npy_divmod's copysign(0, b))
__device__ __forceinline__ double pendulum_angle_normalize(double x) {
  double r = fmod(x + PendulumC::pi, PendulumC::two_pi);
  if (r < 0.0) r += PendulumC::two_pi;
  else if (r == 0.0) r = 0.0;
  return r - PendulumC::pi;
}

__device__ __forceinline__ void pendulum_write_obs(double th, double thd, float* dst) {   // _get_obs(): float32 (cos, sin, theta_dot)
  dst[0] = (float)cos(th); dst[1] = (float)sin(th); dst[2] = (float)thd;
}

// reset(): np_random.uniform(low=-[pi, 1], high=[pi, 1]) = low + (high - low) * u — component k from counter k of the env's Philox stream
__device__ __forceinline__ void pendulum_reset_state(uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, double& th,
                                                     double& thd) {
  th = -PendulumC::pi + PendulumC::two_pi * env_uniform(seed, stream, step, env, 0);
  thd = -1.0 + 2.0 * env_uniform(seed, stream, step, env, 1);
}

__global__ __launch_bounds__(256) void k_pendulum_step(const EnvStepArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_ids) return;
  const int env = A.ids ? A.ids[t] : t;
  if (A.frozen && A.frozen[env]) return;
  double th = A.qpos[env], thd = A.qvel[env];
  float obs_before[3];
  if (A.replay) pendulum_write_obs(th, thd, obs_before);
  const float av = A.act[t];
  const double u = (double)pendulum_torque(av);
  // cost in float64 with u promoted exactly, summed left to right.  Had numpy rounded u**2 to float32 (a float32 scalar to an integer
  // power), the cost would move by < 3e-10: below the resolution of the float32 reward that is stored.
  const double an = pendulum_angle_normalize(th);
  const double cost = an * an + 0.1 * (thd * thd) + 0.001 * (u * u);
  const double reward = -cost;
  // gym 0.22's order: the velocity is clipped BEFORE the position update (0.21 clipped afterwards and wrote -sin(theta + pi))
  thd = thd + (PendulumC::k_sin * sin(th) + PendulumC::k_u * u) * PendulumC::dt;
  thd = thd < -PendulumC::max_speed ? -PendulumC::max_speed : (thd > PendulumC::max_speed ? PendulumC::max_speed : thd);
  th = th + thd * PendulumC::dt;
  const bool done = false;
  float ob[3];
  pendulum_write_obs(th, thd, ob);
  if (A.obs) for (int i = 0; i < 3; ++i) A.obs[(size_t)t * 3 + i] = ob[i];
  if (A.rew) A.rew[t] = (float)reward;
  if (A.done) A.done[t] = 0;
  if (A.replay) {   // fused replay insert (k_env_step's record layout: obs | act | rew | done | next_obs | absorbing[2]); the unmapped action
    long long slot = A.top + env;
    if (slot >= A.cap) slot -= A.cap;
    float* rec = A.stage ? A.stage + ((size_t)env * A.stage_len + A.ep_len[env]) * A.rec : A.replay + (size_t)slot * A.rec;
    for (int i = 0; i < 3; ++i) rec[i] = obs_before[i];
    rec[3] = A.rec_act ? A.rec_act[t] : av;
    rec[4] = (float)reward;
    rec[5] = 0.0f;
    for (int i = 0; i < 3; ++i) rec[6 + i] = ob[i];
    rec[9] = 0.0f; rec[10] = 0.0f;   // absorbing = [0, 0]
  }
  if (A.auto_reset) {
    const int len = A.ep_len[env] + 1;
    const double ret = A.ep_ret[env] + reward;
    const bool finite = isfinite(th) && isfinite(thd);
    const bool end = (done && !A.no_terminal) || len >= A.max_path_length || !finite;   // as k_env_step
    if (end) {
      atomicAdd(&A.stats[0], 1.0);
      atomicAdd(&A.stats[1], ret);
      pendulum_reset_state(A.seed, A.stream, A.step, (uint32_t)env, th, thd);
      pendulum_write_obs(th, thd, ob);
    }
    A.ep_len[env] = end ? 0 : len;
    A.ep_ret[env] = end ? 0.0 : ret;
    if (A.flush_len) A.flush_len[env] = end ? len : 0;   // never terminal
  }
  if (A.obs_cur) for (int i = 0; i < 3; ++i) A.obs_cur[(size_t)env * 3 + i] = ob[i];
  A.qpos[env] = th; A.qvel[env] = thd;
}

__global__ __launch_bounds__(256) void k_pendulum_reset(double* qpos, double* qvel, const int* ids, int n_ids, float* obs, float* obs_cur,
                                                        int* ep_len, double* ep_ret, uint64_t seed, uint32_t stream, unsigned long long step) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_ids) return;
  const int env = ids ? ids[t] : t;
  double th, thd;
  pendulum_reset_state(seed, stream, step, (uint32_t)env, th, thd);
  float ob[3];
  pendulum_write_obs(th, thd, ob);
  for (int i = 0; i < 3; ++i) {
    if (obs) obs[(size_t)t * 3 + i] = ob[i];
    if (obs_cur) obs_cur[(size_t)env * 3 + i] = ob[i];
  }
  ep_len[env] = 0; ep_ret[env] = 0.0;
  qpos[env] = th; qvel[env] = thd;
}
