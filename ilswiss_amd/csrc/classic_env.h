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
//
// InvertedPendulum / InvertedDoublePendulum: gym 0.22's task rules (envs_dict.py `invertedpendulum` / `inverteddoublependulum`) on this
// repository's own cart-and-poles dynamics (k_cartchain_step below).
//
// MountainCarContinuous / MountainCar / Acrobot: gym 0.22's closed-form Continuous_MountainCarEnv, MountainCarEnv and AcrobotEnv
// (envs_dict.py `mountaincarcont`; gym's other two closed-form Discrete(3) tasks), operation for operation in float64 as CartPole and
// Pendulum are; at the end of this file, DESIGN.md section 24.
#pragma once

enum { CLASSIC_CARTPOLE = 0, CLASSIC_PENDULUM = 1, CLASSIC_INVERTED_PENDULUM = 2, CLASSIC_INVERTED_DOUBLE_PENDULUM = 3,
       CLASSIC_MOUNTAINCAR_CONT = 4, CLASSIC_MOUNTAINCAR = 5, CLASSIC_ACROBOT = 6 };

// ------------------------------------------------------------------------------------------------ the lane-per-env frame
// One lane per env, one frame for every task of this engine (and for swimmer_env.h): the rollout protocol is written once here and a task
// type supplies what differs —
//   NQ, NV, O, NA      sizes of qpos, qvel, the observation and the action row
//   Model              constants passed to the kernel by value (empty for CartPole and Pendulum)
//   State              q[NQ], v[NV] and whatever else the task carries from the dynamics to the observation
//   reset_state        the draws of reset_model() from the env's Philox stream
//   write_obs          _get_obs(): a function of the state (and the model's constants)
//   obs_before         the observation the record opens with: write_obs, unless the env showed something the state does not hold
//   advance            one env step: the new state, its reward, done and whether the state is finite
//   step_draws         optional: advance also takes the step's stream coordinates (LaneCoords below), for tasks that draw on every step
//   never_done         the task never reports done: done and the terminal bit of flush_len are constants
// Everything the tail needs from the arguments is turned into per-lane values BEFORE advance (the addresses it stores to, the action the
// record holds, the episode's length): a long dynamics loop then carries them in vector registers, of which there are plenty, instead of
// keeping forty-odd scalar registers of arguments alive across it.
struct LaneResetArgs {
  double *qpos, *qvel;
  int n_env;
  const int* ids;   // nullable, compact indexing of obs as in EnvStepArgs
  int n_ids;
  float *obs, *obs_cur;
  int* ep_len; double* ep_ret;
  uint64_t seed; uint32_t stream; unsigned long long step;
};

// Where a step stands in the env's Philox stream: what env_uniform takes.  A task that draws random numbers on every step declares
// `static constexpr bool step_draws = true` and takes a LaneCoords in advance (before reward); its draws must use counters reset_state
// does not, since an episode that ends is reset at the same coordinates.  Every other task's advance is called as before.
struct LaneCoords { uint64_t seed; uint32_t stream; unsigned long long step; uint32_t env; };
template <class T, class = void>
struct lane_step_draws { static constexpr bool value = false; };
template <class T>
struct lane_step_draws<T, decltype((void)T::step_draws)> { static constexpr bool value = T::step_draws; };

template <class T>
__device__ __forceinline__ void lane_step_frame(const EnvStepArgs& A, const typename T::Model& m) {
  constexpr int NQ = T::NQ, NV = T::NV, O = T::O, NA = T::NA;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_ids) return;
  const int env = A.ids ? A.ids[t] : t;
  if (A.frozen && A.frozen[env]) return;
  const size_t ne = (size_t)A.n_env;
  double* const qp = A.qpos + env;
  double* const vp = A.qvel + env;
  typename T::State s{};
#pragma unroll
  for (int i = 0; i < NQ; ++i) s.q[i] = qp[i * ne];
#pragma unroll
  for (int i = 0; i < NV; ++i) s.v[i] = vp[i * ne];
  float* const obs_p = A.obs ? A.obs + (size_t)t * O : nullptr;
  float* const rew_p = A.rew ? A.rew + t : nullptr;
  unsigned char* const done_p = A.done ? A.done + t : nullptr;
  float* const cur_p = A.obs_cur ? A.obs_cur + (size_t)env * O : nullptr;
  float* rec = nullptr;   // fused replay insert (the planar stepper's record layout: obs | act | rew | done | next_obs | absorbing[2])
  if (A.replay) {
    long long slot = A.top + env;
    if (slot >= A.cap) slot -= A.cap;
    rec = A.stage ? A.stage + ((size_t)env * A.stage_len + A.ep_len[env]) * A.rec : A.replay + (size_t)slot * A.rec;
  }
  float av[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) av[j] = A.act[(size_t)t * NA + j];
  if (rec) {
    float obs_before[O];
    T::obs_before(m, s, cur_p, obs_before);
#pragma unroll
    for (int i = 0; i < O; ++i) rec[i] = obs_before[i];
#pragma unroll
    for (int j = 0; j < NA; ++j) rec[O + j] = A.rec_act ? A.rec_act[(size_t)t * NA + j] : av[j];   // the record holds the unmapped action
  }
  // auto-reset bookkeeping that does not depend on the step: the episode's length and whether it ends at the path limit, the return so far
  int len = 0;
  bool limit = false;
  double ret0 = 0.0;
  int* const len_p = A.ep_len + env;
  double* const ret_p = A.ep_ret + env;
  int* const flush_p = (A.auto_reset && A.flush_len) ? A.flush_len + env : nullptr;
  double* const stats_p = A.stats;
  const bool auto_reset = A.auto_reset != 0, no_terminal = A.no_terminal != 0;
  if (auto_reset) {
    len = *len_p + 1;
    ret0 = *ret_p;
    limit = len >= A.max_path_length;
  }
  double reward;
  bool done, finite;
  if constexpr (lane_step_draws<T>::value) T::advance(m, s, av, LaneCoords{A.seed, A.stream, A.step, (uint32_t)env}, reward, done, finite);
  else T::advance(m, s, av, reward, done, finite);
  const bool terminal = !T::never_done && done && !no_terminal;
  float ob[O];
  T::write_obs(m, s, ob);
  if (obs_p) {
#pragma unroll
    for (int i = 0; i < O; ++i) obs_p[i] = ob[i];
  }
  if (rew_p) *rew_p = (float)reward;
  if (done_p) *done_p = (!T::never_done && done) ? 1 : 0;
  if (rec) {
    rec[O + NA] = (float)reward;
    rec[O + NA + 1] = terminal ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < O; ++i) rec[O + NA + 2 + i] = ob[i];
    rec[2 * O + NA + 2] = 0.0f; rec[2 * O + NA + 3] = 0.0f;   // absorbing = [0, 0]
  }
  if (auto_reset) {
    const double ret = ret0 + reward;
    const bool end = terminal || limit || !finite;   // as envg_step_dev
    if (end) {
      atomicAdd(&stats_p[0], 1.0);
      atomicAdd(&stats_p[1], ret);
      T::reset_state(m, A.seed, A.stream, A.step, (uint32_t)env, s);   // drawn when an episode ends, not on every step
      T::write_obs(m, s, ob);
    }
    *len_p = end ? 0 : len;
    *ret_p = end ? 0.0 : ret;
    if (flush_p) *flush_p = end ? (len | (terminal ? (1 << 30) : 0)) : 0;
  }
  if (cur_p) {
#pragma unroll
    for (int i = 0; i < O; ++i) cur_p[i] = ob[i];
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) qp[i * ne] = s.q[i];
#pragma unroll
  for (int i = 0; i < NV; ++i) vp[i * ne] = s.v[i];
}

template <class T>
__device__ __forceinline__ void lane_reset_frame(const LaneResetArgs& R, const typename T::Model& m) {
  constexpr int NQ = T::NQ, NV = T::NV, O = T::O;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= R.n_ids) return;
  const int env = R.ids ? R.ids[t] : t;
  typename T::State s{};
  T::reset_state(m, R.seed, R.stream, R.step, (uint32_t)env, s);
  float ob[O];
  T::write_obs(m, s, ob);
#pragma unroll
  for (int i = 0; i < O; ++i) {
    if (R.obs) R.obs[(size_t)t * O + i] = ob[i];
    if (R.obs_cur) R.obs_cur[(size_t)env * O + i] = ob[i];
  }
  R.ep_len[env] = 0; R.ep_ret[env] = 0.0;
  const size_t ne = (size_t)R.n_env;
#pragma unroll
  for (int i = 0; i < NQ; ++i) R.qpos[i * ne + env] = s.q[i];
#pragma unroll
  for (int i = 0; i < NV; ++i) R.qvel[i * ne + env] = s.v[i];
}

// What most tasks share: the state is (q, v) and the record opens with the observation of that state
template <int NQ_, int NV_>
struct LaneStateQV { double q[NQ_], v[NV_]; };
struct LaneNoModel {};

// ------------------------------------------------------------------------------------------------ CartPole

struct CartPoleC {
  static constexpr double gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5, force_mag = 10.0, tau = 0.02;
  static constexpr double x_threshold = 2.4;
};

// qpos = (x, theta), qvel = (x_dot, theta_dot)
struct CartPoleTask {
  static constexpr int NQ = 2, NV = 2, O = 4, NA = 1;
  static constexpr bool never_done = false;
  using Model = LaneNoModel;
  using State = LaneStateQV<2, 2>;

  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {
    dst[0] = (float)s.q[0]; dst[1] = (float)s.v[0]; dst[2] = (float)s.q[1]; dst[3] = (float)s.v[1];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset(): np_random.uniform(low=-0.05, high=0.05, size=(4,)) — component k of (x, x_dot, theta, theta_dot) from counter k of the env's
  // Philox stream
  static __device__ __forceinline__ void reset_state(const Model&, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    s.q[0] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 0);
    s.v[0] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 1);
    s.q[1] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 2);
    s.v[1] = -0.05 + 0.1 * env_uniform(seed, stream, step, env, 3);
  }

  static __device__ __forceinline__ void advance(const Model&, State& s, const float (&act)[1], double& reward, bool& done, bool& finite) {
    double x = s.q[0], th = s.q[1], xd = s.v[0], thd = s.v[1];
    // cartpole.py step(): constants derived exactly as __init__ derives them
    const double total_mass = CartPoleC::masspole + CartPoleC::masscart;
    const double polemass_length = CartPoleC::masspole * CartPoleC::length;
    const double theta_threshold = 12.0 * 2.0 * 3.141592653589793 / 360.0;
    const double force = act[0] == 1.0f ? CartPoleC::force_mag : -CartPoleC::force_mag;
    const double costheta = cos(th), sintheta = sin(th);
    const double temp = (force + polemass_length * (thd * thd) * sintheta) / total_mass;
    const double thetaacc = (CartPoleC::gravity * sintheta - costheta * temp) /
                            (CartPoleC::length * (4.0 / 3.0 - CartPoleC::masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    x = x + CartPoleC::tau * xd;
    xd = xd + CartPoleC::tau * xacc;
    th = th + CartPoleC::tau * thd;
    thd = thd + CartPoleC::tau * thetaacc;
    done = x < -CartPoleC::x_threshold || x > CartPoleC::x_threshold || th < -theta_threshold || th > theta_threshold;
    reward = 1.0;   // on every step including the one that ends the episode
    finite = isfinite(x) && isfinite(xd) && isfinite(th) && isfinite(thd);
    s.q[0] = x; s.q[1] = th; s.v[0] = xd; s.v[1] = thd;
  }
};

__global__ __launch_bounds__(256) void k_cartpole_step(const EnvStepArgs A) { lane_step_frame<CartPoleTask>(A, {}); }
__global__ __launch_bounds__(256) void k_cartpole_reset(const LaneResetArgs R) { lane_reset_frame<CartPoleTask>(R, {}); }

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

// qpos = (theta), qvel = (theta_dot)
struct PendulumTask {
  static constexpr int NQ = 1, NV = 1, O = 3, NA = 1;
  static constexpr bool never_done = true;
  using Model = LaneNoModel;
  using State = LaneStateQV<1, 1>;

  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {   // _get_obs(): float32 (cos, sin, theta_dot)
    dst[0] = (float)cos(s.q[0]); dst[1] = (float)sin(s.q[0]); dst[2] = (float)s.v[0];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset(): np_random.uniform(low=-[pi, 1], high=[pi, 1]) = low + (high - low) * u — component k from counter k of the env's Philox stream
  static __device__ __forceinline__ void reset_state(const Model&, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    s.q[0] = -PendulumC::pi + PendulumC::two_pi * env_uniform(seed, stream, step, env, 0);
    s.v[0] = -1.0 + 2.0 * env_uniform(seed, stream, step, env, 1);
  }

  static __device__ __forceinline__ void advance(const Model&, State& s, const float (&act)[1], double& reward, bool& done, bool& finite) {
    double th = s.q[0], thd = s.v[0];
    const double u = (double)pendulum_torque(act[0]);
    // cost in float64 with u promoted exactly, summed left to right.  Had numpy rounded u**2 to float32 (a float32 scalar to an integer
    // power), the cost would move by < 3e-10: below the resolution of the float32 reward that is stored.
    const double an = pendulum_angle_normalize(th);
    const double cost = an * an + 0.1 * (thd * thd) + 0.001 * (u * u);
    reward = -cost;
    // gym 0.22's order: the velocity is clipped BEFORE the position update (0.21 clipped afterwards and wrote -sin(theta + pi))
    thd = thd + (PendulumC::k_sin * sin(th) + PendulumC::k_u * u) * PendulumC::dt;
    thd = thd < -PendulumC::max_speed ? -PendulumC::max_speed : (thd > PendulumC::max_speed ? PendulumC::max_speed : thd);
    th = th + thd * PendulumC::dt;
    done = false;
    finite = isfinite(th) && isfinite(thd);
    s.q[0] = th; s.v[0] = thd;
  }
};

__global__ __launch_bounds__(256) void k_pendulum_step(const EnvStepArgs A) { lane_step_frame<PendulumTask>(A, {}); }
__global__ __launch_bounds__(256) void k_pendulum_reset(const LaneResetArgs R) { lane_reset_frame<PendulumTask>(R, {}); }

// ------------------------------------------------------------------------------------------------ cart + chain of poles
// InvertedPendulum (NP = 1) and InvertedDoublePendulum (NP = 2): gym 0.22's task rules on this repository's own rigid-body dynamics, in
// the form of oracle/planar_env.py for another tree — DoF 0 slides the cart along x, DoF k >= 1 is the hinge of pole k:
//   M(q) qdd + c(q, qd) = tau + J^T f,  M = sum_b m_b Jc_b^T Jc_b + I_b Jphi_b^T Jphi_b + diag(armature),
//   tau = gear * ctrl (slide only) - damping * qd,  gravity (0, -g),
// one unilateral soft row per violated joint limit (planar_env.py's impedance / aref / R rule, projected Gauss-Seidel), classic RK4 with
// the constraint solve inside every stage, frame_skip substeps.  M is 2x2 or 3x3: it, its Cholesky factor and the two possible rows
// (DoF 0 and DoF 1) live in registers, every index is a compile-time constant.  The constants come by value as a kernel argument.
struct CartChainDev {
  int frame_skip, pgs_iters, limited[2];
  double mass[3], inertia[3], com[3][2], anchor[3][2], armature[3], damping[3], range[2][2], tip[2];
  double gear, jsign, timestep, gravity, solimp[3], lim_b, lim_k;   // lim_b = 2 / (dmax tc), lim_k = 1 / (dmax^2 tc^2 dr^2)
  float ctrl_lo, ctrl_hi;
};

// NormalizedBoxEnv.step on float32 arrays: lb + (a + 1.0) * 0.5 * (ub - lb), one rounding per operation, then np.clip (a NaN stays a NaN)
__device__ __forceinline__ float cartchain_ctrl(float a, float lb, float ub) {
  const float s = lb + ((a + 1.0f) * 0.5f) * (ub - lb);
  return s < lb ? lb : (s > ub ? ub : s);
}

// x = M^-1 b from the lower Cholesky factor L of M (forward, then backward substitution)
template <int N>
__device__ __forceinline__ void cartchain_chol_solve(const double (&L)[N][N], const double (&b)[N], double (&x)[N]) {
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
}

// qacc = f(q, v, tau0) with the limit rows solved; qfrc = J^T f, the constraint force in joint space
template <int NP>
__device__ void cartchain_dynamics(const CartChainDev& m, const double (&q)[NP + 1], const double (&v)[NP + 1], double tau0,
                                   double (&qacc)[NP + 1], double (&qfrc)[NP + 1]) {
  constexpr int N = NP + 1;
  const double js = m.jsign;
  // ---- kinematics: (jx, jz)[b] = COM Jacobian of pole b + 1 (column j = jsign * perp(lever about hinge j)), jp[b] its angular Jacobian,
  // (fx, fz)[b] = m_b (g - acceleration of the COM at qdd = 0)
  double jx[NP][N], jz[NP][N], jp[NP][N], fx[NP], fz[NP];
  {
    double s1, c1;
    const double w1 = js * v[1];
    sincos(js * q[1], &s1, &c1);
    const double d1x = c1 * m.com[1][0] - s1 * m.com[1][1], d1z = s1 * m.com[1][0] + c1 * m.com[1][1];
    jx[0][0] = 1.0; jz[0][0] = 0.0; jp[0][0] = 0.0;
    jx[0][1] = -js * d1z; jz[0][1] = js * d1x; jp[0][1] = js;
    if constexpr (NP == 2) { jx[0][2] = 0.0; jz[0][2] = 0.0; jp[0][2] = 0.0; }
    // acceleration of the COM at qdd = 0 is -w^2 * lever; force m (g - acc)
    fx[0] = m.mass[1] * (0.0 - (-(w1 * w1) * d1x));
    fz[0] = m.mass[1] * (-m.gravity - (-(w1 * w1) * d1z));
    if constexpr (NP == 2) {
      double s2, c2;
      const double w2 = w1 + js * v[2];
      sincos(js * q[1] + js * q[2], &s2, &c2);
      const double ex = c1 * m.anchor[2][0] - s1 * m.anchor[2][1], ez = s1 * m.anchor[2][0] + c1 * m.anchor[2][1];
      const double d2x = c2 * m.com[2][0] - s2 * m.com[2][1], d2z = s2 * m.com[2][0] + c2 * m.com[2][1];
      jx[1][0] = 1.0; jz[1][0] = 0.0; jp[1][0] = 0.0;
      jx[1][1] = -js * (ez + d2z); jz[1][1] = js * (ex + d2x); jp[1][1] = js;
      jx[1][2] = -js * d2z; jz[1][2] = js * d2x; jp[1][2] = js;
      const double ax = -(w1 * w1) * ex - (w2 * w2) * d2x, az = -(w1 * w1) * ez - (w2 * w2) * d2z;
      fx[1] = m.mass[2] * (0.0 - ax);
      fz[1] = m.mass[2] * (-m.gravity - az);
    }
  }
  // ---- mass matrix (lower triangle) and right-hand side
  double M[N][N], rhs[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rhs[i] = 0.0;
#pragma unroll
    for (int k = 0; k <= i; ++k) M[i][k] = 0.0;
  }
  M[0][0] = m.mass[0];
#pragma unroll
  for (int b = 0; b < NP; ++b) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      rhs[i] += jx[b][i] * fx[b] + jz[b][i] * fz[b];
#pragma unroll
      for (int k = 0; k <= i; ++k) M[i][k] += m.mass[b + 1] * (jx[b][i] * jx[b][k] + jz[b][i] * jz[b][k]) + m.inertia[b + 1] * jp[b][i] * jp[b][k];
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) { M[i][i] += m.armature[i]; rhs[i] -= m.damping[i] * v[i]; }
  rhs[0] += tau0;
  // ---- Cholesky M = L L^T, in place
  double L[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      double s = M[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) s -= L[i][j] * L[k][j];
      L[i][k] = (i == k) ? sqrt(s) : s / L[k][k];
    }
#pragma unroll
    for (int k = i + 1; k < N; ++k) L[i][k] = 0.0;
  }
  double qacc0[N];
  cartchain_chol_solve<N>(L, rhs, qacc0);
  // ---- limit rows: DoF 0, then DoF 1 (J = sg * e_j, r = distance to the limit, negative when violated)
  bool on[2];
  double sg[2], r[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    on[j] = false; sg[j] = 0.0; r[j] = 0.0;
    if (m.limited[j]) {
      if (q[j] - m.range[j][0] < 0.0) { on[j] = true; sg[j] = 1.0; r[j] = q[j] - m.range[j][0]; }
      else if (m.range[j][1] - q[j] < 0.0) { on[j] = true; sg[j] = -1.0; r[j] = m.range[j][1] - q[j]; }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) { qacc[i] = qacc0[i]; qfrc[i] = 0.0; }
  if (!on[0] && !on[1]) return;
  double u[2][N], e[N];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (i == j) ? 1.0 : 0.0;
    cartchain_chol_solve<N>(L, e, u[j]);
  }
  const double a01 = (sg[0] * sg[1]) * u[0][1];
  double den[2], rc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double ajj = u[j][j];
    const double d = impedance_d(fabs(r[j]), m.solimp);
    const double aref = -m.lim_b * (sg[j] * v[j]) - m.lim_k * d * r[j];
    den[j] = ajj + (1.0 - d) / d * ajj;
    rc[j] = aref - sg[j] * qacc0[j];
  }
  double f0 = 0.0, f1 = 0.0;
#pragma unroll 1
  for (int it = 0; it < m.pgs_iters; ++it) {
    if (on[0]) f0 = fmax((rc[0] - a01 * f1) / den[0], 0.0);
    if (on[1]) f1 = fmax((rc[1] - a01 * f0) / den[1], 0.0);
  }
  const double g0 = sg[0] * f0, g1 = sg[1] * f1;
#pragma unroll
  for (int i = 0; i < N; ++i) qacc[i] = qacc0[i] + (u[0][i] * g0 + u[1][i] * g1);
  qfrc[0] = g0; qfrc[1] = g1;
}

// classic RK4 on (q, qd), the planar stepper's form: ONE dynamics call site in a 4-trip loop, sums in the order q + h/6 (k1 + 2 k2 + 2 k3 + k4).
// qfrc is left holding the constraint force of the last stage.
template <int NP>
__device__ __forceinline__ void cartchain_substep(const CartChainDev& m, double (&q)[NP + 1], double (&v)[NP + 1], double tau0,
                                                  double (&qfrc)[NP + 1]) {
  constexpr int N = NP + 1;
  const double h = m.timestep;
  double qs[N], vs[N], qsum[N], vsum[N], a[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { qs[i] = q[i]; vs[i] = v[i]; qsum[i] = 0.0; vsum[i] = 0.0; }
#pragma unroll 1
  for (int stage = 0; stage < 4; ++stage) {
    cartchain_dynamics<NP>(m, qs, vs, tau0, a, qfrc);
    const double w = (stage == 1 || stage == 2) ? 2.0 : 1.0;
    const double ch = (stage == 2) ? h : 0.5 * h;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      qsum[i] = stage == 0 ? vs[i] : qsum[i] + w * vs[i];
      vsum[i] = stage == 0 ? a[i] : vsum[i] + w * a[i];
      const double vn = v[i] + ch * a[i];
      qs[i] = q[i] + ch * vs[i];
      vs[i] = vn;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double qn = q[i] + h / 6.0 * qsum[i];
    const double vn = v[i] + h / 6.0 * vsum[i];
    q[i] = qn; v[i] = vn;
  }
}

__device__ __forceinline__ float cartchain_clip10(double x) { return (float)(x < -10.0 ? -10.0 : (x > 10.0 ? 10.0 : x)); }   // np.clip: NaN stays

template <int NP>
struct CartChainTask {
  static constexpr int N = NP + 1, NQ = N, NV = N, O = NP == 1 ? 4 : 11, NA = 1;
  static constexpr bool never_done = false;
  using Model = CartChainDev;
  struct State { double q[N], v[N], qfrc[N]; };   // qfrc: the constraint force of the step that produced the state (0 after a reset)

  // _get_obs(): InvertedPendulum (qpos | qvel); InvertedDoublePendulum (x, sin th, cos th, clip(qvel, +-10), clip(qfrc_constraint, +-10))
  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {
    if constexpr (NP == 1) {
      dst[0] = (float)s.q[0]; dst[1] = (float)s.q[1]; dst[2] = (float)s.v[0]; dst[3] = (float)s.v[1];
    } else {
      dst[0] = (float)s.q[0];
      dst[1] = (float)sin(s.q[1]); dst[2] = (float)sin(s.q[2]);
      dst[3] = (float)cos(s.q[1]); dst[4] = (float)cos(s.q[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) { dst[5 + i] = cartchain_clip10(s.v[i]); dst[8 + i] = cartchain_clip10(s.qfrc[i]); }
    }
  }
  // the constraint force belongs to the step that produced the state, which (q, v) does not hold: the record opens with the columns the
  // env showed for it (0 after a reset).  They are loaded BEFORE write_obs, whose trigonometry then hides the round trip: the record's
  // first stores wait for them ahead of the dynamics.
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float* obs_cur, float* dst) {
    float shown[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (NP == 2)
      if (obs_cur)
        for (int i = 0; i < 3; ++i) shown[i] = obs_cur[8 + i];
    write_obs(m, s, dst);
    if constexpr (NP == 2)
      if (obs_cur)
        for (int i = 0; i < 3; ++i) dst[8 + i] = shown[i];
  }

  // reset_model(): InvertedPendulum init + U(+-0.01) on qpos and qvel (counters 0..3 of the env's Philox stream); InvertedDoublePendulum
  // qpos = init + U(+-0.1) (counters 0..2), qvel = 0.1 * randn by env_reset_state's Box-Muller draw (counters 3 + 2 i, 4 + 2 i)
  static __device__ __forceinline__ void reset_state(const Model&, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (NP == 1) {
        s.q[i] = -0.01 + 0.02 * env_uniform(seed, stream, step, env, i);
        s.v[i] = -0.01 + 0.02 * env_uniform(seed, stream, step, env, N + i);
      } else {
        s.q[i] = -0.1 + 0.2 * env_uniform(seed, stream, step, env, i);
        const double u1 = env_uniform(seed, stream, step, env, N + 2 * i), u2 = env_uniform(seed, stream, step, env, N + 2 * i + 1);
        s.v[i] = 0.1 * (sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
      }
      s.qfrc[i] = 0.0;
    }
  }

  static __device__ __forceinline__ void advance(const Model& m, State& s, const float (&act)[1], double& reward, bool& done, bool& finite) {
    double (&q)[N] = s.q, (&v)[N] = s.v;
    const double tau0 = m.gear * (double)cartchain_ctrl(act[0], m.ctrl_lo, m.ctrl_hi);
#pragma unroll 1
    for (int k = 0; k < m.frame_skip; ++k) cartchain_substep<NP>(m, q, v, tau0, s.qfrc);
    finite = true;
#pragma unroll
    for (int i = 0; i < N; ++i) finite = finite && isfinite(q[i]) && isfinite(v[i]);
    if constexpr (NP == 1) {
      reward = 1.0;
      done = !finite || fabs(q[1]) > 0.2;
    } else {
      // tip site of pole 2: cart + hinge 2 (pole 1's frame) + site (pole 2's frame)
      const double p1 = m.jsign * q[1], p2 = m.jsign * q[1] + m.jsign * q[2];
      const double s1 = sin(p1), c1 = cos(p1), s2 = sin(p2), c2 = cos(p2);
      const double xt = q[0] + (c1 * m.anchor[2][0] - s1 * m.anchor[2][1]) + (c2 * m.tip[0] - s2 * m.tip[1]);
      const double yt = (s1 * m.anchor[2][0] + c1 * m.anchor[2][1]) + (s2 * m.tip[0] + c2 * m.tip[1]);
      const double dist_penalty = 0.01 * (xt * xt) + (yt - 2.0) * (yt - 2.0);
      const double vel_penalty = 1e-3 * (v[1] * v[1]) + 5e-3 * (v[2] * v[2]);
      reward = 10.0 - dist_penalty - vel_penalty;
      done = yt <= 1.0;
    }
  }
};

template <int NP>
__global__ __launch_bounds__(256) void k_cartchain_step(const EnvStepArgs A, const CartChainDev m) { lane_step_frame<CartChainTask<NP>>(A, m); }
template <int NP>
__global__ __launch_bounds__(256) void k_cartchain_reset(const LaneResetArgs R) { lane_reset_frame<CartChainTask<NP>>(R, CartChainDev{}); }

// ------------------------------------------------------------------------------------------------ the two mountain cars
// gym 0.22's Continuous_MountainCarEnv (continuous_mountain_car.py, behind NormalizedBoxEnv) and MountainCarEnv (mountain_car.py): a point
// on the curve sin(3 x) pushed by `force`; qpos = (x), qvel = (v).  Both share the clamps and the wall; they differ in the push, the goal,
// the reward and in what the env keeps between steps.
struct MountainCarC {
  static constexpr double min_position = -1.2, max_position = 0.6, max_speed = 0.07;
  static constexpr double power = 0.0015, goal_cont = 0.45;      // Continuous_MountainCarEnv
  static constexpr double force = 0.001, gravity = 0.0025, goal = 0.5;   // MountainCarEnv
};

// NormalizedBoxEnv.step on float32 arrays over Box(-1, 1): lb + (a + 1.0) * 0.5 * (ub - lb), one rounding per operation, then np.clip (which
// is also the env's own min(max(action, -1), 1)).  The comparisons keep a NaN a NaN.
__device__ __forceinline__ float mountaincar_force(float a) {
  const float t = ((a + 1.0f) * 0.5f) * 2.0f;
  const float s = -1.0f + t;
  return s < -1.0f ? -1.0f : (s > 1.0f ? 1.0f : s);
}

// the clamps, the move and the inelastic left wall, as both envs have them (a NaN passes through every comparison)
__device__ __forceinline__ void mountaincar_move(double& x, double& v) {
  v = v < -MountainCarC::max_speed ? -MountainCarC::max_speed : (v > MountainCarC::max_speed ? MountainCarC::max_speed : v);
  x = x + v;
  x = x < MountainCarC::min_position ? MountainCarC::min_position : (x > MountainCarC::max_position ? MountainCarC::max_position : x);
  if (x == MountainCarC::min_position && v < 0.0) v = 0.0;
}

template <bool CONT>
struct MountainCarTask {
  static constexpr int NQ = 1, NV = 1, O = 2, NA = 1;
  static constexpr bool never_done = false;
  using Model = LaneNoModel;
  using State = LaneStateQV<1, 1>;

  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) { dst[0] = (float)s.q[0]; dst[1] = (float)s.v[0]; }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset(): (np_random.uniform(low=-0.6, high=-0.4), 0) from counter 0 of the env's Philox stream.  The continuous env keeps a float32 array
  static __device__ __forceinline__ void reset_state(const Model&, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    const double x = -0.6 + 0.2 * env_uniform(seed, stream, step, env, 0);
    s.q[0] = CONT ? (double)(float)x : x;
    s.v[0] = 0.0;
  }

  static __device__ __forceinline__ void advance(const Model&, State& s, const float (&act)[1], double& reward, bool& done, bool& finite) {
    double x = s.q[0], v = s.v[0];
    if constexpr (CONT) {
      const double force = (double)mountaincar_force(act[0]);
      v = v + (force * MountainCarC::power - MountainCarC::gravity * cos(3.0 * x));
      mountaincar_move(x, v);
      done = x >= MountainCarC::goal_cont && v >= 0.0;
      reward = (done ? 100.0 : 0.0) - (force * force) * 0.1;
      // self.state = np.array([position, velocity], dtype=np.float32): the env carries float32 values from step to step
      x = (double)(float)x; v = (double)(float)v;
    } else {
      // the action is the index held as a float, used as it is: 0, 1, 2 push left, not at all, right
      v = v + (((double)act[0] - 1.0) * MountainCarC::force + cos(3.0 * x) * (-MountainCarC::gravity));
      mountaincar_move(x, v);
      done = x >= MountainCarC::goal && v >= 0.0;
      reward = -1.0;
    }
    finite = isfinite(x) && isfinite(v);
    s.q[0] = x; s.v[0] = v;
  }
};

__global__ __launch_bounds__(256) void k_mountaincar_cont_step(const EnvStepArgs A) { lane_step_frame<MountainCarTask<true>>(A, {}); }
__global__ __launch_bounds__(256) void k_mountaincar_cont_reset(const LaneResetArgs R) { lane_reset_frame<MountainCarTask<true>>(R, {}); }
__global__ __launch_bounds__(256) void k_mountaincar_step(const EnvStepArgs A) { lane_step_frame<MountainCarTask<false>>(A, {}); }
__global__ __launch_bounds__(256) void k_mountaincar_reset(const LaneResetArgs R) { lane_reset_frame<MountainCarTask<false>>(R, {}); }

// ------------------------------------------------------------------------------------------------ Acrobot
// gym 0.22's AcrobotEnv (acrobot.py), book_or_nips = "book", no torque noise: qpos = (theta1, theta2), qvel = (dtheta1, dtheta2).  Every
// constant is written as gym's expression of LINK_MASS = LINK_LENGTH = LINK_MOI = 1, LINK_COM_POS = 0.5, g = 9.8 and folds, in float64, to
// what Python computes.
struct AcrobotC {
  static constexpr double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8, dt = 0.2;
  static constexpr double pi = 3.141592653589793, max_vel_1 = 4.0 * pi, max_vel_2 = 9.0 * pi;
  static constexpr int wrap_trips = 16;   // wrap()'s loops end after this many turns: an angle further out is not finite for the frame
};

// _dsdt, the "book" branch, in Python's order of evaluation (x ** 2 as x * x)
__device__ __forceinline__ void acrobot_dsdt(const double (&q)[2], const double (&v)[2], double a, double (&acc)[2]) {
  using C = AcrobotC;
  const double c2 = cos(q[1]), s2 = sin(q[1]);
  const double d1 = C::m1 * (C::lc1 * C::lc1) + C::m2 * (((C::l1 * C::l1) + (C::lc2 * C::lc2)) + ((2.0 * C::l1) * C::lc2) * c2) + C::I1 + C::I2;
  const double d2 = C::m2 * ((C::lc2 * C::lc2) + (C::l1 * C::lc2) * c2) + C::I2;
  const double phi2 = ((C::m2 * C::lc2) * C::g) * cos((q[0] + q[1]) - C::pi / 2.0);
  const double phi1 = ((((-C::m2 * C::l1) * C::lc2) * (v[1] * v[1])) * s2 - (((((2.0 * C::m2) * C::l1) * C::lc2) * v[1]) * v[0]) * s2 +
                       ((C::m1 * C::lc1 + C::m2 * C::l1) * C::g) * cos(q[0] - C::pi / 2.0)) + phi2;
  const double dd2 = (((a + (d2 / d1) * phi1) - (((C::m2 * C::l1) * C::lc2) * (v[0] * v[0])) * s2) - phi2) /
                     ((C::m2 * (C::lc2 * C::lc2) + C::I2) - (d2 * d2) / d1);
  acc[0] = -(d2 * dd2 + phi1) / d1;
  acc[1] = dd2;
}

// wrap(x, -pi, pi): gym's subtract / add 2 pi loops, ended after wrap_trips turns (gym's would not end on an infinite angle)
__device__ __forceinline__ double acrobot_wrap(double x) {
  const double diff = AcrobotC::pi - (-AcrobotC::pi);
#pragma unroll 1
  for (int i = 0; i < AcrobotC::wrap_trips && x > AcrobotC::pi; ++i) x = x - diff;
#pragma unroll 1
  for (int i = 0; i < AcrobotC::wrap_trips && x < -AcrobotC::pi; ++i) x = x + diff;
  return x;
}
__device__ __forceinline__ double acrobot_bound(double x, double m, double M) { return x < m ? m : (x > M ? M : x); }   // min(max(x, m), M): NaN stays

struct AcrobotTask {
  static constexpr int NQ = 2, NV = 2, O = 6, NA = 1;
  static constexpr bool never_done = false;
  using Model = LaneNoModel;
  using State = LaneStateQV<2, 2>;

  // _get_ob(): float32 (cos theta1, sin theta1, cos theta2, sin theta2, dtheta1, dtheta2)
  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {
    dst[0] = (float)cos(s.q[0]); dst[1] = (float)sin(s.q[0]); dst[2] = (float)cos(s.q[1]); dst[3] = (float)sin(s.q[1]);
    dst[4] = (float)s.v[0]; dst[5] = (float)s.v[1];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset(): np_random.uniform(low=-0.1, high=0.1, size=(4,)).astype(np.float32) — component k of (theta1, theta2, dtheta1, dtheta2) from
  // counter k of the env's Philox stream, rounded to float32
  static __device__ __forceinline__ void reset_state(const Model&, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    s.q[0] = (double)(float)(-0.1 + 0.2 * env_uniform(seed, stream, step, env, 0));
    s.q[1] = (double)(float)(-0.1 + 0.2 * env_uniform(seed, stream, step, env, 1));
    s.v[0] = (double)(float)(-0.1 + 0.2 * env_uniform(seed, stream, step, env, 2));
    s.v[1] = (double)(float)(-0.1 + 0.2 * env_uniform(seed, stream, step, env, 3));
  }

  static __device__ __forceinline__ void advance(const Model&, State& s, const float (&act)[1], double& reward, bool& done, bool& finite) {
    // AVAIL_TORQUE[a] = a - 1: the index held as a float, used as it is.  rk4() carries it as a fifth component whose derivative is 0:
    // y0[4] + dt * 0.0 is the torque itself in every stage
    const double torque = (double)act[0] - 1.0;
    const double h = AcrobotC::dt;
    double qs[2], vs[2], qsum[2], vsum[2], a[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { qs[i] = s.q[i]; vs[i] = s.v[i]; qsum[i] = 0.0; vsum[i] = 0.0; }
    // rk4(): ONE dynamics call site in a 4-trip loop, cartchain_substep's form; y0 + dt / 6 * (k1 + 2 k2 + 2 k3 + k4), dt2 = dt / 2
#pragma unroll 1
    for (int stage = 0; stage < 4; ++stage) {
      acrobot_dsdt(qs, vs, torque, a);
      const double w = (stage == 1 || stage == 2) ? 2.0 : 1.0;
      const double ch = (stage == 2) ? h : h / 2.0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        qsum[i] = stage == 0 ? vs[i] : qsum[i] + w * vs[i];
        vsum[i] = stage == 0 ? a[i] : vsum[i] + w * a[i];
        const double vn = s.v[i] + ch * a[i];
        qs[i] = s.q[i] + ch * vs[i];
        vs[i] = vn;
      }
    }
    double th1 = s.q[0] + h / 6.0 * qsum[0], th2 = s.q[1] + h / 6.0 * qsum[1];
    double w1 = s.v[0] + h / 6.0 * vsum[0], w2 = s.v[1] + h / 6.0 * vsum[1];
    th1 = acrobot_wrap(th1); th2 = acrobot_wrap(th2);
    w1 = acrobot_bound(w1, -AcrobotC::max_vel_1, AcrobotC::max_vel_1);
    w2 = acrobot_bound(w2, -AcrobotC::max_vel_2, AcrobotC::max_vel_2);
    done = -cos(th1) - cos(th2 + th1) > 1.0;
    reward = done ? 0.0 : -1.0;
    // an angle the capped wrap left outside [-pi, pi] counts as not finite: the episode ends there
    finite = isfinite(w1) && isfinite(w2) && fabs(th1) <= AcrobotC::pi && fabs(th2) <= AcrobotC::pi;
    s.q[0] = th1; s.q[1] = th2; s.v[0] = w1; s.v[1] = w2;
  }
};

__global__ __launch_bounds__(256) void k_acrobot_step(const EnvStepArgs A) { lane_step_frame<AcrobotTask>(A, {}); }
__global__ __launch_bounds__(256) void k_acrobot_reset(const LaneResetArgs R) { lane_reset_frame<AcrobotTask>(R, {}); }
