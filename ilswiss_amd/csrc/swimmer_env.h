// swimmer_env.h — Swimmer stepper of ilsx_vecenv, included by ilsx_env.hip after classic_env.h (it uses EnvStepArgs, env_uniform,
// impedance_d, cartchain_ctrl and cartchain_chol_solve).
//
// gym 0.22's SwimmerEnv task rules (rlkit/envs/envs_dict.py `swimmer`) behind the reference's NormalizedBoxEnv, on this repository's own
// dynamics of a free planar chain in a viscous medium (the constants are ilswiss_amd/envs/models_swimmer.py,
// UNVERIFIED against MuJoCo).  DoF (x, y, theta_0, q_1, ..., q_{NL-1}): link 0 carries two slides and a hinge at its origin, link k >= 1
// hinges on link k - 1 at anchor[k]; phi_b = theta_0 + q_1 + ... + q_b is a link's absolute angle, counter-clockwise.
//   M(q) qdd + c(q, qd) = tau + J^T f,  M = sum_b m_b Jc_b^T Jc_b + I_b Jphi_b^T Jphi_b + diag(armature),
//   tau = gear * ctrl - damping * qd + sum_b (Jc_b^T F_b + Jphi_b^T t_b),  no gravity in the plane, no contacts,
// F_b, t_b the drag of link b's inertia box (sides bx along the link, by across it, bz normal to the plane; d = (bx + by + bz) / 3), from
// the velocity (vx, vy) of its centre of mass in the link's own axes and its angular rate w:
//   fx = -3 pi beta d vx - 1/2 rho by bz |vx| vx,  fy = -3 pi beta d vy - 1/2 rho bx bz |vy| vy,
//   t  = -pi beta d^3 w - rho bz (bx^4 + by^4) |w| w / 64,
// evaluated with every RK4 stage's own state.  One unilateral soft row per violated hinge limit (section 19's rule, projected
// Gauss-Seidel), classic RK4 with the constraint solve inside every stage, frame_skip substeps.  One lane per env; the lower triangle of
// the (NL + 2)^2 mass matrix, its Cholesky factor, two columns of M^-1 and the 2x2 A of the rows live in registers, every index is a
// compile-time constant; no LDS.  The five drag coefficients of a link are formed on the host from the box sides.
#pragma once

struct SwimmerDev {
  int frame_skip, pgs_iters, limited[2];      // limited / range: the hinges q_1, q_2
  double mass[3], inertia[3], com[3][2], anchor[3][2];
  double drag[3][5];                          // 3 pi beta d | rho by bz / 2 | rho bx bz / 2 | pi beta d^3 | rho bz (bx^4 + by^4) / 64
  double armature[5], damping[5], range[2][2], gear[2], init_qpos[5];
  double timestep, solimp[3], lim_b, lim_k;   // lim_b = 2 / (dmax tc), lim_k = 1 / (dmax^2 tc^2 dr^2)
  float ctrl_lo, ctrl_hi;
};

// qacc = f(q, v, tau) with the limit rows solved; tau[j] drives hinge q_{j+1}
template <int NL>
__device__ __forceinline__ void swimmer_dynamics(const SwimmerDev& m, const double (&q)[NL + 2], const double (&v)[NL + 2],
                                                 const double (&tau)[NL - 1], double (&qacc)[NL + 2]) {
  static_assert(NL == 3, "two limit rows and a 2x2 A: three links");
  constexpr int N = NL + 2;
  // ---- absolute angles and rates; e[k] = link k's hinge seen from link k - 1's origin, d[b] = COM of link b seen from its origin (world axes)
  double sn[NL], cs[NL], w[NL], ex[NL], ey[NL], dx[NL], dy[NL];
  {
    double ph = q[2], om = v[2];
#pragma unroll
    for (int b = 0; b < NL; ++b) {
      if (b > 0) { ph += q[2 + b]; om += v[2 + b]; }
      double sb, cb;
      sincos(ph, &sb, &cb);
      sn[b] = sb; cs[b] = cb;
      w[b] = om;
      dx[b] = cs[b] * m.com[b][0] - sn[b] * m.com[b][1];
      dy[b] = sn[b] * m.com[b][0] + cs[b] * m.com[b][1];
      if (b > 0) {
        ex[b] = cs[b - 1] * m.anchor[b][0] - sn[b - 1] * m.anchor[b][1];
        ey[b] = sn[b - 1] * m.anchor[b][0] + cs[b - 1] * m.anchor[b][1];
      } else {
        ex[b] = 0.0; ey[b] = 0.0;
      }
    }
  }
  // ---- mass matrix (lower triangle) and right-hand side, one link at a time: only one link's Jacobian is alive
  double M[N][N], rhs[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rhs[i] = 0.0;
#pragma unroll
    for (int k = 0; k <= i; ++k) M[i][k] = 0.0;
  }
#pragma unroll
  for (int b = 0; b < NL; ++b) {
    // COM Jacobian: columns x, y are the unit vectors, column 2 + j (j <= b) is perp(COM - origin of link j); the angular Jacobian is 1 there
    double jx[N], jy[N];
    jx[0] = 1.0; jy[0] = 0.0; jx[1] = 0.0; jy[1] = 1.0;
    double rx = dx[b], ry = dy[b];
    double ax = -(w[b] * w[b]) * dx[b], ay = -(w[b] * w[b]) * dy[b];   // acceleration of the COM at qdd = 0
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      if (j > b) { jx[2 + j] = 0.0; jy[2 + j] = 0.0; continue; }
      jx[2 + j] = -ry; jy[2 + j] = rx;
      if (j > 0) {
        rx += ex[j]; ry += ey[j];
        ax -= (w[j - 1] * w[j - 1]) * ex[j]; ay -= (w[j - 1] * w[j - 1]) * ey[j];
      }
    }
    double vcx = v[0], vcy = v[1];
#pragma unroll
    for (int j = 0; j <= b; ++j) { vcx += jx[2 + j] * v[2 + j]; vcy += jy[2 + j] * v[2 + j]; }
    // drag in the link's axes, turned to the world
    const double vx = cs[b] * vcx + sn[b] * vcy, vy = cs[b] * vcy - sn[b] * vcx;
    const double fx = -m.drag[b][0] * vx - m.drag[b][1] * (fabs(vx) * vx);
    const double fy = -m.drag[b][0] * vy - m.drag[b][2] * (fabs(vy) * vy);
    const double tz = -m.drag[b][3] * w[b] - m.drag[b][4] * (fabs(w[b]) * w[b]);
    const double Fx = (cs[b] * fx - sn[b] * fy) - m.mass[b] * ax, Fy = (sn[b] * fx + cs[b] * fy) - m.mass[b] * ay;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const bool ai = i >= 2 && i - 2 <= b;
      rhs[i] += jx[i] * Fx + jy[i] * Fy;
      if (ai) rhs[i] += tz;
#pragma unroll
      for (int k = 0; k <= i; ++k) {
        M[i][k] += m.mass[b] * (jx[i] * jx[k] + jy[i] * jy[k]);
        if (ai && k >= 2) M[i][k] += m.inertia[b];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) { M[i][i] += m.armature[i]; rhs[i] -= m.damping[i] * v[i]; }
#pragma unroll
  for (int j = 0; j < NL - 1; ++j) rhs[3 + j] += tau[j];
  // ---- Cholesky M = L L^T
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
#pragma unroll
  for (int i = 0; i < N; ++i) qacc[i] = qacc0[i];
  // ---- limit rows: hinge q_1 (DoF 3), then hinge q_2 (DoF 4); J = sg * e_dof, r = distance to the limit, negative when violated
  bool on[2];
  double sg[2], r[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    on[j] = false; sg[j] = 0.0; r[j] = 0.0;
    if (m.limited[j]) {
      if (q[3 + j] - m.range[j][0] < 0.0) { on[j] = true; sg[j] = 1.0; r[j] = q[3 + j] - m.range[j][0]; }
      else if (m.range[j][1] - q[3 + j] < 0.0) { on[j] = true; sg[j] = -1.0; r[j] = m.range[j][1] - q[3 + j]; }
    }
  }
  if (!on[0] && !on[1]) return;
  double u[2][N], e[N];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (i == 3 + j) ? 1.0 : 0.0;
    cartchain_chol_solve<N>(L, e, u[j]);
  }
  const double a01 = (sg[0] * sg[1]) * u[0][4];
  double den[2], rc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double ajj = u[j][3 + j];
    const double d = impedance_d(fabs(r[j]), m.solimp);
    const double aref = -m.lim_b * (sg[j] * v[3 + j]) - m.lim_k * d * r[j];
    den[j] = ajj + (1.0 - d) / d * ajj;
    rc[j] = aref - sg[j] * qacc0[3 + j];
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
}

// classic RK4 on (q, qd), cartchain_substep's form: ONE dynamics call site in a 4-trip loop, sums in the order q + h/6 (k1 + 2 k2 + 2 k3 + k4)
template <int NL>
__device__ __forceinline__ void swimmer_substep(const SwimmerDev& m, double (&q)[NL + 2], double (&v)[NL + 2], const double (&tau)[NL - 1]) {
  constexpr int N = NL + 2;
  const double h = m.timestep;
  double qs[N], vs[N], qsum[N], vsum[N], a[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { qs[i] = q[i]; vs[i] = v[i]; qsum[i] = 0.0; vsum[i] = 0.0; }
#pragma unroll 1
  for (int stage = 0; stage < 4; ++stage) {
    swimmer_dynamics<NL>(m, qs, vs, tau, a);
    const double wt = (stage == 1 || stage == 2) ? 2.0 : 1.0;
    const double ch = (stage == 2) ? h : 0.5 * h;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      qsum[i] = stage == 0 ? vs[i] : qsum[i] + wt * vs[i];
      vsum[i] = stage == 0 ? a[i] : vsum[i] + wt * a[i];
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

// _get_obs(): float32 (qpos[2:] | qvel)
template <int NL>
__device__ __forceinline__ void swimmer_write_obs(const double (&q)[NL + 2], const double (&v)[NL + 2], float* dst) {
#pragma unroll
  for (int i = 0; i < NL; ++i) dst[i] = (float)q[2 + i];
#pragma unroll
  for (int i = 0; i < NL + 2; ++i) dst[NL + i] = (float)v[i];
}

// reset_model(): qpos = init + U(+-0.1) (counters 0 .. N-1 of the env's Philox stream), qvel = U(+-0.1) (counters N .. 2N-1)
template <int NL>
__device__ __forceinline__ void swimmer_reset_state(const SwimmerDev& m, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env,
                                                    double (&q)[NL + 2], double (&v)[NL + 2]) {
  static_assert(NL == 3, "the draws are written out for five degrees of freedom");
#define SWIMMER_DRAW(k) env_uniform(seed, stream, step, env, k)
  q[0] = m.init_qpos[0] + (-0.1 + 0.2 * SWIMMER_DRAW(0));
  q[1] = m.init_qpos[1] + (-0.1 + 0.2 * SWIMMER_DRAW(1));
  q[2] = m.init_qpos[2] + (-0.1 + 0.2 * SWIMMER_DRAW(2));
  q[3] = m.init_qpos[3] + (-0.1 + 0.2 * SWIMMER_DRAW(3));
  q[4] = m.init_qpos[4] + (-0.1 + 0.2 * SWIMMER_DRAW(4));
  v[0] = -0.1 + 0.2 * SWIMMER_DRAW(5);
  v[1] = -0.1 + 0.2 * SWIMMER_DRAW(6);
  v[2] = -0.1 + 0.2 * SWIMMER_DRAW(7);
  v[3] = -0.1 + 0.2 * SWIMMER_DRAW(8);
  v[4] = -0.1 + 0.2 * SWIMMER_DRAW(9);
#undef SWIMMER_DRAW
}

// Everything the tail needs from the arguments is turned into per-lane values BEFORE the RK4 loop (the addresses it stores to, the reset
// state it may select): the loop then carries them in vector registers, of which there are plenty, instead of keeping forty-odd scalar
// registers of arguments alive across the dynamics.  With the arguments read after the loop the scalar allocator spilled an 8-dword
// tuple it later rematerialised, and the dead spill slot left the kernel a private segment.
template <int NL>
__global__ __launch_bounds__(256) void k_swimmer_step(const EnvStepArgs A, const SwimmerDev m) {
  constexpr int N = NL + 2, O = 2 * NL + 2, NA = NL - 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.n_ids) return;
  const int env = A.ids ? A.ids[t] : t;
  if (A.frozen && A.frozen[env]) return;
  const size_t ne = (size_t)A.n_env;
  double* const qp = A.qpos + env;
  double* const vp = A.qvel + env;
  double q[N], v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { q[i] = qp[i * ne]; v[i] = vp[i * ne]; }
  float* const obs_p = A.obs ? A.obs + (size_t)t * O : nullptr;
  float* const rew_p = A.rew ? A.rew + t : nullptr;
  unsigned char* const done_p = A.done ? A.done + t : nullptr;
  float* const cur_p = A.obs_cur ? A.obs_cur + (size_t)env * O : nullptr;
  float* rec = nullptr;   // fused replay insert (k_env_step's record layout: obs | act | rew | done | next_obs | absorbing[2])
  if (A.replay) {
    long long slot = A.top + env;
    if (slot >= A.cap) slot -= A.cap;
    rec = A.stage ? A.stage + ((size_t)env * A.stage_len + A.ep_len[env]) * A.rec : A.replay + (size_t)slot * A.rec;
  }
  float av[NA], rav[NA];
  double tau[NA], ctrl2 = 0.0;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    av[j] = A.act[(size_t)t * NA + j];
    rav[j] = A.rec_act ? A.rec_act[(size_t)t * NA + j] : av[j];   // the record holds the unmapped action
    const double c = (double)cartchain_ctrl(av[j], m.ctrl_lo, m.ctrl_hi);
    tau[j] = m.gear[j] * c;
    ctrl2 += c * c;
  }
  if (rec) {
    float obs_before[O];
    swimmer_write_obs<NL>(q, v, obs_before);
#pragma unroll
    for (int i = 0; i < O; ++i) rec[i] = obs_before[i];
#pragma unroll
    for (int j = 0; j < NA; ++j) rec[O + j] = rav[j];
  }
  // auto-reset bookkeeping that does not depend on the step: the episode's length and whether it ends at the path limit, the return so
  // far, and the state a reset would give (ten Philox blocks: nothing beside the dynamics)
  int len = 0;
  bool limit = false;
  double ret0 = 0.0, rq[N], rv[N];
  int* const len_p = A.ep_len + env;
  double* const ret_p = A.ep_ret + env;
  int* const flush_p = (A.auto_reset && A.flush_len) ? A.flush_len + env : nullptr;
  double* const stats_p = A.stats;
  const bool auto_reset = A.auto_reset != 0;
  if (auto_reset) {
    len = *len_p + 1;
    ret0 = *ret_p;
    limit = len >= A.max_path_length;
    swimmer_reset_state<NL>(m, A.seed, A.stream, A.step, (uint32_t)env, rq, rv);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) { rq[i] = 0.0; rv[i] = 0.0; }
  }
  const double x_before = q[0];
#pragma unroll 1
  for (int s = 0; s < m.frame_skip; ++s) swimmer_substep<NL>(m, q, v, tau);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < N; ++i) finite = finite && isfinite(q[i]) && isfinite(v[i]);
  const double reward = (q[0] - x_before) / ((double)m.frame_skip * m.timestep) - 1e-4 * ctrl2;
  float ob[O];
  swimmer_write_obs<NL>(q, v, ob);
  if (obs_p) {
#pragma unroll
    for (int i = 0; i < O; ++i) obs_p[i] = ob[i];
  }
  if (rew_p) *rew_p = (float)reward;
  if (done_p) *done_p = 0;   // never done
  if (rec) {
    rec[O + NA] = (float)reward;
    rec[O + NA + 1] = 0.0f;
#pragma unroll
    for (int i = 0; i < O; ++i) rec[O + NA + 2 + i] = ob[i];
    rec[2 * O + NA + 2] = 0.0f; rec[2 * O + NA + 3] = 0.0f;   // absorbing = [0, 0]
  }
  if (auto_reset) {
    const double ret = ret0 + reward;
    const bool end = limit || !finite;   // never done: the path limit or a non-finite state ends the episode
    if (end) {
      atomicAdd(&stats_p[0], 1.0);
      atomicAdd(&stats_p[1], ret);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) { q[i] = end ? rq[i] : q[i]; v[i] = end ? rv[i] : v[i]; }
    swimmer_write_obs<NL>(q, v, ob);
    *len_p = end ? 0 : len;
    *ret_p = end ? 0.0 : ret;
    if (flush_p) *flush_p = end ? len : 0;   // never terminal
  }
  if (cur_p) {
#pragma unroll
    for (int i = 0; i < O; ++i) cur_p[i] = ob[i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) { qp[i * ne] = q[i]; vp[i * ne] = v[i]; }
}

template <int NL>
__global__ __launch_bounds__(256) void k_swimmer_reset(double* qpos, double* qvel, int n_env, const int* ids, int n_ids, float* obs,
                                                       float* obs_cur, int* ep_len, double* ep_ret, uint64_t seed, uint32_t stream,
                                                       unsigned long long step, const SwimmerDev m) {
  constexpr int N = NL + 2, O = 2 * NL + 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_ids) return;
  const int env = ids ? ids[t] : t;
  double q[N], v[N];
  swimmer_reset_state<NL>(m, seed, stream, step, (uint32_t)env, q, v);
  float ob[O];
  swimmer_write_obs<NL>(q, v, ob);
#pragma unroll
  for (int i = 0; i < O; ++i) {
    if (obs) obs[(size_t)t * O + i] = ob[i];
    if (obs_cur) obs_cur[(size_t)env * O + i] = ob[i];
  }
  ep_len[env] = 0; ep_ret[env] = 0.0;
  const size_t ne = (size_t)n_env;
#pragma unroll
  for (int i = 0; i < N; ++i) { qpos[i * ne + env] = q[i]; qvel[i * ne + env] = v[i]; }
}
