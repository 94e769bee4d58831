// swimmer_env.h — Swimmer stepper of ilsx_vecenv: a task of the lane-per-env frame.  It uses, by name, env_uniform and impedance_d
// (ilsx_env.hip) and lane_step_frame / lane_reset_frame, LaneStateQV, cartchain_ctrl and cartchain_chol_solve (classic_env.h).
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

// The task of the lane-per-env frame (classic_env.h).  The frame turns the arguments its tail needs into per-lane values before the RK4
// loop: read after the loop they cost this kernel a private segment (a dead scalar spill slot).
template <int NL>
struct SwimmerTask {
  static constexpr int N = NL + 2, NQ = N, NV = N, O = 2 * NL + 2, NA = NL - 1;
  static constexpr bool never_done = true;
  using Model = SwimmerDev;
  using State = LaneStateQV<N, N>;

  // _get_obs(): float32 (qpos[2:] | qvel)
  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {
#pragma unroll
    for (int i = 0; i < NL; ++i) dst[i] = (float)s.q[2 + i];
#pragma unroll
    for (int i = 0; i < NL + 2; ++i) dst[NL + i] = (float)s.v[i];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset_model(): qpos = init + U(+-0.1) (counters 0 .. N-1 of the env's Philox stream), qvel = U(+-0.1) (counters N .. 2N-1)
  static __device__ __forceinline__ void reset_state(const Model& m, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    static_assert(NL == 3, "the draws are written out for five degrees of freedom");
#define SWIMMER_DRAW(k) env_uniform(seed, stream, step, env, k)
    s.q[0] = m.init_qpos[0] + (-0.1 + 0.2 * SWIMMER_DRAW(0));
    s.q[1] = m.init_qpos[1] + (-0.1 + 0.2 * SWIMMER_DRAW(1));
    s.q[2] = m.init_qpos[2] + (-0.1 + 0.2 * SWIMMER_DRAW(2));
    s.q[3] = m.init_qpos[3] + (-0.1 + 0.2 * SWIMMER_DRAW(3));
    s.q[4] = m.init_qpos[4] + (-0.1 + 0.2 * SWIMMER_DRAW(4));
    s.v[0] = -0.1 + 0.2 * SWIMMER_DRAW(5);
    s.v[1] = -0.1 + 0.2 * SWIMMER_DRAW(6);
    s.v[2] = -0.1 + 0.2 * SWIMMER_DRAW(7);
    s.v[3] = -0.1 + 0.2 * SWIMMER_DRAW(8);
    s.v[4] = -0.1 + 0.2 * SWIMMER_DRAW(9);
#undef SWIMMER_DRAW
  }

  static __device__ __forceinline__ void advance(const Model& m, State& s, const float (&act)[NA], double& reward, bool& done, bool& finite) {
    double tau[NA], ctrl2 = 0.0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const double c = (double)cartchain_ctrl(act[j], m.ctrl_lo, m.ctrl_hi);
      tau[j] = m.gear[j] * c;
      ctrl2 += c * c;
    }
    const double x_before = s.q[0];
#pragma unroll 1
    for (int k = 0; k < m.frame_skip; ++k) swimmer_substep<NL>(m, s.q, s.v, tau);
    finite = true;
#pragma unroll
    for (int i = 0; i < N; ++i) finite = finite && isfinite(s.q[i]) && isfinite(s.v[i]);
    reward = (s.q[0] - x_before) / ((double)m.frame_skip * m.timestep) - 1e-4 * ctrl2;
    done = false;
  }
};

template <int NL>
__global__ __launch_bounds__(256) void k_swimmer_step(const EnvStepArgs A, const SwimmerDev m) { lane_step_frame<SwimmerTask<NL>>(A, m); }
template <int NL>
__global__ __launch_bounds__(256) void k_swimmer_reset(const LaneResetArgs R, const SwimmerDev m) { lane_reset_frame<SwimmerTask<NL>>(R, m); }
