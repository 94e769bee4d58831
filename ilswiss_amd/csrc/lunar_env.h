// lunar_env.h — LunarLanderContinuous stepper of ilsx_vecenv: a task of the lane-per-env frame.  It uses, by name, env_uniform and
// impedance_d (ilsx_env.hip) and lane_step_frame / lane_reset_frame, LaneStateQV and LaneCoords (classic_env.h).
//
// gym 0.22's LunarLander task rules, continuous branch (rlkit/envs/envs_dict.py `lunarlandercont`; NormalizedBoxEnv over Box(-1, 1) is the
// identity map), on this repository's own dynamics (the constants are ilswiss_amd/envs/models_lunar.py, UNVERIFIED
// against gym and Box2D).  ONE rigid body of three degrees of freedom: hull and legs move as one, the legs held at their rest angle.
//   state    qpos = (x, y, theta of the hull origin | smooth_y[0..10], the episode's terrain), qvel = (vx, vy of the hull origin, omega |
//            sleep_time); float64.  The dynamics run on the centre of mass, where M = diag(m, m, I).
//   engines  impulses on the body about its centre of mass, once, before the substeps; their dispersion is drawn on every step
//   step     frame_skip substeps of semi-implicit Euler over 1 / FPS: a = g + M^-1 J^T f, v += h a, q += h v
//   contact  the two foot points against the terrain segment under their x (clamped to [0, W]): a foot at or below the segment's line
//            gives a soft unilateral normal row and a friction row along the segment, |f_t| <= mu f_n, rows by the planar engine's rule
//              (A + R) f = aref - J a0,  A = J M^-1 J^T,  R_i = (1 - d_i) / d_i A_ii,  aref_n = -b J_n v - k d r,  aref_t = -b J_t v,
//              b = 2 / (dmax tc),  k = 1 / (dmax^2 tc^2 dr^2),  d = impedance(|r|),
//            pgs_iters projected Gauss-Seidel sweeps in the order (n0, t0, n1, t1).  A is 4x4 and stays in registers.
//   crash    a hull vertex at or below the terrain after the step ends the episode (no contact response for the hull)
//   sleep    sleep_time += 1 / FPS while |v|^2 <= lin_tol^2 and omega^2 <= ang_tol^2 after the step, else 0; asleep at sleep_time >= 0.5
// One lane per env; the terrain is read with a chain of selects on the segment index (no indexed registers); no LDS.
#pragma once

struct LunarDev {
  int frame_skip, pgs_iters;
  double fps, scale, w, h, gravity, main_power, side_power, initial_random, side_height, side_away, leg_down, helipad_y;
  double mass, inertia, com[2], foot[2][2], hull[6][2];
  double friction, solimp[3], con_b, con_k;   // con_b = 2 / (dmax tc), con_k = 1 / (dmax^2 tc^2 dr^2)
  double sleep_lin2, sleep_ang2, sleep_time;  // the two tolerances squared
  double chunk_dx;                            // W / (CHUNKS - 1)
};

// signed distance of the point (px, py) from the line of the terrain segment under px (px clamped to [0, W]), positive above; the
// segment's unit tangent (tx, ty) comes back too, its normal is (-ty, tx)
__device__ __forceinline__ double lunar_gap(const LunarDev& m, const double* sy, double px, double py, double& tx, double& ty) {
  const double xc = fmin(fmax(px, 0.0), m.w);
  int j = (int)(xc / m.chunk_dx);
  j = j > 9 ? 9 : j;
  double y0 = sy[0], y1 = sy[1];
#pragma unroll
  for (int k = 1; k < 10; ++k)
    if (j == k) { y0 = sy[k]; y1 = sy[k + 1]; }
  const double x0 = (double)j * m.chunk_dx;
  const double dy = y1 - y0;
  const double len = sqrt(m.chunk_dx * m.chunk_dx + dy * dy);
  tx = m.chunk_dx / len; ty = dy / len;
  return (py - y0) * tx - (px - x0) * ty;
}

// the observation in float64: a function of the state alone
__device__ __forceinline__ void lunar_obs64(const LunarDev& m, const double (&q)[14], const double (&v)[4], double (&o)[8]) {
  double s, c, tx, ty;
  sincos(q[2], &s, &c);
  o[0] = (q[0] - m.w / 2.0) / (m.w / 2.0);
  o[1] = (q[1] - (m.helipad_y + m.leg_down / m.scale)) / (m.h / 2.0);
  o[2] = v[0] * (m.w / 2.0) / m.fps;
  o[3] = v[1] * (m.h / 2.0) / m.fps;
  o[4] = q[2];
  o[5] = 20.0 * v[2] / m.fps;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double fx = q[0] + (c * m.foot[i][0] - s * m.foot[i][1]), fy = q[1] + (s * m.foot[i][0] + c * m.foot[i][1]);
    o[6 + i] = lunar_gap(m, q + 3, fx, fy, tx, ty) <= 0.0 ? 1.0 : 0.0;
  }
}

__device__ __forceinline__ double lunar_shaping(const double (&o)[8]) {
  return -100.0 * sqrt(o[0] * o[0] + o[1] * o[1]) - 100.0 * sqrt(o[2] * o[2] + o[3] * o[3]) - 100.0 * fabs(o[4]) + 10.0 * o[6] + 10.0 * o[7];
}

// One env step after the engines: (jx, jy) is the impulse they gave the body and jw its moment about the centre of mass.  Leaves the
// new state in (q, v), sleep_time included, and says whether a hull vertex touched the terrain.
__device__ __forceinline__ void lunar_move(const LunarDev& m, double (&q)[14], double (&v)[4], double jx, double jy, double jw, bool& game_over) {
  const double* sy = q + 3;
  double th = q[2], w = v[2] + jw / m.inertia;
  double s, c;
  sincos(th, &s, &c);
  // the centre of mass and its velocity
  double rx = c * m.com[0] - s * m.com[1], ry = s * m.com[0] + c * m.com[1];
  double cx = q[0] + rx, cy = q[1] + ry;
  double ux = (v[0] - v[2] * ry) + jx / m.mass, uy = (v[1] + v[2] * rx) + jy / m.mass;
  const double h = 1.0 / m.fps / (double)m.frame_skip;
  const double im = 1.0 / m.mass, ii = 1.0 / m.inertia;
#pragma unroll 1
  for (int k = 0; k < m.frame_skip; ++k) {
    sincos(th, &s, &c);
    double ax = 0.0, ay = m.gravity, aw = 0.0;
    // rows 2 i (normal) and 2 i + 1 (tangent) of foot i: J = (dir_x, dir_y, lever x dir)
    double J[4][3], rc[4], den[4];
    bool on[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double lx = c * (m.foot[i][0] - m.com[0]) - s * (m.foot[i][1] - m.com[1]);
      const double ly = s * (m.foot[i][0] - m.com[0]) + c * (m.foot[i][1] - m.com[1]);
      double tx, ty;
      const double r = lunar_gap(m, sy, cx + lx, cy + ly, tx, ty);
      on[i] = r <= 0.0;
      J[2 * i][0] = -ty; J[2 * i][1] = tx; J[2 * i][2] = lx * tx + ly * ty;
      J[2 * i + 1][0] = tx; J[2 * i + 1][1] = ty; J[2 * i + 1][2] = lx * ty - ly * tx;
      const double d = impedance_d(fabs(r), m.solimp);
#pragma unroll
      for (int t = 2 * i; t < 2 * i + 2; ++t) {
        const double jv = J[t][0] * ux + J[t][1] * uy + J[t][2] * w;
        const double att = (J[t][0] * J[t][0] + J[t][1] * J[t][1]) * im + J[t][2] * J[t][2] * ii;
        const double aref = t == 2 * i ? -m.con_b * jv - m.con_k * d * r : -m.con_b * jv;
        den[t] = att + (1.0 - d) / d * att;
        rc[t] = aref - (J[t][0] * ax + J[t][1] * ay + J[t][2] * aw);
      }
    }
    if (on[0] || on[1]) {
      double A[4][4], f[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) A[t][u] = (J[t][0] * J[u][0] + J[t][1] * J[u][1]) * im + J[t][2] * J[u][2] * ii;
#pragma unroll 1
      for (int it = 0; it < m.pgs_iters; ++it) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (!on[t >> 1]) continue;
          double res = rc[t];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (u != t) res -= A[t][u] * f[u];
          double fi = res / den[t];
          if ((t & 1) == 0) fi = fmax(fi, 0.0);
          else { const double lim = m.friction * f[t - 1]; fi = fmin(fmax(fi, -lim), lim); }
          f[t] = fi;
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) { ax += im * (J[t][0] * f[t]); ay += im * (J[t][1] * f[t]); aw += ii * (J[t][2] * f[t]); }
    }
    ux += h * ax; uy += h * ay; w += h * aw;
    cx += h * ux; cy += h * uy; th += h * w;
  }
  sincos(th, &s, &c);
  rx = c * m.com[0] - s * m.com[1]; ry = s * m.com[0] + c * m.com[1];
  q[0] = cx - rx; q[1] = cy - ry; q[2] = th;
  v[0] = ux + w * ry; v[1] = uy - w * rx; v[2] = w;
  game_over = false;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double tx, ty;
    const double px = q[0] + (c * m.hull[k][0] - s * m.hull[k][1]), py = q[1] + (s * m.hull[k][0] + c * m.hull[k][1]);
    game_over = game_over || lunar_gap(m, sy, px, py, tx, ty) <= 0.0;
  }
  const bool still = v[0] * v[0] + v[1] * v[1] <= m.sleep_lin2 && v[2] * v[2] <= m.sleep_ang2;
  v[3] = still ? v[3] + 1.0 / m.fps : 0.0;
}

struct LunarTask {
  static constexpr int NQ = 14, NV = 4, O = 8, NA = 2;
  static constexpr bool never_done = false;
  static constexpr bool step_draws = true;   // advance takes the step's stream coordinates (LaneCoords): the engines' dispersion
  using Model = LunarDev;
  using State = LaneStateQV<14, 4>;

  static __device__ __forceinline__ void write_obs(const Model& m, const State& s, float* dst) {
    double o[8];
    lunar_obs64(m, s.q, s.v, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = (float)o[i];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  // reset(): height[0..11] = U(0, H / 2) from counters 0..11 of the env's Philox stream, the pad's five entries set to helipad_y,
  // smooth_y[i] = 0.33 (height[i-1] + height[i] + height[i+1]) with height[-1] the last entry; the initial force U(+-1000)^2 from
  // counters 12 and 13 acts over the first 1 / FPS; one zero-action step from (W / 2, H, 0) at rest gives the state reset returns
  static __device__ __forceinline__ void reset_state(const Model& m, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    double hgt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) hgt[k] = (k >= 3 && k <= 7) ? m.helipad_y : (m.h / 2.0) * env_uniform(seed, stream, step, env, k);
#pragma unroll
    for (int i = 0; i < 11; ++i) s.q[3 + i] = 0.33 * (hgt[i == 0 ? 11 : i - 1] + hgt[i] + hgt[i + 1]);
    const double fx = -m.initial_random + 2.0 * m.initial_random * env_uniform(seed, stream, step, env, 12);
    const double fy = -m.initial_random + 2.0 * m.initial_random * env_uniform(seed, stream, step, env, 13);
    s.q[0] = m.w / 2.0; s.q[1] = m.h; s.q[2] = 0.0;
    s.v[0] = 0.0; s.v[1] = 0.0; s.v[2] = 0.0; s.v[3] = 0.0;
    bool over;
    lunar_move(m, s.q, s.v, fx / m.fps, fy / m.fps, 0.0, over);
  }

  static __device__ __forceinline__ void advance(const Model& m, State& s, const float (&act)[2], const LaneCoords& at, double& reward,
                                                 bool& done, bool& finite) {
    double o[8];
    lunar_obs64(m, s.q, s.v, o);
    const double before = lunar_shaping(o);
    // np.clip(action, -1, +1) on float32 (a NaN stays a NaN and fires nothing)
    const float a0f = act[0] < -1.0f ? -1.0f : (act[0] > 1.0f ? 1.0f : act[0]);
    const float a1f = act[1] < -1.0f ? -1.0f : (act[1] > 1.0f ? 1.0f : act[1]);
    const double a0 = (double)a0f, a1 = (double)a1f;
    double sn, cs;
    sincos(s.q[2], &sn, &cs);
    const double tipx = sn, tipy = cs, sidex = -tipy, sidey = tipx;
    const double d0 = (2.0 * env_uniform(at.seed, at.stream, at.step, at.env, 14) - 1.0) / m.scale;
    const double d1 = (2.0 * env_uniform(at.seed, at.stream, at.step, at.env, 15) - 1.0) / m.scale;
    const double rx = cs * m.com[0] - sn * m.com[1], ry = sn * m.com[0] + cs * m.com[1];   // centre of mass from the hull origin
    double jx = 0.0, jy = 0.0, jw = 0.0, m_power = 0.0, s_power = 0.0;
    if (a0 > 0.0) {
      m_power = (fmin(fmax(a0, 0.0), 1.0) + 1.0) * 0.5;
      const double ox = tipx * (4.0 / m.scale + 2.0 * d0) + sidex * d1;
      const double oy = -tipy * (4.0 / m.scale + 2.0 * d0) - sidey * d1;
      const double ix = -ox * m.main_power * m_power, iy = -oy * m.main_power * m_power;
      jx += ix; jy += iy;
      jw += (ox - rx) * iy - (oy - ry) * ix;
    }
    if (fabs(a1) > 0.5) {
      const double dir = a1 > 0.0 ? 1.0 : -1.0;
      s_power = fmin(fmax(fabs(a1), 0.5), 1.0);
      const double ox = tipx * d0 + sidex * (3.0 * d1 + dir * m.side_away / m.scale);
      const double oy = -tipy * d0 - sidey * (3.0 * d1 + dir * m.side_away / m.scale);
      const double ix = -ox * m.side_power * s_power, iy = -oy * m.side_power * s_power;
      const double px = ox - tipx * 17.0 / m.scale, py = oy + tipy * m.side_height / m.scale;   // from the hull origin
      jx += ix; jy += iy;
      jw += (px - rx) * iy - (py - ry) * ix;
    }
    bool game_over;
    lunar_move(m, s.q, s.v, jx, jy, jw, game_over);
    lunar_obs64(m, s.q, s.v, o);
    reward = (lunar_shaping(o) - before) - 0.30 * m_power - 0.03 * s_power;
    done = false;
    if (game_over || fabs(o[0]) >= 1.0) { done = true; reward = -100.0; }
    if (s.v[3] >= m.sleep_time) { done = true; reward = 100.0; }   // gym's order: `not lander.awake` is tested last
    finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) finite = finite && isfinite(s.q[i]) && isfinite(s.v[i]);
  }
};

__global__ __launch_bounds__(256) void k_lunar_step(const EnvStepArgs A, const LunarDev m) { lane_step_frame<LunarTask>(A, m); }
__global__ __launch_bounds__(256) void k_lunar_reset(const LaneResetArgs R, const LunarDev m) { lane_reset_frame<LunarTask>(R, m); }
