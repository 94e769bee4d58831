// goal_env.h — the goal env of ilsx_vecenv: a task of the lane-per-env frame.  It uses, by name, env_uniform (ilsx_env.hip) and
// lane_step_frame / lane_reset_frame and LaneStateQV (classic_env.h).
//
// PointReachTask is ilswiss_amd/her.py's PointReachEnv as a device stepper (the host class is its oracle): a 2-D
// point under velocity control must come within `tol` of a goal drawn at reset.  A STAND-IN for the reference's goal envs (gym's MuJoCo
// Fetch robots), not one of them.
//   state    qpos = (p_x, p_y, g_x, g_y) — the goal is episode state and lives in qpos, as the lander's terrain does —, qvel = (v_x, v_y);
//            float64
//   row      8 float32 columns: observation (p | v) | desired_goal (g) | achieved_goal (p) — the segment layout of ilsx_her_gather and
//            ilsx_her_sample; the policy reads the first 6 (observation | desired_goal), the record holds all 8
//   step     v = step_scale * clip(a, -1, 1) as numpy evaluates it for a float32 action: in float32, widened afterwards;
//            p = clip(p + v, -1, 1) in float64; reward -(|p - g| > tol) (sparse) or -|p - g| (dense) on float64; never done
//   reset    p = U(+-p_range)^2 from counters 0 and 1 of the env's Philox stream, v = 0, g = U(+-g_range)^2 from counters 2 and 3
#pragma once

struct GoalDev {
  double tol, p_range, g_range;
  float step_scale;
  int reward_kind;   // 0 sparse, 1 dense
};

struct PointReachTask {
  static constexpr int NQ = 4, NV = 2, O = 8, NA = 2;
  static constexpr int D_OBS = 4, D_GOAL = 2;
  static constexpr bool never_done = true;
  using Model = GoalDev;
  using State = LaneStateQV<4, 2>;

  static __device__ __forceinline__ void write_obs(const Model&, const State& s, float* dst) {
    dst[0] = (float)s.q[0]; dst[1] = (float)s.q[1]; dst[2] = (float)s.v[0]; dst[3] = (float)s.v[1];
    dst[4] = (float)s.q[2]; dst[5] = (float)s.q[3];
    dst[6] = (float)s.q[0]; dst[7] = (float)s.q[1];
  }
  static __device__ __forceinline__ void obs_before(const Model& m, const State& s, const float*, float* dst) { write_obs(m, s, dst); }

  static __device__ __forceinline__ void reset_state(const Model& m, uint64_t seed, uint32_t stream, unsigned long long step, uint32_t env, State& s) {
    s.q[0] = -m.p_range + (2.0 * m.p_range) * env_uniform(seed, stream, step, env, 0);
    s.q[1] = -m.p_range + (2.0 * m.p_range) * env_uniform(seed, stream, step, env, 1);
    s.q[2] = -m.g_range + (2.0 * m.g_range) * env_uniform(seed, stream, step, env, 2);
    s.q[3] = -m.g_range + (2.0 * m.g_range) * env_uniform(seed, stream, step, env, 3);
    s.v[0] = 0.0; s.v[1] = 0.0;
  }

  static __device__ __forceinline__ void advance(const Model& m, State& s, const float (&act)[2], double& reward, bool& done, bool& finite) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      // np.clip on float32 (a NaN stays a NaN), the product in float32
      const float c = act[i] < -1.0f ? -1.0f : (act[i] > 1.0f ? 1.0f : act[i]);
      const double v = (double)(m.step_scale * c);
      const double p = s.q[i] + v;
      s.v[i] = v;
      s.q[i] = p < -1.0 ? -1.0 : (p > 1.0 ? 1.0 : p);
    }
    const double dx = s.q[0] - s.q[2], dy = s.q[1] - s.q[3];
    const double dist = sqrt(dx * dx + dy * dy);   // np.linalg.norm: sqrt of the sum of squares
    reward = m.reward_kind == 0 ? (dist > m.tol ? -1.0 : -0.0) : -dist;
    done = false;
    finite = isfinite(s.q[0]) && isfinite(s.q[1]) && isfinite(s.v[0]) && isfinite(s.v[1]);
  }
};

__global__ __launch_bounds__(256) void k_goal_step(const EnvStepArgs A, const GoalDev m) { lane_step_frame<PointReachTask>(A, m); }
__global__ __launch_bounds__(256) void k_goal_reset(const LaneResetArgs R, const GoalDev m) { lane_reset_frame<PointReachTask>(R, m); }
