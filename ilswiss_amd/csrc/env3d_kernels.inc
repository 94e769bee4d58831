// env3d_kernels.inc — the two kernels of the 3-D stepper (wave-per-env step / reset), included by ilsx_env.hip once per observation
// layout: E3K(name) names the kernels, E3K_TRUNC is e3w_observe's TRUNC (0: the full observation, kernels k_env3dw_*; 1: qpos[2:] | qvel
// of the *_trunc_obs tasks, kernels k_env3dw_*_trunc).  Two inclusions of one text rather than one templated body: the full-observation
// kernels compile to the instructions they had before the truncated tasks existed.  (The lane-per-env kernels were removed: DESIGN §27.)
template <int NV>
__global__ __launch_bounds__(64) void E3K(k_env3dw_step)(const EnvStepArgs A, const Spatial3Dev* mp) {
  extern __shared__ __attribute__((aligned(16))) double e3w_smem[];
  e3w_lds* S = (e3w_lds*)e3w_smem;
  const Spatial3Dev& m = *mp;
  const int t = blockIdx.x, lane = threadIdx.x;
  const int env = A.ids ? A.ids[t] : t, n_env = A.n_env;
  if (A.frozen && A.frozen[env]) return;
  const int o = m.obs_dim, na = m.n_act;
  E3W_FOR(i, m.nq) S[E3WOff::Q0 + i] = A.qpos[(size_t)i * n_env + env];
  E3W_FOR(i, m.nv) S[E3WOff::V0 + i] = A.qvel[(size_t)i * n_env + env];
  float* rec = nullptr;
  if (A.replay) {   // fused replay insert: the observation the policy acted on is the stored current observation
    long long slot = A.top + env;
    if (slot >= A.cap) slot -= A.cap;
    rec = A.stage ? A.stage + ((size_t)env * A.stage_len + A.ep_len[env]) * A.rec : A.replay + (size_t)slot * A.rec;
    E3W_FOR(i, o) rec[i] = A.obs_cur[(size_t)env * o + i];
  }
  E3W_SYNC();
  E3WRegs regs[1];
  e3w_regs_init(regs[0], m, lane);
  e3w_regs_pin(regs[0]);
  double reward; bool done;
  e3w_task_step<NV>(S, m, lane, regs, A.act + (size_t)t * na, reward, done);
  bool end = false; int len = 0; double ret = 0.0;
  if (A.auto_reset) {
    len = A.ep_len[env] + 1; ret = A.ep_ret[env] + reward;
    bool finite = isfinite(reward);
    end = (done && !A.no_terminal) || len >= A.max_path_length || !finite;   // see envg_step_dev: no_terminal keeps stepping an unhealthy env
  }
  float* obs_out = A.obs ? A.obs + (size_t)t * o : nullptr;
  float* cur = (A.obs_cur && !end) ? A.obs_cur + (size_t)env * o : nullptr;
  float* rnext = rec ? rec + o + na + 2 : nullptr;
  e3w_observe<E3K_TRUNC>(S, m, lane, [&](int i, double val) {
    const float f = (float)((val - m.obs_shift[i]) * m.obs_inv_scale[i]);
    if (obs_out) obs_out[i] = f;
    if (cur) cur[i] = f;
    if (rnext) rnext[i] = f;
  });
  if (lane == 0) {
    if (A.rew) A.rew[t] = (float)reward;
    if (A.done) A.done[t] = done ? 1 : 0;
  }
  if (rec) {
    const float* ra = A.rec_act ? A.rec_act : A.act;
    E3W_FOR(k, na) rec[o + k] = ra[(size_t)t * na + k];
    if (lane == 0) {
      rec[o + na] = (float)reward;
      rec[o + na + 1] = (done && !A.no_terminal) ? 1.0f : 0.0f;
      rec[2 * o + na + 2] = 0.0f; rec[2 * o + na + 3] = 0.0f;
    }
  }
  if (A.auto_reset) {
    if (end) {
      if (lane == 0) { atomicAdd(&A.stats[0], 1.0); atomicAdd(&A.stats[1], ret); }
      E3W_SYNC();
      e3w_reset_state(S, m, lane, A.seed, A.stream, A.step, (uint32_t)env);
      e3w_kinematics(S, m, lane, regs, E3WOff::Q0, E3WOff::V0);
      float* c2 = A.obs_cur + (size_t)env * o;
      e3w_observe<E3K_TRUNC>(S, m, lane, [&](int i, double val) { c2[i] = (float)((val - m.obs_shift[i]) * m.obs_inv_scale[i]); });
    }
    if (lane == 0) {
      A.ep_len[env] = end ? 0 : len; A.ep_ret[env] = end ? 0.0 : ret;
      if (A.flush_len) A.flush_len[env] = end ? (len | ((done && !A.no_terminal) ? (1 << 30) : 0)) : 0;
    }
  }
  E3W_FOR(i, m.nq) A.qpos[(size_t)i * n_env + env] = S[E3WOff::Q0 + i];
  E3W_FOR(i, m.nv) A.qvel[(size_t)i * n_env + env] = S[E3WOff::V0 + i];
}

__global__ __launch_bounds__(64) void E3K(k_env3dw_reset)(const Spatial3Dev* mp, double* qpos, double* qvel, int n_env, const int* ids, float* obs,
                                                     float* obs_cur, int* ep_len, double* ep_ret, uint64_t seed, uint32_t stream,
                                                     unsigned long long step) {
  extern __shared__ __attribute__((aligned(16))) double e3w_smem[];
  e3w_lds* S = (e3w_lds*)e3w_smem;
  const Spatial3Dev& m = *mp;
  const int t = blockIdx.x, lane = threadIdx.x;
  const int env = ids ? ids[t] : t;
  e3w_reset_state(S, m, lane, seed, stream, step, (uint32_t)env);
  E3WRegs regs[1];
  e3w_regs_init(regs[0], m, lane);
  e3w_regs_pin(regs[0]);
  e3w_kinematics(S, m, lane, regs, E3WOff::Q0, E3WOff::V0);
  const int o = m.obs_dim;
  e3w_observe<E3K_TRUNC>(S, m, lane, [&](int i, double val) {
    const float f = (float)((val - m.obs_shift[i]) * m.obs_inv_scale[i]);
    if (obs) obs[(size_t)t * o + i] = f;
    if (obs_cur) obs_cur[(size_t)env * o + i] = f;
  });
  if (lane == 0) { ep_len[env] = 0; ep_ret[env] = 0.0; }
  E3W_FOR(i, m.nq) qpos[(size_t)i * n_env + env] = S[E3WOff::Q0 + i];
  E3W_FOR(i, m.nv) qvel[(size_t)i * n_env + env] = S[E3WOff::V0 + i];
}
