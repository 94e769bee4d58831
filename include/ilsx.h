/* ilsx.h — C ABI of libilsx.so, the MI355X (gfx950) engine behind ILSwiss's hot path.
 *
 * The reference (Ericonaldo/ILSwiss) is pure Python and has no FFI; the boundary this library sits
 * behind is the set of duck-typed Python interfaces its training loop calls.  Each
 * entry point below names the reference interface (file:line under /root/reference) whose arithmetic
 * it replaces; ilswiss_amd/*.py binds them with ctypes and re-exposes the reference's class/method
 * names.  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - return value: 0 = OK, <0 = ilsx_status; text via ilsx_last_error() (thread-local). No C++
 *     exception crosses the ABI.
 *   - pointers are DEVICE pointers on the ctx's GPU unless the name/flag says host.
 *   - caller owns every input/output buffer; the library owns what *_create returned until *_destroy.
 *   - a ctx is bound to one HIP stream; calls are asynchronous on that stream unless they return
 *     host-visible values (stats, sizes), in which case they synchronise the stream themselves.
 *   - flat parameter layout of a network ("torch parameters() order", rlkit/torch/common/networks.py:57-83,
 *     policies.py:231-239): fc0.W[H,in] row-major | fc0.b[H] | fc1.W[H,H] | fc1.b[H] | ... |
 *     head0.W[out,H] | head0.b[out] [| head1.W[out,H] | head1.b[out]]      (y = x W^T + b).
 *   - stochastic entry points take optional explicit noise / indices (parity mode) and otherwise use
 *     counter-based Philox4x32-10 keyed by (ctx seed, stream id, step counter).
 */
#ifndef ILSX_H
#define ILSX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILSX_ABI_VERSION 1

typedef enum {
  ILSX_OK = 0,
  ILSX_ERR_ARG = -1,      /* bad argument / shape */
  ILSX_ERR_HIP = -2,      /* a HIP runtime call failed */
  ILSX_ERR_NOMEM = -3,
  ILSX_ERR_STATE = -4,    /* call not valid in the object's current state */
  ILSX_ERR_UNSUPPORTED = -5
} ilsx_status;

typedef struct ilsx_ctx ilsx_ctx;
typedef struct ilsx_net ilsx_net;
typedef struct ilsx_replay ilsx_replay;
typedef struct ilsx_sac ilsx_sac;
typedef struct ilsx_sac_group ilsx_sac_group;
typedef struct ilsx_vecenv ilsx_vecenv;
typedef struct ilsx_disc ilsx_disc;
typedef struct ilsx_ppo ilsx_ppo;
typedef struct ilsx_td3 ilsx_td3;
typedef struct ilsx_ddpg ilsx_ddpg;
typedef struct ilsx_sacv ilsx_sacv;
typedef struct ilsx_bc ilsx_bc;
typedef struct ilsx_dsac ilsx_dsac;
typedef struct ilsx_dqn ilsx_dqn;

enum { ILSX_ACT_RELU = 0, ILSX_ACT_TANH = 1 };

/* ---------------------------------------------------------------- context */
int ilsx_abi_version(void);
const char* ilsx_last_error(void);
/* stream: an existing hipStream_t to run on (e.g. torch's current stream), or NULL to create one. */
int ilsx_ctx_create(int hip_device, void* hip_stream, uint64_t seed, ilsx_ctx** out);
int ilsx_ctx_sync(ilsx_ctx* ctx);
int ilsx_ctx_destroy(ilsx_ctx* ctx);
void* ilsx_ctx_stream(ilsx_ctx* ctx);
/* Every object that draws random numbers (vec env, replay ring, trainer, discriminator) takes the ctx's next Philox stream id when it is
   created.  Reads the cursor into *current (nullable) and, when set_to > 0, moves it: an object built on ANOTHER ctx of the same run (the eval
   env of rl_alg_params.eval_async lives on a stream of its own) can then take the id it would have had on this one, and this ctx skips it, so
   the run's other objects keep their streams.  The reference has one global torch / numpy generator per process (no counterpart). */
int ilsx_ctx_rng_stream_cursor(ilsx_ctx* ctx, uint32_t set_to, uint32_t* current);
/* Device scratch owned by the ctx (freed with it); used by the Python adapters for staging. */
int ilsx_ctx_alloc(ilsx_ctx* ctx, size_t bytes, void** out);
int ilsx_ctx_free(ilsx_ctx* ctx, void* ptr);
int ilsx_memcpy_h2d(ilsx_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int ilsx_memcpy_d2h(ilsx_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* syncs */

/* ---------------------------------------------------------------- split-run communicator
 * The path's ONE exchange step: when a single run is split over G GPUs (one process / ctx per GPU, every rank a full
 * replica of the parameters, B/G rows of the batch each, mean-loss gradients pre-scaled by 1/(B*G) through
 * ilsx_sac_cfg.grad_world), the flat gradient arena is all-reduced (sum) between backward and the optimiser step.  No
 * reference counterpart (run_experiment.py:57-78 runs independent processes only).  The collective is RCCL's
 * ncclAllReduce enqueued on the ctx stream; librccl.so.1 is dlopen'ed at the first call here.  Rank 0 draws the id, the
 * host program carries its 128 bytes to the other ranks (file, socket, torch.distributed — ilswiss_amd/parallel.py), then
 * every rank calls ilsx_comm_init.  With a communicator of grad_world ranks on the ctx, ilsx_sac_train_step and
 * ilsx_sac_train_from_replay run critic-backward -> all-reduce -> critic Adam+Polyak -> actor-backward -> all-reduce
 * (alpha gradient in the same message) -> actor Adam, all stream-ordered, no host synchronisation. */
#define ILSX_COMM_ID_BYTES 128
int ilsx_comm_unique_id(uint8_t* id_host /* [ILSX_COMM_ID_BYTES] */);
int ilsx_comm_init(ilsx_ctx* ctx, const uint8_t* id_host, int n_ranks, int rank);
int ilsx_comm_destroy(ilsx_ctx* ctx);
int ilsx_comm_info(const ilsx_ctx* ctx, int* n_ranks, int* rank);   /* 0 ranks = no communicator */
int ilsx_comm_allreduce_sum(ilsx_ctx* ctx, float* dev_buf, size_t n);   /* in place, on the ctx stream */

/* ---------------------------------------------------------------- kernel timing (bench.py roofline leg)
 * When enabled, every launch of a library kernel carries a start / stop hipEvent stamped with the dispatch's own
 * begin / end time (hipExtLaunchKernelGGL — the interval rocprofv3's kernel trace reports; the graph path is
 * bypassed while profiling); ilsx_prof_read synchronises and returns launches + summed ms of a slot,
 * ilsx_prof_kernel the source spelling of the kernel last launched under it (several kernels share a slot:
 * the column-split and the generic MLP kernels). */
enum { ILSX_K_MLP_FWD = 0, ILSX_K_MLP_BWD_DX = 1, ILSX_K_MLP_BWD_DW = 2, ILSX_K_ADAM = 3,
       ILSX_K_REPLAY_SAMPLE = 4, ILSX_K_REPLAY_ADD = 5, ILSX_K_REPLAY_SAMPLE_MANY = 6, ILSX_K_SAC_STATS = 7,
       ILSX_K_SAC_FINISH = 8, ILSX_K_ENV_STEP = 9, ILSX_K_POLICY_FINISH = 10, ILSX_K_DISC_BWD = 11, ILSX_K_PPO_GAE = 12,
       ILSX_K_SAC_PHASE_A = 13, ILSX_K_SAC_PHASE_C = 14,   /* the merged phase launches of the single-run SAC step */
       ILSX_K_COUNT = 16 };
int ilsx_prof_enable(ilsx_ctx* ctx, int on);
int ilsx_prof_reset(ilsx_ctx* ctx);
int ilsx_prof_read(ilsx_ctx* ctx, int kernel_id, uint64_t* launches, double* total_ms);
const char* ilsx_prof_kernel(ilsx_ctx* ctx, int kernel_id);
const char* ilsx_kernel_name(int kernel_id);
/* debugging aid (tools/step_gantt.py): while a trace buffer is set, thread 0 of EVERY workgroup of every MLP forward /
 * backward / weight-gradient launch writes its phase timestamps (100 MHz constant clock) into
 * dev_trace[launch][2048 workgroups][8 slots] (uint64; launch = order of launch since the buffer was set, at most
 * max_launches; slot 0 = workgroup start, 7 = end, 1..3 = phase boundaries).  NULL = off; launches_so_far (nullable)
 * receives the number of launches recorded into the PREVIOUS buffer. */
int ilsx_debug_set_stamp_buffer(ilsx_ctx* ctx, void* dev_trace, int max_launches, int* launches_so_far);
/* Host arithmetic only (no device needed): how a weight-gradient launch over `rows` batch rows is cut into row ranges (`big` != 0: the
 * large-batch block kernel).  Every range is non-empty and a whole number of the kernel's row steps; together they cover [0, rows).
 * The reference has no counterpart (torch.autograd sums the batch in one GEMM, e.g. ppo.py:145-153): test hook for the split plan. */
int ilsx_debug_dw_split(int rows, int big, int* splits, int* rows_per_split);

/* ---------------------------------------------------------------- networks
 * Replaces rlkit/torch/common/networks.py:23-115 (Mlp / FlattenMlp) and the heads of
 * rlkit/torch/common/policies.py:191-345 (n_heads = 2: mean | log_std). */
typedef struct {
  int32_t in_dim;      /* FlattenMlp: sum of the concatenated input dims */
  int32_t n_hidden;    /* 1..3 hidden layers */
  int32_t hidden;      /* the width the kernels run at: 64, 128 or 256 */
  int32_t out_dim;     /* per head */
  int32_t n_heads;     /* 1 (Mlp) or 2 (Gaussian policy: last_fc, last_fc_log_std) */
  int32_t act;         /* ILSX_ACT_* hidden activation */
  int32_t hidden_sizes[3];   /* networks.py:23-60 takes ANY list of widths: hidden_sizes[l] = the logical width of hidden layer l, 1..hidden
                                (0 = hidden).  A layer narrower than `hidden` is embedded in the `hidden`-wide kernels as structural zeros:
                                units past its width have zero weights and bias, hence pre-activation 0, output 0 (relu and tanh), gradient 0,
                                and Adam / Polyak / L2 never move them — the padded network IS the hidden_sizes network.  Every flat parameter /
                                gradient / optimiser-state vector that crosses this ABI has the LOGICAL sizes (torch's parameters() order). */
} ilsx_mlp_cfg;

int ilsx_net_create(ilsx_ctx* ctx, const ilsx_mlp_cfg* cfg, ilsx_net** out);
/* ILSX_ERR_STATE (and the network stays alive) while an agent created around it exists: the agent's destroy writes through the
 * network to give it storage of its own back — destroy the agent first. */
int ilsx_net_destroy(ilsx_net* net);
int ilsx_net_num_params(const ilsx_net* net, size_t* out);
/* networks.py:57-83 + pytorch_util.py:20-29 init rule: hidden W ~ U(+-1/sqrt(out_features)),
 * hidden b = b_init, heads W,b ~ U(+-init_w); host RNG (splitmix64/xoshiro) seeded by `seed`. */
int ilsx_net_init(ilsx_net* net, uint64_t seed, float init_w, float b_init);
int ilsx_net_set_params(ilsx_net* net, const float* src, size_t n, int src_is_device);
int ilsx_net_get_params(const ilsx_net* net, float* dst, size_t n, int dst_is_device);
/* Mlp.forward (networks.py:85-101): x[rows,in_dim] -> y[rows, n_heads*out_dim] (raw head outputs). */
int ilsx_mlp_forward(ilsx_net* net, const float* x, int rows, float* y);
/* ReparamTanhMultivariateGaussianPolicy.get_actions / forward (policies.py:241-307):
 * obs[n,o] -> act[n,a]; deterministic: tanh(mean); else tanh(mean + std*eps), eps[n,a] or NULL=Philox.
 * logp (nullable) [n] receives log pi(a|s) (distributions.py:74-97). */
int ilsx_policy_act(ilsx_net* pi, const float* obs, int n, int deterministic, const float* eps,
                    float* act, float* logp);
/* ReparamTanhMultivariateNormal.log_prob with pre_tanh_value=None (policies.py:329-345):
 * logp[n] of GIVEN actions act[n,a] under pi(.|obs). */
int ilsx_policy_log_prob(ilsx_net* pi, const float* obs, const float* act, int n, float* logp);
/* Marks a single-head Mlp as MlpGaussianNoisePolicy (policies.py:130-188): ilsx_policy_act / ilsx_rollout_step then
 * return max_act*tanh(out) + clip(policy_noise*N(0,1), +-policy_noise_clip) (no noise when deterministic). */
int ilsx_net_set_noise_policy(ilsx_net* pi, float policy_noise, float policy_noise_clip, float max_act);
/* Output activation of a noise policy: 0 = tanh (what td3_exp_script.py:75 passes), 1 = identity (Mlp's default, networks.py:31:
 * action = max_act * last_fc(h) + clipped noise).  Set it before ilsx_td3_create adopts the network. */
int ilsx_net_set_output_linear(ilsx_net* pi, int linear);
/* Marks a single-head Mlp with n = out_dim outputs (2 <= n <= 64) as DiscretePolicy (policies.py:39-101): LogSoftmax over the last linear
 * layer.  ilsx_policy_act then writes the action INDEX as a float to act[n_rows][1] — stochastic: Gumbel-max argmax(z_j - log(-log u_j)), u
 * from Philox on the 'ACT' stream; deterministic: the first maximal log-probability — and logp (nullable) = log pi(a|s).  eps must be NULL.
 * on = 0 clears the mark.  Set it before a trainer adopts the network; continuous trainers refuse a categorical policy. */
int ilsx_net_set_categorical(ilsx_net* pi, int on);
/* Marks a single-head Mlp with n = out_dim outputs (2 <= n <= 64), neither categorical nor a noise policy, as ArgmaxDiscretePolicy(qf)
 * under EpsilonGreedy (rlkit/policies/argmax.py, rlkit/exploration_strategies/epsilon_greedy.py:21-24).  ilsx_policy_act then writes the
 * action INDEX as a float to act[n_rows][1] — deterministic: the first maximal output (numpy argmax); otherwise one Philox call per row on
 * the 'EGR' stream, keyed by (row, the ctx's act-call counter): u0 <= epsilon takes min(n - 1, floor(u1 * n)), a uniform action that may
 * coincide with the greedy one, anything else the argmax.  eps and logp must be NULL.  epsilon lies in [0, 1]; calling it again changes
 * epsilon; on = 0 clears the mark.  A marked network counts as a policy over a Discrete space (ilsx_rollout_step, ilsx_eval_rollout);
 * ilsx_dqn_create takes it marked or not, every other trainer refuses it. */
int ilsx_net_set_epsilon_greedy(ilsx_net* qf, int on, float epsilon);
/* DiscretePolicy.get_log_pis (policies.py:99-100) of a categorical policy: obs[n_rows,o] -> log_pis[n_rows,n] = log_softmax of the last
 * linear layer (max-shifted; device pointers). */
int ilsx_policy_log_pis(ilsx_net* pi, const float* obs, int n_rows, float* log_pis);

/* ---------------------------------------------------------------- replay buffer
 * Replaces rlkit/data_management/simple_replay_buffer.py:17-442 + env_replay_buffer.py:7-49.
 * HBM-resident ring of transition records (obs|act|rew|done|next_obs|absorbing, one 128-byte-aligned record per
 * transition).  Cursor semantics (_top/_size/_traj_endpoints) follow the reference exactly. */
int ilsx_replay_create(ilsx_ctx* ctx, int64_t capacity, int obs_dim, int act_dim, uint64_t seed,
                       ilsx_replay** out);
int ilsx_replay_destroy(ilsx_replay* rb);
/* n x add_sample (+ terminate_episode() after rows whose ep_end flag is set; simple_replay_buffer.py:78-132).
 * Row arrays are contiguous [n,dim]; `data_is_device` says where obs/act/rew/done/nobs live;
 * ep_end_host is a HOST array of n flags or NULL. */
int ilsx_replay_add(ilsx_replay* rb, const float* obs, const float* act, const float* rew,
                    const uint8_t* done, const float* nobs, int n, const uint8_t* ep_end_host,
                    int data_is_device);
int ilsx_replay_terminate_episode(ilsx_replay* rb);
/* _absorbing[cap,2] (simple_replay_buffer.py:66-67,91-92; the wrap_absorbing branch of add_path, :163-213): the flags of the n
 * slots from slot0 on (ring order) are set from HOST absorbing[n,2]; rows added without them hold [0,0].  get: device
 * idx int64[n] -> device absorbing[n,2] (the `absorbing` key of random_batch, :266-268). */
int ilsx_replay_set_absorbing(ilsx_replay* rb, int64_t slot0, int n, const float* absorbing_host);
int ilsx_replay_get_absorbing(ilsx_replay* rb, const int64_t* idx, int n, float* absorbing);
/* random_batch (simple_replay_buffer.py:239-293): idx (device int64[B]) or NULL = uniform with
 * replacement over [0,size) from Philox.  Outputs (device): obs[B,o] act[B,a] rew[B] done[B] (0/1 as
 * float, rlkit/torch/core.py:124-143) nobs[B,o]; idx_out (nullable device int64[B]) gets the rows used. */
int ilsx_replay_sample(ilsx_replay* rb, int B, const int64_t* idx, float* obs, float* act, float* rew,
                       float* done, float* nobs, int64_t* idx_out);
/* Bandwidth microbenchmark form of the same kernel: n_batches x B rows gathered in ONE launch into
 * out[n_batches*B, record] (device, record = ilsx_replay_record_floats()). */
int ilsx_replay_sample_many(ilsx_replay* rb, int n_batches, int B, float* out_records);
int ilsx_replay_record_floats(const ilsx_replay* rb, int* out);
/* Hindsight relabelling gather — HindsightReplayBuffer.random_batch (rlkit/data_management/relabel_replay_buffer.py:66-163) over a ring
 * whose observation segment is [observation (d_obs) | desired_goal (d_goal) | achieved_goal (d_goal)].  idx / idx_relabel: DEVICE int64[B]
 * (the sampled steps and their `future` / `final` relabel steps, drawn by the caller in the reference's RandomState order); the first
 * n_relabel rows get the relabel step's next achieved goal as desired goal (:106-113); relabel_on: every reward is recomputed from
 * (next achieved goal, desired goal) (:139-147) by gym's GoalEnv rule, reward_kind 0 = sparse -(dist > threshold), 1 = dense -dist.
 * Device outputs: obs_cat[B, d_obs + d_goal] = observation | desired_goal and nobs_cat likewise (what her/td3.py:95-99 and
 * her/sac.py:80-84 feed the networks), act[B, a], rew[B], done[B]. */
int ilsx_her_gather(ilsx_replay* rb, const int64_t* idx, const int64_t* idx_relabel, int B, int n_relabel, int relabel_on, int d_obs,
                    int d_goal, int reward_kind, float threshold, float* obs_cat, float* act, float* rew, float* done, float* nobs_cat);
/* The same batch with its indices DRAWN ON THE DEVICE, in one launch: draw, gather, relabel, reward, concatenation.  The ring keeps a
 * device mirror of its trajectory table (start, length per registered trajectory, in insertion order), uploaded again only after the table
 * changed.  Row b takes three uniforms (u0, u1, u2) in [0, 1): u = DEVICE float64 [B, 3], or NULL = Philox keyed by (the ring's seed, its
 * stream, its sample counter, b).  With floor(u n) taken in float64 and clamped to n - 1:
 *   t = floor(u0 n_traj), k = floor(u1 L_t), idx = (start_t + k) mod capacity;
 *   relabel_type 1 `future`: kf = k + floor(u2 (L_t - k)); 2 `final`: kf = L_t - 1; 0 none: kf = k (no goal is replaced, rewards stay);
 *   idx_relabel = (start_t + kf) mod capacity.
 * For a trajectory that does not wrap the ring this is the distribution of relabel_replay_buffer.py:71-94; for one that wraps, the
 * reference's randint(step, traj_len + start) draws from a wrong range or raises, while here the relabel step always lies in the same
 * trajectory at or after the sampled step.  The first n_relabel rows are relabelled (relabel_type != 0); outputs as ilsx_her_gather, bit for
 * bit what ilsx_her_gather(idx_out, idx_relabel_out, ...) writes; idx_out / idx_relabel_out: DEVICE int64[B], nullable.
 * ILSX_ERR_STATE: no registered trajectory.  ILSX_ERR_ARG: ring width != d_obs + 2 d_goal, n_relabel outside [0, B], relabel_type outside
 * {0, 1, 2}, reward_kind outside {0, 1}.  ILSX_ERR_UNSUPPORTED: act_dim > d_obs + d_goal (as ilsx_her_gather). */
int ilsx_her_sample(ilsx_replay* rb, int B, int n_relabel, int relabel_type, int d_obs, int d_goal, int reward_kind, float threshold,
                    const double* u, float* obs_cat, float* act, float* rew, float* done, float* nobs_cat, int64_t* idx_out,
                    int64_t* idx_relabel_out);
int ilsx_replay_size(ilsx_replay* rb, int64_t* size, int64_t* top);
int ilsx_replay_clear(ilsx_replay* rb);
/* _traj_endpoints in insertion order: writes up to max pairs (start,end) to HOST arrays; *n = count. */
int ilsx_replay_traj_endpoints(ilsx_replay* rb, int64_t* starts_host, int64_t* ends_host, int max, int* n);

/* ---------------------------------------------------------------- SAC (twin Q, auto alpha)
 * Replaces rlkit/torch/algorithms/sac/sac_alpha.py:21-76 (ctor kwargs == cfg fields) and
 * :78-181 (train_step), :245-247 (_update_target_network). */
typedef struct {
  float reward_scale, discount, policy_lr, qf_lr, alpha_lr, soft_target_tau, alpha;
  int32_t train_alpha;
  float policy_mean_reg_weight, policy_std_reg_weight, beta_1;
  int32_t has_target_entropy;  /* 0: default -dim(A)/2 (sac_alpha.py:56-58) */
  float target_entropy;
  int32_t max_batch;           /* largest B any train call will use (workspace size) */
  int32_t grad_world;          /* split-run mode: number of ranks sharing one batch (1 = off); the
                                  mean-over-batch scale becomes 1/(B*grad_world) */
} ilsx_sac_cfg;

typedef struct {              /* scalars of sac_alpha.py:186-233 for the step just taken */
  float qf1_loss, qf2_loss, policy_loss, alpha_loss, alpha;
  float q1_mean, q2_mean, log_pi_mean, policy_mu_mean, policy_log_std_mean;
  double log_alpha;
  /* Std / Max / Min of {Q1 Predictions, Q2 Predictions, Log Pis, Policy mu, Policy log std} (sac_alpha.py:202-233) */
  float ext_std[5], ext_max[5], ext_min[5];
} ilsx_sac_stats;

/* Takes over the storage of pi/q1/q2 (they become views into the agent's parameter arena and stay
 * valid for ilsx_policy_act / get_params until the agent is destroyed). */
int ilsx_sac_create(ilsx_ctx* ctx, const ilsx_sac_cfg* cfg, ilsx_net* pi, ilsx_net* q1, ilsx_net* q2,
                    ilsx_sac** out);
int ilsx_sac_destroy(ilsx_sac* sac);
/* One SoftActorCritic.train_step on an explicit batch (device pointers, fp32; rew/done are [B]).
 * eps_next / eps_cur: the two N(0,1) draws [B,a] (sac_alpha.py:102,142) or NULL = Philox. */
int ilsx_sac_train_step(ilsx_sac* sac, const float* obs, const float* act, const float* rew,
                        const float* done, const float* nobs, int B, const float* eps_next,
                        const float* eps_cur, ilsx_sac_stats* stats);
/* TorchRLAlgorithm._do_training (torch_rl_algorithm.py:28-34): n_steps x (random_batch + train_step)
 * with on-device sampling; one hipGraph replay per step, no host round trip.  stats (nullable): the statistics of the
 * FIRST batch of the call — the reference fills eval_statistics on the first train_step after end_epoch
 * (sac_alpha.py:185-190) and the caller passes `stats` exactly then. */
int ilsx_sac_train_from_replay(ilsx_sac* sac, ilsx_replay* rb, int n_steps, int B, ilsx_sac_stats* stats);
/* A single run's steps inside ilsx_sac_train_from_replay / ilsx_advirl_train run on merged "phase" kernels whose workgroups hand data to
 * each other inside one launch; that needs the GPU to this process.  The reference's launcher starts every worker of a sweep on the SAME
 * GPU (run_experiment.py:57-78), so the library checkpoints parameters / optimiser state / counters at the start of every such window
 * and, if a hand-off timed out or a row tile's workgroups were placed on two XCDs, rolls the window back and re-runs it on one launch
 * per stage (where the agent then stays): the caller sees the same updates either way.  This reports what happened:
 * fallbacks = windows rolled back so far, disabled = 1 once the agent has left the phase kernels, last_window_on_phase = 1 if the most
 * recent window used them, wgs_per_cu_a / _c = resident workgroups per CU the runtime's occupancy calculator gives the two kernels
 * (what the "every waited-for workgroup is resident" check is made with).  Every output nullable. */
int ilsx_sac_phase_state(ilsx_sac* sac, int* fallbacks, int* disabled, int* last_window_on_phase, int* wgs_per_cu_a, int* wgs_per_cu_c);
/* test aid: the next window behaves as if one of its hand-offs had timed out (exercises the roll-back path on an exclusive GPU) */
int ilsx_sac_debug_break_phase(ilsx_sac* sac);
/* Test aid (no device needed) for what the merged phase kernels fix at compile time (loss kind per stage, one head output per critic, slab
 * counts, the tanh-Gaussian epilogue, no explicit noise, no policy finished in phase C): 1 if a phase launch (stage 0 = A, 1 = C) takes
 * descriptors with these properties, 0 if it refuses them.  flags: 1 = explicit noise for the epilogue, 2 = phase C's stage 1 finishes a policy. */
int ilsx_debug_phase_static_ok(int stage, int loss_critic, int loss_policy, int no_critic, int slabs, int fin_head, int a, int H, int cs, int flags);
/* Split-run (multi-GPU) phases: train_step == critic_backward ; critic_update ; actor_backward ;
 * actor_update, with an all-reduce(sum) of the gradient arena between backward and update. */
int ilsx_sac_set_batch(ilsx_sac* sac, const float* obs, const float* act, const float* rew,
                       const float* done, const float* nobs, int B, const float* eps_next,
                       const float* eps_cur);
int ilsx_sac_critic_backward(ilsx_sac* sac);
int ilsx_sac_critic_update(ilsx_sac* sac);
int ilsx_sac_actor_backward(ilsx_sac* sac);
int ilsx_sac_actor_update(ilsx_sac* sac);
/* The statistics most recently asked for (a train call with `stats` / a grouped call with want_stats), as they stood right after their
 * step; after hand-driven phases: the device scalars as they are now. */
int ilsx_sac_last_stats(ilsx_sac* sac, ilsx_sac_stats* stats);
/* flat fp32 views: which = 0 pi, 1 q1, 2 q2, 3 target_q1, 4 target_q2 */
int ilsx_sac_get_params(ilsx_sac* sac, int which, float* dst, size_t n, int dst_is_device);
int ilsx_sac_set_params(ilsx_sac* sac, int which, const float* src, size_t n, int src_is_device);
/* gradients of the last backward, same layout/which as the parameters (0 pi, 1 q1, 2 q2) */
int ilsx_sac_get_grads(ilsx_sac* sac, int which, float* dst, size_t n, int dst_is_device);
/* gradient arena for the RCCL all-reduce: segment 0 = critics (q1|q2), 1 = actor (pi | alpha slot) */
int ilsx_sac_grads_ptr(ilsx_sac* sac, int segment, float** dev_ptr, size_t* n);
int ilsx_sac_get_log_alpha(ilsx_sac* sac, double* out);
int ilsx_sac_set_log_alpha(ilsx_sac* sac, double v);
/* optimiser state for snapshots (sac_alpha.py:249-273): which = 0 pi, 1 q1, 2 q2; m,v host fp32[n] */
int ilsx_sac_get_adam(ilsx_sac* sac, int which, float* m_host, float* v_host, size_t n, int64_t* t);
int ilsx_sac_set_adam(ilsx_sac* sac, int which, const float* m_host, const float* v_host, size_t n, int64_t t);
/* alpha_optimizer state (float64 scalar Adam, sac_alpha.py:74-76) + the Philox step counter */
int ilsx_sac_get_alpha_opt(ilsx_sac* sac, double* m, double* v, int64_t* t, uint64_t* rng_step);
int ilsx_sac_set_alpha_opt(ilsx_sac* sac, double m, double v, int64_t t, uint64_t rng_step);

/* Parity aids for the fused path (tests only; nothing in the training path calls them).
 * ilsx_sac_debug_batch re-derives, with the STANDALONE sample kernel (the one behind ilsx_replay_sample) and a
 * standalone Philox kernel, the batch rows and the two N(0,1) draws that gradient step number `step` of this agent
 * takes when it samples from `rb` inside ilsx_sac_train_from_replay / ilsx_sac_group_train_from_replay (`step` = the
 * agent's Philox step counter when that step runs: 0 for a fresh agent's first step; ilsx_sac_get_alpha_opt's
 * rng_step is the counter of the NEXT step).  All outputs are device pointers: obs[B,o] act[B,a] rew[B] done[B]
 * nobs[B,o] eps_next[B,a] eps_cur[B,a] idx int64[B]; every one nullable.
 * ilsx_sac_debug_last_batch copies what the LAST step actually used out of the agent's workspace: the rows its first
 * forward launch gathered and published (obs/act/rew/done/nobs) and the eps_cur its policy head consumed. */
int ilsx_sac_debug_batch(ilsx_sac* sac, ilsx_replay* rb, uint64_t step, int B, float* obs, float* act, float* rew,
                         float* done, float* nobs, float* eps_next, float* eps_cur, int64_t* idx);
int ilsx_sac_debug_last_batch(ilsx_sac* sac, int B, float* obs, float* act, float* rew, float* done, float* nobs,
                              float* eps_cur);
/* Known-answer aid (tests only): device raw[n_rows*4] = the Philox4x32-10 block of counter (row, 0, step lo, step hi ^ stream*0x9E3779B9)
 * under key (seed lo, seed hi ^ stream); device normals[n_rows*a] = the N(0,1) draws every stochastic policy epilogue of the library
 * makes for (seed, step, stream, row, dim).  Either output nullable. */
/* kind: 0 = ilsx_replay, 1 = ilsx_sac (its two streams are id, id + 1: eps_next, eps_cur), 2 = ilsx_disc.  The Philox stream id the
 * object was given at creation (ids are handed out per ctx in creation order) and the seed its draws are keyed by. */
int ilsx_debug_rng_stream(const void* object, int kind, uint32_t* stream, uint64_t* seed);
int ilsx_debug_philox(ilsx_ctx* ctx, uint64_t seed, uint64_t step, uint32_t stream, int n_rows, int a, uint32_t* raw, float* normals);
/* Leak check aid (tests only): the number of device allocations the context holds right now. */
int ilsx_debug_ctx_allocs(ilsx_ctx* ctx, size_t* count);

/* ---------------------------------------------------------------- adversarial-IRL discriminator
 * Replaces rlkit/torch/algorithms/adv_irl/disc_models/simple_disc_models.py:8-48 (MLPDisc, with and without batch norm),
 * AdvIRL._do_reward_training (adv_irl.py:133-216: BCE-with-logits on [expert; policy] + WGAN-GP gradient
 * penalty, the double backward derived by hand) and the reward modes of _do_policy_training (:277-298).
 * cfg fields == the YAML keys (exp_specs/gail/gail_walker.yaml:24-28,55-59). */
enum { ILSX_DISC_AIRL = 0, ILSX_DISC_GAIL = 1, ILSX_DISC_GAIL2 = 2, ILSX_DISC_FAIRL = 3 };
typedef struct {
  int32_t obs_dim, act_dim;       /* discriminator input = cat(obs, act); state_only: cat(obs, next_obs), act_dim == obs_dim */
  int32_t hid_dim, hid_act;       /* layer blocks of hid_dim (64/128/256), ILSX_ACT_* */
  int32_t use_grad_pen;
  float clamp_magnitude, disc_lr, disc_momentum, grad_pen_weight;
  int32_t max_batch;              /* disc_optim_batch_size upper bound (rows per class) */
  int32_t state_only;             /* adv_irl.py:140-162,269: discriminator input = cat(obs, next_obs); act_dim must equal obs_dim and
                                     every `act` row pointer of the entry points below carries next_obs rows */
  int32_t num_layer_blocks;       /* simple_disc_models.py:11,29-39: hidden (Linear, act) blocks, 1..3; 0 = 2.  2 runs the fused
                                     double-backward kernel, 1 and 3 the same mathematics as a chain of per-layer launches */
  int32_t use_bn;                 /* simple_disc_models.py:15,30-31,36-37 (the constructor's default): every block is Linear -> BatchNorm1d ->
                                     act.  Train mode in both forwards of a step (cross-entropy rows and penalty interpolates, each with its
                                     own batch statistics, running statistics updated by both), the penalty's double backward through the
                                     batch statistics; ilsx_disc_reward uses the running statistics (eval mode, adv_irl.py:268-274).  Any
                                     hid_dim; parameters in torch's order: per block W | b | gamma | beta, then the output layer.  A chain of
                                     simple launches (csrc/disc_bn.h), not the fused MFMA kernels of use_bn = 0 */
  int32_t grad_world;             /* split-run mode (SURVEY section 8e "Disc: same"; 0 / 1 = off): this rank holds B / G rows per class (and B / G
                                     interpolates); the cross-entropy and penalty means are over B * G rows, the gradient arena is all-reduced
                                     (sum) on the ctx's communicator before Adam; the logged statistics are this rank's rows'.  use_bn = 1 is
                                     refused (batch statistics would have to cross ranks) */
} ilsx_disc_cfg;
typedef struct { float ce_loss, grad_pen, accuracy; } ilsx_disc_stats;   /* "Disc CE Loss", "Grad Pen", "Disc Acc" */
int ilsx_disc_create(ilsx_ctx* ctx, const ilsx_disc_cfg* cfg, ilsx_disc** out);
int ilsx_disc_destroy(ilsx_disc* disc);
int ilsx_disc_num_params(const ilsx_disc* disc, size_t* out);
/* flat layout: fc0.W | fc0.b | fc1.W | fc1.b | out.W | out.b (nn.Sequential parameters() order); HOST arrays */
int ilsx_disc_set_params(ilsx_disc* disc, const float* src_host, size_t n);
int ilsx_disc_get_params(ilsx_disc* disc, float* dst_host, size_t n);
int ilsx_disc_get_grads(ilsx_disc* disc, float* dst_host, size_t n);
/* use_bn discriminators: the BatchNorm running statistics (module buffers, not parameters: snapshots carry them beside the parameters),
 * HOST arrays [num_layer_blocks * hid_dim] each, block-major */
int ilsx_disc_get_bn_stats(ilsx_disc* disc, float* running_mean_host, float* running_var_host, size_t n);
int ilsx_disc_set_bn_stats(ilsx_disc* disc, const float* running_mean_host, const float* running_var_host, size_t n);
/* one _do_reward_training step; inputs are device rows exp_obs[B,o] exp_act[B,a] pol_obs[B,o] pol_act[B,a];
 * eps (device [B], U[0,1) interpolation weights) or NULL = Philox. */
int ilsx_disc_train_step(ilsx_disc* disc, const float* exp_obs, const float* exp_act, const float* pol_obs,
                         const float* pol_act, int B, const float* eps, ilsx_disc_stats* stats);
/* reward relabelling: rew[n] (nullable) by mode + optional clip; logits[n] (nullable) = clamped D(s,a) */
int ilsx_disc_reward(ilsx_disc* disc, const float* obs, const float* act, int n, int mode, int has_min, float rew_clip_min,
                     int has_max, float rew_clip_max, float* rew, float* logits);

/* ---------------------------------------------------------------- co-resident seeds
 * The reference runs a seed sweep as independent processes (run_experiment.py:57-78).  A group steps K independent
 * SoftActorCritic agents of identical shape in lock-step on ONE GPU: every stage of the fused step is one launch whose grid
 * carries all agents' tasks ("grouped GEMMs, weights differ per seed"), so K runs cost 9 dependent launches per step
 * instead of 9K.  The agents stay ordinary ilsx_sac objects (parameters, statistics, snapshots through their own entry
 * points); results are bit-identical to stepping each agent alone with ilsx_sac_train_from_replay. */
int ilsx_sac_group_create(ilsx_ctx* ctx, ilsx_sac* const* agents, int n_agents, ilsx_sac_group** out);
int ilsx_sac_group_destroy(ilsx_sac_group* group);
/* n_steps gradient steps of every agent; agent k samples its batch from rbs[k].  want_stats: the FIRST step of the call also
 * computes every agent's statistics (sac_alpha.py:185-190; read them with ilsx_sac_last_stats).
 * The agents may live in sibling contexts of the group's ctx — contexts created on the SAME device and HIP stream
 * (ilsx_ctx_create(device, ilsx_ctx_stream(ctx), seed_k, ...)): each run then keeps the Philox key and per-object stream ids it would have in a
 * process of its own, which is what makes K grouped seeds reproduce K single-process runs (run_experiment.py --group). */
int ilsx_sac_group_train_from_replay(ilsx_sac_group* group, ilsx_replay* const* rbs, int n_steps, int B, int want_stats);

/* AdvIRL._do_training (adv_irl.py:126-131) for one train call: `loops` x { disc_updates discriminator steps ;
 * policy_updates SAC steps on rewards relabelled by the discriminator (mode / clips as ilsx_disc_reward) }, every batch
 * drawn on the device from the expert / policy replay rings (get_batch, :106-113).  Statistics (all nullable, host) are
 * those of the first discriminator / policy batch of the call; rew_stats4 = {Mean, Std, Max, Min} of its rewards. */
int ilsx_advirl_train(ilsx_disc* disc, ilsx_sac* policy_trainer, ilsx_replay* expert_rb, ilsx_replay* policy_rb, int loops,
                      int disc_updates, int policy_updates, int disc_batch, int policy_batch, int mode, int has_min,
                      float rew_clip_min, int has_max, float rew_clip_max, ilsx_disc_stats* disc_stats,
                      ilsx_sac_stats* sac_stats, float* rew_stats4);
/* policy_optim_batch_size_from_expert (adv_irl.py:239-255): the last n_from_expert rows of every policy batch are drawn from the
 * expert ring (torch.cat([policy rows, expert rows])), relabelled and trained on like the others.  0 (default) = off. */
int ilsx_advirl_set_policy_batch_from_expert(ilsx_disc* disc, int n_from_expert);

/* ---------------------------------------------------------------- TD3
 * Replaces rlkit/torch/algorithms/td3/td3.py:21-70 (ctor), :72-124 (train_step), :180-183 (soft updates).  cfg fields ==
 * the YAML keys of exp_specs/td3/td3_hopper.yaml:12-13,39-45 (policy_noise / policy_noise_clip are the noise of the
 * policy MODULE, which the target policy inherits through policy.copy(); td3.py's target_policy_noise* are unused).
 * The value list of a statistic is {Mean, Std, Max, Min} (core/eval_util.py create_stats_ordered_dict). */
typedef struct {
  float reward_scale, discount, policy_lr, qf_lr;
  int32_t policy_and_target_update_period;
  float soft_target_tau, policy_noise, policy_noise_clip, max_act;
  int32_t max_batch;
  /* her != 0: rlkit/torch/algorithms/her/td3.py (goal-conditioned TD3; the caller concatenates observation | desired_goal): target
   * action = clamp(policy_noise * N(0,1), -max_act, max_act) as that file computes it (:104-114), target value clipped to
   * [clip_return_l, clip_return_r] (:116-122; defaults -1/(1-discount), 0 are the caller's to fill), policy loss + mean(a^2) (:148-152) */
  int32_t her;
  float clip_return_l, clip_return_r;
} ilsx_td3_cfg;
typedef struct {
  float qf1_loss, qf2_loss, policy_loss;
  float q1_pred[4], q2_pred[4], q_target[4], bellman1[4], bellman2[4], policy_action[4];
} ilsx_td3_stats;
/* adopts the three networks' storage like ilsx_sac_create; pi: single-head Mlp (becomes a noise policy) */
int ilsx_td3_create(ilsx_ctx* ctx, const ilsx_td3_cfg* cfg, ilsx_net* pi, ilsx_net* qf1, ilsx_net* qf2, ilsx_td3** out);
int ilsx_td3_destroy(ilsx_td3* td3);
/* device batch rows as in ilsx_sac_train_step; eps_target: device [B,a] N(0,1) draws of the target policy's noise
 * (policies.py:182-184) or NULL = Philox; stats nullable (host). */
int ilsx_td3_train_step(ilsx_td3* td3, const float* obs, const float* act, const float* rew, const float* done,
                        const float* nobs, int B, const float* eps_target, ilsx_td3_stats* stats);
int ilsx_td3_train_from_replay(ilsx_td3* td3, ilsx_replay* rb, int n_steps, int B, ilsx_td3_stats* stats);
/* which: 0 qf1, 1 qf2, 2 policy, 3 target_qf1, 4 target_qf2, 5 target_policy; HOST flat arrays */
int ilsx_td3_get_params(ilsx_td3* td3, int which, float* dst_host, size_t n);
int ilsx_td3_set_params(ilsx_td3* td3, int which, const float* src_host, size_t n);

/* ---------------------------------------------------------------- DDPG
 * Replaces rlkit/torch/algorithms/ddpg/ddpg.py:21-100 (ctor), :102-226 (train_step), :228-235 (target updates).  pi: a single-head Mlp
 * with tanh or identity output (ilsx_net_set_output_linear), adopted as a noise policy with noise 0 (policies.py:106-127 MlpPolicy);
 * qf: one single-output FlattenMlp.  `discount` is a field here because the reference reads self.discount without ever setting it.
 * Policy loss -mean(Q(s, pi(s))) + policy_pre_activation_weight * mean_rows(sum_cols(pre^2)); target clamp(r + (1-d) * discount *
 * Q_tgt(s', pi_tgt(s')), min_q_value, max_q_value) (+-inf allowed); critic loss MSE + qf_weight_decay * sum ||W||^2 over the critic's
 * weight matrices (biases excluded, core.py:62-72).  Both gradients are taken at the pre-update parameters.  Targets: Polyak with
 * soft_target_tau when use_soft_update, else a hard copy on the steps whose counter (tested before its increment, one per train step)
 * is a multiple of target_update_period — the first step copies. */
typedef struct {
  float discount, policy_lr, qf_lr, qf_weight_decay, soft_target_tau;
  int32_t use_soft_update, target_update_period;
  float policy_pre_activation_weight, min_q_value, max_q_value, max_act;
  int32_t max_batch;
} ilsx_ddpg_cfg;
typedef struct {   /* ddpg.py:187-225; qf_loss includes the decay term */
  float qf_loss, policy_loss, raw_policy_loss, preactivation_policy_loss;
  float q_pred[4], q_target[4], bellman[4], policy_action[4];
} ilsx_ddpg_stats;
int ilsx_ddpg_create(ilsx_ctx* ctx, const ilsx_ddpg_cfg* cfg, ilsx_net* pi, ilsx_net* qf, ilsx_ddpg** out);
int ilsx_ddpg_destroy(ilsx_ddpg* ddpg);
int ilsx_ddpg_train_step(ilsx_ddpg* ddpg, const float* obs, const float* act, const float* rew, const float* done,
                         const float* nobs, int B, ilsx_ddpg_stats* stats);
int ilsx_ddpg_train_from_replay(ilsx_ddpg* ddpg, ilsx_replay* rb, int n_steps, int B, ilsx_ddpg_stats* stats);
/* which: 0 qf, 1 policy, 2 target_qf, 3 target_policy; HOST flat arrays */
int ilsx_ddpg_get_params(ilsx_ddpg* ddpg, int which, float* dst_host, size_t n);
int ilsx_ddpg_set_params(ilsx_ddpg* ddpg, int which, const float* src_host, size_t n);

/* ---------------------------------------------------------------- discrete SAC
 * Replaces rlkit/torch/algorithms/discrete_sac/discrete_sac.py:23-58 (ctor), :62-181 (train_step), :196-198 (soft updates).  pi: a
 * categorical policy (ilsx_net_set_categorical) of n outputs; qf1 / qf2: identical FlattenMlp's obs -> n.  Batches carry the action INDEX
 * as a float in a 1-wide action column.  Fixed alpha (the reference has no automatic tuning); Adam betas (beta_1, 0.999) for all three
 * optimisers.  Statistics are those of the first batch of a call (discrete_sac.py:149-151). */
typedef struct {
  float discount, reward_scale, alpha, soft_target_tau, policy_lr, qf_lr, beta_1;
  int32_t max_batch;
} ilsx_dsac_cfg;
typedef struct {
  float qf1_loss, qf2_loss, policy_loss;
  float q1_pred[4], q2_pred[4];   /* {Mean, Std, Max, Min} of Q_i(s)[a] */
} ilsx_dsac_stats;
int ilsx_dsac_create(ilsx_ctx* ctx, const ilsx_dsac_cfg* cfg, ilsx_net* pi, ilsx_net* qf1, ilsx_net* qf2, ilsx_dsac** out);
int ilsx_dsac_destroy(ilsx_dsac* d);
/* device batch rows: obs[B,o], act[B,1] (indices), rew[B], done[B], nobs[B,o]; an index outside [0, n) or not integral = ILSX_ERR_ARG
 * (the check reads the action column back to the host).  stats nullable (host). */
int ilsx_dsac_train_step(ilsx_dsac* d, const float* obs, const float* act, const float* rew, const float* done, const float* nobs, int B,
                         ilsx_dsac_stats* stats);
int ilsx_dsac_train_from_replay(ilsx_dsac* d, ilsx_replay* rb, int n_steps, int B, ilsx_dsac_stats* stats);
/* which: 0 qf1, 1 qf2, 2 policy, 3 target_qf1, 4 target_qf2; HOST flat arrays */
int ilsx_dsac_get_params(ilsx_dsac* d, int which, float* dst_host, size_t n);
int ilsx_dsac_set_params(ilsx_dsac* d, int which, const float* src_host, size_t n);

/* ---------------------------------------------------------------- DQN / Double DQN
 * Replaces rlkit/torch/algorithms/dqn/dqn.py:17-65 (ctor), :67-105 (_do_training), :107-112 (_update_target_network) and
 * double_dqn.py:12-51.  qf: one FlattenMlp obs -> n action values, with or without the epsilon-greedy mark (the env acts with this very
 * network).  Batches carry the action INDEX as a float in a 1-wide action column (the reference's one-hot row, as its index).
 * v = max_j TQ(s')_j, or with double_q TQ(s')_{j*}, j* the first maximal Q(s')_j; y = r + (1 - d) * discount * v (no reward scale);
 * loss nn.MSELoss()(Q(s)_a, y); Adam(lr = learning_rate), torch's default betas.  Targets: Polyak with tau after the Adam step, or with
 * use_hard_updates a hard copy on the steps whose counter (tested before its increment, one per train step) is a multiple of
 * hard_update_period — the first step copies.  Statistics are those of the first batch of a call (dqn.py:97). */
typedef struct {
  float discount, learning_rate, tau;
  int32_t use_hard_updates, hard_update_period, double_q, max_batch;
} ilsx_dqn_cfg;
typedef struct {
  float qf_loss;     /* mean((Q(s)_a - y)^2) */
  float y_pred[4];   /* {Mean, Std, Max, Min} of Q(s)_a */
} ilsx_dqn_stats;
int ilsx_dqn_create(ilsx_ctx* ctx, const ilsx_dqn_cfg* cfg, ilsx_net* qf, ilsx_dqn** out);
int ilsx_dqn_destroy(ilsx_dqn* dqn);
/* device batch rows: obs[B,o], act[B,1] (indices), rew[B], done[B], nobs[B,o]; an index outside [0, n) or not integral = ILSX_ERR_ARG
 * (the check reads the action column back to the host).  stats nullable (host). */
int ilsx_dqn_train_step(ilsx_dqn* dqn, const float* obs, const float* act, const float* rew, const float* done, const float* nobs, int B,
                        ilsx_dqn_stats* stats);
int ilsx_dqn_train_from_replay(ilsx_dqn* dqn, ilsx_replay* rb, int n_steps, int B, ilsx_dqn_stats* stats);
/* which: 0 qf, 1 target_qf; HOST flat arrays */
int ilsx_dqn_get_params(ilsx_dqn* dqn, int which, float* dst_host, size_t n);
int ilsx_dqn_set_params(ilsx_dqn* dqn, int which, const float* src_host, size_t n);

/* ---------------------------------------------------------------- SAC with a state-value function
 * Replaces rlkit/torch/algorithms/sac/sac.py:23-68 (ctor), :70-179 (train_step), :242-243 (soft update of V).
 * cfg fields == the YAML `sac_params` keys (exp_specs/sac/sac_hopper.yaml:36-47 with run_scripts/sac_exp_script.py). */
typedef struct {
  float reward_scale, discount, alpha, policy_lr, qf_lr, vf_lr, soft_target_tau;
  float policy_mean_reg_weight, policy_std_reg_weight, beta_1;
  int32_t max_batch;
} ilsx_sacv_cfg;
typedef struct {
  float qf1_loss, qf2_loss, vf_loss, policy_loss;
  float q1_pred[4], q2_pred[4], v_pred[4], log_pi[4], policy_mu[4], policy_log_std[4];
} ilsx_sacv_stats;
int ilsx_sacv_create(ilsx_ctx* ctx, const ilsx_sacv_cfg* cfg, ilsx_net* pi, ilsx_net* qf1, ilsx_net* qf2, ilsx_net* vf,
                     ilsx_sacv** out);
int ilsx_sacv_destroy(ilsx_sacv* sac);
/* eps: device [B,a] N(0,1) draws of the single policy sample of the step (sac.py:123) or NULL = Philox */
int ilsx_sacv_train_step(ilsx_sacv* sac, const float* obs, const float* act, const float* rew, const float* done,
                         const float* nobs, int B, const float* eps, ilsx_sacv_stats* stats);
int ilsx_sacv_train_from_replay(ilsx_sacv* sac, ilsx_replay* rb, int n_steps, int B, ilsx_sacv_stats* stats);
/* which: 0 qf1, 1 qf2, 2 vf, 3 policy, 6 target_vf; HOST flat arrays */
int ilsx_sacv_get_params(ilsx_sacv* sac, int which, float* dst_host, size_t n);
int ilsx_sacv_set_params(ilsx_sacv* sac, int which, const float* src_host, size_t n);

/* ---------------------------------------------------------------- optimiser state (snapshots / resume)
 * The optimizer.state_dict() halves of the reference's get_snapshot / load_snapshot pairs (td3.py:185-210, sac.py:245-270,
 * ppo.py:47-55 policy/value optimisers, adv_irl.py:75-77 disc_optimizer, bc.py:33-41) and what `load_params` resumes from
 * (run_scripts/sac_alpha_exp_script.py:106-108,142-146; rlkit/core/logger.py:31-49).  Adam's exp_avg / exp_avg_sq travel in
 * the flat ABI layout of the parameter block they belong to (HOST fp32 [n], n = that block's parameter count); meta.t is the
 * owning optimiser's step count, meta.rng_step the agent's Philox step counter, meta.n_train_steps the trainer's own step
 * counter where it has one (TD3's delayed-update parity, td3.py:101).  `which` numbers the TRAINABLE blocks exactly like the
 * agent's *_get_params.  SAC-alpha has its own pair (ilsx_sac_get_adam / _set_adam / _alpha_opt above). */
typedef struct { int64_t t; uint64_t rng_step; int64_t n_train_steps; } ilsx_opt_meta;
int ilsx_td3_get_opt(ilsx_td3* td3, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);    /* 0 qf1, 1 qf2, 2 policy */
int ilsx_td3_set_opt(ilsx_td3* td3, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_ddpg_get_opt(ilsx_ddpg* ddpg, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);    /* 0 qf, 1 policy; n_train_steps = the hard-update counter */
int ilsx_ddpg_set_opt(ilsx_ddpg* ddpg, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_dsac_get_opt(ilsx_dsac* d, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);     /* 0 qf1, 1 qf2, 2 policy */
int ilsx_dsac_set_opt(ilsx_dsac* d, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_dqn_get_opt(ilsx_dqn* dqn, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);      /* 0 qf; n_train_steps = the hard-update counter */
int ilsx_dqn_set_opt(ilsx_dqn* dqn, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_sacv_get_opt(ilsx_sacv* sac, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);  /* 0 qf1, 1 qf2, 2 vf, 3 policy */
int ilsx_sacv_set_opt(ilsx_sacv* sac, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_bc_get_opt(ilsx_bc* bc, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);
int ilsx_bc_set_opt(ilsx_bc* bc, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_ppo_get_opt(ilsx_ppo* ppo, int which, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);    /* 0 policy (| action_log_std), 1 value net */
int ilsx_ppo_set_opt(ilsx_ppo* ppo, int which, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
int ilsx_disc_get_opt(ilsx_disc* disc, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);
int ilsx_disc_set_opt(ilsx_disc* disc, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);

/* ---------------------------------------------------------------- behaviour cloning
 * Replaces rlkit/torch/algorithms/bc/bc.py:14-41 (ctor: Adam(lr, betas=(momentum, 0.999)) over the policy) and :77-106
 * (_do_training / _do_update_step).  MLE: loss = -mean(policy.get_log_prob(obs, acts)); MSE: loss = mean over rows of
 * sum_j (policy(obs)[0] - acts)^2 with policy(obs)[0] a SAMPLED action, like the reference. */
enum { ILSX_BC_MLE = 0, ILSX_BC_MSE = 1 };
typedef struct { int32_t mode; float lr, momentum; int32_t max_batch; } ilsx_bc_cfg;
int ilsx_bc_create(ilsx_ctx* ctx, const ilsx_bc_cfg* cfg, ilsx_net* pi, ilsx_bc** out);   /* adopts pi like ilsx_sac_create */
int ilsx_bc_destroy(ilsx_bc* bc);
/* device rows obs[B,o], act[B,a]; eps (device [B,a], MSE mode's N(0,1) draws) or NULL = Philox; stat (host, nullable) =
 * "Log-Likelihood" (MLE) or "MSE" of this batch (bc.py:92-102) */
int ilsx_bc_train_step(ilsx_bc* bc, const float* obs, const float* act, int B, const float* eps, float* stat);
int ilsx_bc_train_from_replay(ilsx_bc* bc, ilsx_replay* expert_rb, int n_updates, int B, float* stat);

/* ---------------------------------------------------------------- PPO
 * Replaces rlkit/torch/algorithms/ppo/ppo.py:57-100 (calc_adv: per-trajectory GAE, zero bootstrap, per-trajectory
 * advantage standardisation) and :102-170 (train_step: update_epoch x shuffled minibatches of value MSE + L2 and
 * the clipped surrogate, grad-norm clip 20), with ReparamMultivariateGaussianPolicy (both conditioned_std settings)
 * (rlkit/torch/common/policies.py:348-478) and the tanh value net of run_scripts/ppo_exp_script.py:82-96.
 * cfg fields == the YAML keys of exp_specs/ppo/ppo_hopper.yaml:41-50 (+ net_size / num_hidden_layers :13-14). */
typedef struct {
  int32_t obs_dim, act_dim, n_hidden, hidden;
  float reward_scale, discount, clip_eps, policy_lr, value_lr, gae_tau, value_l2_reg;
  int32_t mini_batch_size, update_epoch;
  int32_t max_samples;            /* upper bound on the on-policy samples of one train call */
  int32_t use_value_clip;         /* ppo.py:24,137-143: value loss = mean(max((v-R)^2, (v_old + clamp(v-v_old, +-clip_eps) - R)^2)) */
  int32_t conditioned_std;        /* policies.py:354,368-374,401-405: log_std = clamp(last_fc_log_std(h), -20, 2), a second head of the policy net
                                   * (flat: fc.. | last_fc | last_fc_log_std) instead of the action_log_std parameter behind the mean net */
  int32_t hidden_sizes[3];        /* networks.py:23-60 takes any list of widths: logical width of hidden layer l (1..hidden; 0 = hidden), for the
                                   * policy and the value net alike (ppo_exp_script.py:79-96 builds both from one list) — ilsx_mlp_cfg::hidden_sizes */
  int32_t grad_world;             /* split-run mode (SURVEY section 8e "PPO split: same, per-minibatch grads"; 0 / 1 = off): this rank holds N / G of the
                                   * on-policy samples (its own envs' trajectories: GAE and the per-trajectory advantage standardisation stay local)
                                   * and mini_batch_size / G rows of every minibatch; mean-loss gradients are scaled 1 / (rows * G); the value arena
                                   * is all-reduced (sum) before its Adam (+ L2, applied once), the policy arena (with the action_log_std gradient)
                                   * before clip_grad_norm_ + Adam, on the communicator of the ctx (ilsx_comm_init).  Every rank must hold the
                                   * same number of samples and use the same minibatch size */
} ilsx_ppo_cfg;
int ilsx_ppo_create(ilsx_ctx* ctx, const ilsx_ppo_cfg* cfg, ilsx_ppo** out);
int ilsx_ppo_destroy(ilsx_ppo* ppo);
/* which: 0 = policy, flat = fc*.W|fc*.b|last_fc.W|last_fc.b|action_log_std[a] ; 1 = value net.  HOST arrays. */
int ilsx_ppo_num_params(const ilsx_ppo* ppo, int which, size_t* out);
int ilsx_ppo_set_params(ilsx_ppo* ppo, int which, const float* src_host, size_t n);
int ilsx_ppo_get_params(ilsx_ppo* ppo, int which, float* dst_host, size_t n);
/* calc_adv + the fixed log-probs over N = traj_offsets_host[n_traj] device rows obs[N,o] act[N,a] rew[N]; trajectory
 * t owns rows [traj_offsets_host[t], traj_offsets_host[t+1]).  bootstrap_values (device [n_traj], nullable): V of the
 * observation that follows each trajectory's last sample; NULL = 0 everywhere = the reference, which also zeroes it at
 * time-limit ends (ppo.py:74).  Device outputs [N], all nullable. */
int ilsx_ppo_gae(ilsx_ppo* ppo, const float* obs, const float* act, const float* rew, const int32_t* traj_offsets_host,
                 int n_traj, const float* bootstrap_values, float* returns, float* advantages, float* values,
                 float* fixed_log_probs);
/* values[n] = vf(obs[n,o]) (device) */
int ilsx_ppo_values(ilsx_ppo* ppo, const float* obs, int n, float* values);
/* one PPO.train_step.  perms_host [update_epoch][N] int32 row permutations (torch.randperm in the reference,
 * ppo.py:116) or NULL = drawn by the library. */
int ilsx_ppo_train(ilsx_ppo* ppo, const float* obs, const float* act, const float* rew, const int32_t* traj_offsets_host,
                   int n_traj, const float* bootstrap_values, const int32_t* perms_host);
/* debug: one library-drawn shuffle of [0,n) (keyed Feistel bijection; the NULL-perms path of ilsx_ppo_train) -> HOST */
int ilsx_ppo_debug_perm(ilsx_ppo* ppo, int n, uint32_t key, int32_t* perm_host);
/* test hook: the norm of the last minibatch's policy gradient as clip_grad_norm_ saw it (ppo.py:166; split run: of the all-reduced gradient) */
int ilsx_ppo_debug_grad_norm(ilsx_ppo* ppo, float* out);
/* get_actions (policies.py:392-417): act[n,a] = mean + exp(log_std)*eps (eps device [n,a] or NULL = Philox), or the
 * mean when deterministic; logp[n] nullable. */
int ilsx_ppo_policy_act(ilsx_ppo* ppo, const float* obs, int n, int deterministic, const float* eps, float* act,
                        float* logp);

/* ---------------------------------------------------------------- vectorised env stepper
 * Replaces the reference's vec-env path: rlkit/envs/vecenvs.py:158-257 (BaseVectorEnv.reset/step),
 * rlkit/envs/worker/subproc.py:59-113 (process + pipe per env), rlkit/envs/wrappers.py:342-352
 * (NormalizedBoxEnv action map + clip) and the MuJoCo step under gym's HopperEnv / Walker2dEnv, whose
 * reward / termination / reset rules are restated in rlkit/envs/mujoco/hopper.py:11-40, walker2d.py:11-36
 * (HalfCheetah: gym's HalfCheetahEnv — forward velocity - 0.1*|a|^2, no termination; rlkit/envs/envs_dict.py:7).
 * The dynamics model is a planar articulated-body engine (body 0: slide-x, slide-z, hinge; every other body
 * one hinge; capsule-vs-floor soft contacts + soft joint limits solved by PGS; RK4).  Model constants come
 * from the caller (ilswiss_amd/envs/models.py); physics parity with MuJoCo is UNPINNED. */
#define ILSX_ENV_MAX_BODY 8
#define ILSX_ENV_MAX_GEOM 8
enum { ILSX_TASK_HOPPER = 0, ILSX_TASK_WALKER2D = 1, ILSX_TASK_HALFCHEETAH = 2 /* never terminates */ };
typedef struct {
  int32_t task, n_body, n_geom, frame_skip, pgs_iters, pad0;
  int32_t parent[ILSX_ENV_MAX_BODY], limited[ILSX_ENV_MAX_BODY], geom_body[ILSX_ENV_MAX_GEOM];
  double anchor[ILSX_ENV_MAX_BODY][2];   /* hinge position in the parent's frame */
  double com[ILSX_ENV_MAX_BODY][2];      /* centre of mass in the body frame */
  double mass[ILSX_ENV_MAX_BODY], inertia[ILSX_ENV_MAX_BODY], jsign[ILSX_ENV_MAX_BODY];
  double armature[ILSX_ENV_MAX_BODY], damping[ILSX_ENV_MAX_BODY], range[ILSX_ENV_MAX_BODY][2], gear[ILSX_ENV_MAX_BODY];
  double geom_p1[ILSX_ENV_MAX_GEOM][2], geom_p2[ILSX_ENV_MAX_GEOM][2], geom_radius[ILSX_ENV_MAX_GEOM],
      geom_friction[ILSX_ENV_MAX_GEOM];  /* capsule end points (body frame), radius, sliding friction */
  double timestep, gravity, reset_noise, contact_margin;
  double contact_solref[2], contact_solimp[3], limit_solref[2], limit_solimp[3];
  double ctrl_cost, alive_bonus, z_min, z_max, ang_max, state_max;
  double init_qpos[ILSX_ENV_MAX_BODY + 2];
  double stiffness[ILSX_ENV_MAX_BODY];   /* joint spring towards 0 (half_cheetah.xml) */
  double reset_noise_vel_std;            /* > 0: reset qvel ~ N(0, std) instead of U(+-reset_noise) (HalfCheetahEnv.reset_model) */
  double qvel_clip;                      /* > 0: observations clip qvel to +-qvel_clip (Hopper / Walker2d: 10); <= 0: none */
  int32_t max_rows, pad1;                /* constraint rows per env the solver keeps (0 = 8 for 4 bodies, 12 otherwise; <= 16) */
} ilsx_planar_model;

int ilsx_vecenv_create(ilsx_ctx* ctx, const ilsx_planar_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* 3-D models — Ant-v2 and Humanoid-v2 (rlkit/envs/envs_dict.py:6,9; reward / termination / observation / reset rules of
 * rlkit/envs/mujoco/ant.py:11-43 and humanoid.py:24-73, Humanoid with the full 376-dim observation of gym's -v2: qpos[2:] | qvel |
 * cinert | cvel | qfrc_actuator | cfrc_ext).  Link 0 is the root body on a free joint (qpos = position + unit quaternion w x y z,
 * qvel = world linear + BODY-frame angular velocity); every other link hangs off its parent by one hinge (a MuJoCo body with k
 * hinges is a chain of k links, the first k-1 massless).  Constants come from the caller (ilswiss_amd/envs/models3d.py); the
 * engine is stated in oracle/spatial_env.py; physics parity with MuJoCo is UNPINNED.  The handle is an ordinary
 * ilsx_vecenv: reset / step / rollout / evaluation entry points are the ones below.  obs_trunc selects MBPO's truncated tasks
 * (ant_trunc_obs / humanoid_trunc_obs): the same task observed as qpos[2:] | qvel only. */
#define ILSX_ENV3_MAX_LINK 20
#define ILSX_ENV3_MAX_CONTACT 32
#define ILSX_ENV3_MAX_BODY 16
enum { ILSX_TASK_ANT = 3, ILSX_TASK_HUMANOID = 4 };
typedef struct {
  int32_t task, n_link, n_act, n_contact, n_body, frame_skip, pgs_iters, max_rows;
  int32_t parent[ILSX_ENV3_MAX_LINK], limited[ILSX_ENV3_MAX_LINK], act_link[ILSX_ENV3_MAX_LINK];   /* act_link[k]: link whose hinge actuator k drives */
  int32_t contact_link[ILSX_ENV3_MAX_CONTACT], body_link[ILSX_ENV3_MAX_BODY];   /* body_link[b]: link carrying MuJoCo body b+1 (observation rows) */
  double anchor[ILSX_ENV3_MAX_LINK][3];   /* hinge anchor in the parent link's frame */
  double axis[ILSX_ENV3_MAX_LINK][3];     /* unit hinge axis, link frame */
  double quat0[ILSX_ENV3_MAX_LINK][4];    /* fixed rotation parent -> link at q = 0 (w x y z) */
  double com[ILSX_ENV3_MAX_LINK][3], mass[ILSX_ENV3_MAX_LINK], inertia[ILSX_ENV3_MAX_LINK][6];   /* about the COM, link frame: xx yy zz xy xz yz */
  double armature[ILSX_ENV3_MAX_LINK], damping[ILSX_ENV3_MAX_LINK], stiffness[ILSX_ENV3_MAX_LINK], range[ILSX_ENV3_MAX_LINK][2],
      gear[ILSX_ENV3_MAX_LINK];
  double contact_pos[ILSX_ENV3_MAX_CONTACT][3], contact_radius[ILSX_ENV3_MAX_CONTACT], contact_friction[ILSX_ENV3_MAX_CONTACT];
  double timestep, gravity, reset_noise, reset_noise_vel_std, contact_margin, ctrl_range;
  double contact_solref[2], contact_solimp[3], limit_solref[2], limit_solimp[3];
  double ctrl_cost, alive_bonus, vel_weight, z_min, z_max;
  double init_qpos[ILSX_ENV3_MAX_LINK + 6];
  int32_t obs_trunc, pad0;   /* != 0: the observation is qpos[2:] | qvel only (MBPO's ant_trunc_obs / humanoid_trunc_obs: 27 / 45
                              * columns); reward, termination, reset and the state layout are those of the full task; refused for trees with
                              * other dof counts than the Ant's 14 and the Humanoid's 23.  0: as above */
} ilsx_spatial_model;
int ilsx_vecenv_create_spatial(ilsx_ctx* ctx, const ilsx_spatial_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* Classic control — gym 0.22's CartPoleEnv (gym/envs/classic_control/cartpole.py; rlkit/envs/envs_dict.py:2): closed-form Euler
 * dynamics, float64 in gym's order and constants, one lane per env.  State rows: qpos = (x, theta), qvel = (x_dot, theta_dot) (nq = nv = 2);
 * observation = float32 (x, x_dot, theta, theta_dot); reward 1 on every step, the terminal one included; done = |x| > 2.4 or |theta| > 12 deg;
 * reset: every component U[-0.05, 0.05) from the env's Philox stream.  Actions are a Discrete(2) index held as a float in a 1-wide action
 * column (act_dim 1; env_replay_buffer.py:40); random actions are uniform indices.
 * ILSX_CLASSIC_PENDULUM — gym 0.22's PendulumEnv behind the reference's NormalizedBoxEnv (rlkit/envs/wrappers.py:342-346): Box(-1, 1)
 * actions of width 1 (discrete_n 0), torque = clip(-2 + (a + 1) * 0.5 * 4, +-2) in float32; float64 state qpos = (theta), qvel =
 * (theta_dot) (nq = nv = 1, theta never wrapped); observation = float32 (cos theta, sin theta, theta_dot); reward = -(angle_normalize(theta)^2
 * + 0.1 theta_dot^2 + 0.001 u^2) of the state before the step; theta_dot' = clip(theta_dot + (15 sin theta + 3 u) * 0.05, +-8), theta' =
 * theta + theta_dot' * 0.05; never done (max_path_length ends episodes); reset: theta ~ U[-pi, pi), theta_dot ~ U[-1, 1).  The replay
 * record holds the action as the policy gave it, before the map.
 * ILSX_CLASSIC_INVERTED_PENDULUM / ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM — gym 0.22's InvertedPendulumEnv / InvertedDoublePendulumEnv
 * (envs_dict `invertedpendulum` / `inverteddoublependulum`) behind NormalizedBoxEnv, on this library's own rigid-body dynamics of a cart
 * on a rail carrying 1 or 2 poles (ilsx_cartchain_model below; no MuJoCo): float64 state qpos = (x, theta_1[, theta_2]), qvel likewise
 * (nq = nv = 2 or 3), RK4 with a soft joint-limit solve in every stage, frame_skip substeps; Box(-1, 1) actions of width 1, ctrl =
 * clip(lb + (a + 1) * 0.5 * (ub - lb), lb, ub) in float32.  InvertedPendulum: observation float32 (qpos | qvel), reward 1, done = a
 * non-finite state or |theta| > 0.2, reset = U(+-0.01) on qpos and qvel.  InvertedDoublePendulum: observation float32 (x, sin theta_1,
 * sin theta_2, cos theta_1, cos theta_2, clip(qvel, +-10), clip(qfrc_constraint, +-10)) (11 wide, the layout
 * ILSX_TERM_INVERTED_DOUBLE_PENDULUM reads), qfrc_constraint = J^T f of the last RK4 stage of the last substep (0 after a reset),
 * reward = 10 - (0.01 x_tip^2 + (y_tip - 2)^2) - (1e-3 qvel_1^2 + 5e-3 qvel_2^2) of the state after the step, done = y_tip <= 1, reset
 * qpos = U(+-0.1), qvel = 0.1 N(0, 1).  ilsx_vecenv_create_classic builds them from the built-in constants (the values of
 * ilswiss_amd/envs/models_cartchain.py); ilsx_vecenv_create_cartchain takes the constants from the caller.
 * ILSX_CLASSIC_MOUNTAINCAR_CONT — gym 0.22's Continuous_MountainCarEnv (envs_dict `mountaincarcont`) behind NormalizedBoxEnv: Box(-1, 1)
 * actions of width 1 (discrete_n 0), force = clip(-1 + (a + 1) * 0.5 * 2, +-1) in float32; state qpos = (x), qvel = (v) (nq = nv = 1),
 * doubles holding float32 values (the env keeps a float32 array between steps), the arithmetic of a step float64: v' = clip(v + force *
 * 0.0015 - 0.0025 cos(3 x), +-0.07), x' = clip(x + v', -1.2, 0.6), v' = 0 where x' = -1.2 and v' < 0; done = x' >= 0.45 and v' >= 0;
 * reward = (done ? 100 : 0) - 0.1 force^2; observation = the two floats; reset: x = float32(-0.6 + 0.2 u), v = 0.
 * ILSX_CLASSIC_MOUNTAINCAR — gym 0.22's MountainCarEnv: Discrete(3) (the index as a float in a 1-wide action column, used as it is: 0 left,
 * 1 none, 2 right); float64 state qpos = (x), qvel = (v); v' = clip(v + (a - 1) * 0.001 + cos(3 x) * (-0.0025), +-0.07), x' and the wall
 * as above; done = x' >= 0.5 and v' >= 0; reward -1 on every step; observation = float32 (x, v); reset: x = -0.6 + 0.2 u, v = 0.
 * ILSX_CLASSIC_ACROBOT — gym 0.22's AcrobotEnv ("book" dynamics, no torque noise): Discrete(3), torque = a - 1; float64 state qpos =
 * (theta_1, theta_2), qvel = (dtheta_1, dtheta_2) (nq = nv = 2); one classic RK4 step of 0.2 s, then wrap() of both angles into [-pi, pi]
 * (its loops end after 16 turns; an angle still outside ends the episode as a non-finite state does) and bound() of the velocities to
 * +-4 pi / +-9 pi; done = -cos theta_1 - cos(theta_2 + theta_1) > 1; reward = done ? 0 : -1; observation = float32 (cos theta_1,
 * sin theta_1, cos theta_2, sin theta_2, dtheta_1, dtheta_2) (6 wide); reset: four draws U(-0.1, 0.1) rounded to float32.
 * None of the three carries a TimeLimit (the reference builds the classes directly): max_path_length ends episodes.
 * Reset / step / rollout / evaluation entry points are the ordinary ones; ilsx_vecenv_set_obs_affine is not available. */
enum { ILSX_CLASSIC_CARTPOLE = 0, ILSX_CLASSIC_PENDULUM = 1, ILSX_CLASSIC_INVERTED_PENDULUM = 2, ILSX_CLASSIC_INVERTED_DOUBLE_PENDULUM = 3 };
enum { ILSX_CLASSIC_MOUNTAINCAR_CONT = 4, ILSX_CLASSIC_MOUNTAINCAR = 5, ILSX_CLASSIC_ACROBOT = 6 };   /* gym's closed-form tasks, no model */
int ilsx_vecenv_create_classic(ilsx_ctx* ctx, int kind, int n_env, uint64_t seed, ilsx_vecenv** out);
/* A cart on a rail (DoF 0, slide along x) carrying n_pole poles in a chain (DoF k = hinge of pole k, angle relative to its parent).
 * Body 0 is the cart, body k pole k; a pole's absolute angle is jsign * (q_1 + ... + q_k), counter-clockwise in (x, z).  anchor[k] =
 * hinge k in the parent's frame, com[k] = centre of mass in the body's frame, tip = the reward's site in the last pole's frame.  The
 * actuator (gear, ctrl_range) drives the slide only.  Limits are soft unilateral rows (limit_solref = (timeconst, dampratio),
 * limit_solimp = (d0, dmax, width)); DoF 0 and DoF 1 may be limited. */
#define ILSX_CARTCHAIN_MAX_DOF 3
typedef struct {
  int n_pole, frame_skip, pgs_iters;      /* n_pole 1 (InvertedPendulum rules) or 2 (InvertedDoublePendulum rules) */
  int limited[ILSX_CARTCHAIN_MAX_DOF];
  double mass[ILSX_CARTCHAIN_MAX_DOF], inertia[ILSX_CARTCHAIN_MAX_DOF];   /* inertia about the COM, axis normal to the plane */
  double com[ILSX_CARTCHAIN_MAX_DOF][2], anchor[ILSX_CARTCHAIN_MAX_DOF][2];
  double armature[ILSX_CARTCHAIN_MAX_DOF], damping[ILSX_CARTCHAIN_MAX_DOF], range[ILSX_CARTCHAIN_MAX_DOF][2];
  double tip[2], gear, ctrl_range[2], jsign;
  double timestep, gravity, limit_solref[2], limit_solimp[3];
} ilsx_cartchain_model;
int ilsx_vecenv_create_cartchain(ilsx_ctx* ctx, const ilsx_cartchain_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* Swimmer — gym 0.22's SwimmerEnv rules (envs_dict `swimmer`) behind NormalizedBoxEnv, on this library's own dynamics of a free planar
 * chain of n_link links in a viscous medium (csrc/swimmer_env.h; no MuJoCo).  DoF (x, y, theta_0, q_1, ...): the
 * first link carries two slides and a hinge at its origin, link k >= 1 hinges on link k - 1 at anchor[k] (the parent's frame); a link's
 * absolute angle is theta_0 + q_1 + ... + q_k, counter-clockwise.  float64 state, nq = nv = n_link + 2; RK4 with a soft joint-limit solve
 * in every stage, frame_skip substeps; no gravity in the plane, no contacts.  Each link feels the drag of its inertia box: box[k] holds
 * the box's full sides (along the link, across it in the plane, normal to the plane), which the caller derives from mass and
 * inertia[k] = (I_x, I_y, I_z) about the COM; force and torque are in the header of swimmer_env.h.  The arrays indexed by DoF
 * (limited, armature, damping, range, gear, init_qpos) have n_link + 2 entries; only the hinges q_k may be limited, and gear drives them
 * (ctrl = clip(lb + (a + 1) * 0.5 * (ub - lb), lb, ub) in float32 per actuator).  Box(-1, 1) actions of width n_link - 1; observation
 * float32 (qpos[2:] | qvel); reward = (x' - x) / (frame_skip * timestep) - 1e-4 * sum ctrl^2; never done; reset = init_qpos + U(+-0.1)
 * on qpos, U(+-0.1) on qvel.  The kernels are instantiated for n_link = 3.  The handle is an ordinary ilsx_vecenv of the classic-control
 * kind (ilsx_vecenv_set_obs_affine is not available); ilsx_vecenv_create_classic does not build it: the caller is the one source of the
 * constants (ilswiss_amd/envs/models_swimmer.py). */
#define ILSX_SWIMMER_MAX_LINK 4
#define ILSX_SWIMMER_MAX_DOF (ILSX_SWIMMER_MAX_LINK + 2)
enum { ILSX_SWIMMER_TASK = 16 };   /* the task id of the handle, outside ILSX_CLASSIC_* */
typedef struct {
  int n_link, frame_skip, pgs_iters;
  int limited[ILSX_SWIMMER_MAX_DOF];
  double mass[ILSX_SWIMMER_MAX_LINK], inertia[ILSX_SWIMMER_MAX_LINK][3], box[ILSX_SWIMMER_MAX_LINK][3];
  double com[ILSX_SWIMMER_MAX_LINK][2], anchor[ILSX_SWIMMER_MAX_LINK][2];
  double armature[ILSX_SWIMMER_MAX_DOF], damping[ILSX_SWIMMER_MAX_DOF], range[ILSX_SWIMMER_MAX_DOF][2], gear[ILSX_SWIMMER_MAX_DOF];
  double init_qpos[ILSX_SWIMMER_MAX_DOF];
  double ctrl_range[2], timestep, density, viscosity, limit_solref[2], limit_solimp[3];
} ilsx_swimmer_model;
int ilsx_vecenv_create_swimmer(ilsx_ctx* ctx, const ilsx_swimmer_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* LunarLanderContinuous — gym 0.22's LunarLander rules, continuous branch (envs_dict `lunarlandercont`; NormalizedBoxEnv over Box(-1, 1)
 * is the identity), on this library's own dynamics (csrc/lunar_env.h; no Box2D): ONE rigid body of three degrees
 * of freedom (hull and legs as one, the legs at their rest angle), soft contacts at the two foot points, semi-implicit Euler with
 * frame_skip substeps per 1 / fps.  float64 state, nq = 14: qpos = (x, y, theta of the hull origin, smooth_y[0..10] of the episode's
 * terrain); nv = 4: qvel = (vx, vy, omega, sleep_time); ilsx_vecenv_dims reports 3 degrees of freedom.  Lengths in metres (pixels /
 * scale); com, foot (0 = left, 1 = right) and hull (the polygon's six vertices) are in the hull frame; mass and inertia (about com) are
 * the composite body's.  Box(-1, 1) actions of width 2 (main engine, side engines), clipped to +-1; the engines' dispersion is drawn on
 * every step.  Observation float32, 8 wide, gym's `state`, the two contact flags set when a foot is at or below the terrain; reward =
 * shaping(after) - shaping(before) - 0.30 m_power - 0.03 s_power; done with reward -100 when a hull vertex touches the terrain or
 * |obs[0]| >= 1, with +100 once the body has been below both sleep tolerances for sleep_time; no time limit of its own.  Contacts are soft
 * rows (contact_solref = (timeconst, dampratio), contact_solimp = (d0, dmax, width)) with Coulomb friction.  The handle is an ordinary
 * ilsx_vecenv of the classic-control kind (ilsx_vecenv_set_obs_affine is not available); ilsx_vecenv_create_classic does not build it:
 * the caller is the one source of the constants (ilswiss_amd/envs/models_lunar.py).  Refused: non-finite constants; non-positive mass,
 * inertia, fps, scale, w, h, frame_skip, pgs_iters, solref, impedances or sleep tolerances; a foot that is not below the hull's bottom. */
enum { ILSX_LUNAR_TASK = 17 };   /* the task id of the handle, outside ILSX_CLASSIC_* */
typedef struct {
  int frame_skip, pgs_iters;
  double fps, scale, w, h, gravity, main_engine_power, side_engine_power, initial_random;
  double side_engine_height, side_engine_away, leg_down, helipad_y;
  double mass, inertia, com[2], foot[2][2], hull[6][2];
  double friction, contact_solref[2], contact_solimp[3];
  double sleep_lin_tol, sleep_ang_tol, sleep_time;
} ilsx_lunar_model;
int ilsx_vecenv_create_lunar(ilsx_ctx* ctx, const ilsx_lunar_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* A goal env on the lane-per-env frame: ilswiss_amd/her.py's PointReachEnv as a device stepper (a STAND-IN for the reference's MuJoCo Fetch
 * tasks, not one of them).  float64 state qpos = (p_x, p_y, g_x, g_y) — the goal is episode state —, qvel = (v_x, v_y); Box(-1, 1)^2 actions.
 * An observation row is 8 float32 columns, observation (p | v) | desired_goal (g) | achieved_goal (p): the segment layout of ilsx_her_gather
 * and ilsx_her_sample, so a ring of width 8 filled by ilsx_rollout_step (path mode) is a hindsight ring.  A policy on this env reads the
 * first d_obs + d_goal = 6 columns of the row in place; one of any other input width is refused (ILSX_ERR_ARG).
 *   step   v = step_scale * clip(a, -1, 1) in float32 (as numpy evaluates it for a float32 action), widened; p = clip(p + v, -1, 1) in float64;
 *          reward_kind 0: -(|p - g| > tol), 1: -|p - g|, on float64; never done (max_path_length ends episodes)
 *   reset  p = U(+-p_range)^2, v = 0, g = U(+-g_range)^2 from counters 0..3 of the env's Philox stream
 * Constants must be finite and positive (ranges at most 1), else ILSX_ERR_ARG before anything is allocated.  Refused on a goal env with
 * ILSX_ERR_UNSUPPORTED: ilsx_vecenv_obs_norm(norm_obs=1), ilsx_vecenv_set_obs_affine, ilsx_rollout_steps_lockstep,
 * ilsx_eval_rollouts_lockstep, ilsx_ppo_rollout. */
enum { ILSX_GOAL_TASK = 18 };   /* the task id of the handle, outside ILSX_CLASSIC_* */
typedef struct {
  double tol, step_scale, p_range, g_range;
  int32_t reward_kind;   /* 0 sparse, 1 dense */
  int32_t pad;
} ilsx_goal_model;
int ilsx_vecenv_create_goal(ilsx_ctx* ctx, const ilsx_goal_model* model, int n_env, uint64_t seed, ilsx_vecenv** out);
/* widths of the observation and goal segments of a goal env's row (ILSX_ERR_STATE on any other env) */
int ilsx_vecenv_goal_dims(const ilsx_vecenv* env, int* d_obs, int* d_goal);
/* discrete_n = n of a Discrete(n) action space, 0 for Box actions */
int ilsx_vecenv_action_space(const ilsx_vecenv* env, int* discrete_n);
/* Path mode of the fused rollout (ilsx_rollout_step with a replay ring): 0 (default) = every transition enters the ring when it
 * happens; 1 = the reference's order (rlkit/core/base_algorithm.py:509-519, simple_replay_buffer.py:78-132): an episode's samples are
 * staged in HBM and enter the ring contiguously when the episode ends (ended envs in ascending order), the trajectory is registered in
 * _traj_endpoints, unfinished episodes are not sampleable.  Costs one 4-byte-per-env read-back per rollout step. */
int ilsx_vecenv_set_path_mode(ilsx_vecenv* env, int on);
/* sizes of the simulator state rows of ilsx_vecenv_get_state / _set_state (planar: nq == nv; 3-D: nq == nv + 1) */
int ilsx_vecenv_state_dims(const ilsx_vecenv* env, int* nq, int* nv);
int ilsx_vecenv_destroy(ilsx_vecenv* env);
int ilsx_vecenv_dims(const ilsx_vecenv* env, int* obs_dim, int* act_dim, int* n_dof, int* n_env);
/* BaseVectorEnv.reset(id) (vecenvs.py:158-181): ids_host = NULL resets all; obs (device, nullable) [n_ids,o]. */
int ilsx_vecenv_reset(ilsx_vecenv* env, const int32_t* ids_host, int n_ids, float* obs);
/* BaseVectorEnv.step(action, id) (vecenvs.py:183-257), sync mode: act[n_ids,a] -> obs[n_ids,o], rew[n_ids],
 * done[n_ids] (all device; outputs nullable).  No auto-reset (the caller resets finished ids, like the reference). */
int ilsx_vecenv_step(ilsx_vecenv* env, const float* act, const int32_t* ids_host, int n_ids, float* obs, float* rew,
                     uint8_t* done);
/* simulator state, HOST float64 qpos [n_env, nq], qvel [n_env, nv] (tests / snapshots) */
int ilsx_vecenv_get_state(ilsx_vecenv* env, double* qpos_host, double* qvel_host);
int ilsx_vecenv_set_state(ilsx_vecenv* env, const double* qpos_host, const double* qvel_host);
int ilsx_vecenv_cur_obs(ilsx_vecenv* env, float** dev_ptr);  /* [n_env,o] current (normalised if norm_obs) observations (device) */
/* ScaledEnv / MinmaxEnv (rlkit/envs/wrappers.py:53-203): every observation the env hands out or records becomes
 * (raw - shift) / scale; shift / scale are HOST float64 [obs_dim], scale already including the wrappers' EPS
 * (std + EPS, or max - min + EPS).  Resets all envs. */
int ilsx_vecenv_set_obs_affine(ilsx_vecenv* env, const double* shift_host, const double* scale_host);
/* Batched terminal predicates of rlkit/envs/terminals.py:14-117 (TerminalFunc.is_terminal(obs, act, next_obs), the functions
 * MBPO's FakeEnv and model rollouts label transitions with): done[n] = f(next_obs[n,o]) on the device, NaN / inf
 * semantics and the Hopper upper-bound-only state check (:61) as in the reference. */
enum { ILSX_TERM_INVERTED_PENDULUM = 0, ILSX_TERM_INVERTED_DOUBLE_PENDULUM = 1, ILSX_TERM_HOPPER = 2, ILSX_TERM_WALKER2D = 3,
       ILSX_TERM_HALFCHEETAH = 4, ILSX_TERM_HUMANOID = 5, ILSX_TERM_ANT = 6 };
int ilsx_is_terminal(ilsx_ctx* ctx, int kind, const float* next_obs, int n, int obs_dim, uint8_t* done);
/* Running observation statistics of BaseVectorEnv (vecenvs.py:104-113,299-327; RunningMeanStd normalizer.py:128-152):
 * norm_obs: reset/step/cur_obs/rollouts return clip((obs-mean)/sqrt(var+eps), +-10); update_obs_rms: every batch of
 * observations returned by reset/step updates (mean, var, count) first.  Statistics are float64; get/set use HOST arrays
 * [obs_dim] (an eval env shares the training env's statistics by set after get, ppo_exp_script.py:68-75). */
int ilsx_vecenv_obs_norm(ilsx_vecenv* env, int norm_obs, int update_obs_rms);
int ilsx_vecenv_get_obs_rms(ilsx_vecenv* env, double* mean_host, double* var_host, double* count);
int ilsx_vecenv_set_obs_rms(ilsx_vecenv* env, const double* mean_host, const double* var_host, double count);
/* PPO's sampling phase for ALL envs on the device (torch_rl_algorithm.py:30-32 over base_algorithm.py:183-277): T vec
 * steps with ppo's Gaussian policy, auto-reset on done / max_path_length, into env-major device buffers (sample (env,t) at
 * row env*T+t): obs[n_env*T,o] as the policy saw it, act[n_env*T,a], rew[n_env*T], ends[n_env*T] (1 = the episode ended
 * after this sample); last_values[n_env] (nullable) = vf(observation after the last step). */
int ilsx_ppo_rollout(ilsx_ppo* ppo, ilsx_vecenv* env, int T, int max_path_length, float* obs, float* act, float* rew,
                     uint8_t* ends, float* last_values);
/* One iteration of BaseAlgorithm's sampling loop for ALL envs on the device (base_algorithm.py:183-277):
 * actions (policy, or env.action_space.sample() when random_actions) -> physics -> one transition record per
 * env written straight into the replay ring (nullable) -> auto-reset on done or max_path_length.  no_terminal: the
 * stored terminal flag is forced to 0 (base_algorithm.py:195-196,208-210; the adv-IRL configs).
 * A normalising env (ilsx_vecenv_obs_norm, flat envs only) with a ring records what the policy saw, as the reference does
 * (vecenvs.py:251-257): the record's observation is bit for bit the policy input of the step, its next observation is the
 * step's observation normalised under the statistics updated with that batch, and for an env whose episode goes on that
 * value IS the next policy input (never re-normalised; old rows do not follow the statistics).  Envs whose episode ended
 * feed their reset observations to the statistics next and are normalised under the newest ones.  update_obs_rms = 0:
 * the same without the two updates.  The same holds for _begin / _end, _relabel (policy and expert both act on the
 * normalised input) and the lock-step form, with and without path mode.  Without a ring the policy input is re-normalised
 * as a whole after every step, as before. */
int ilsx_rollout_step(ilsx_vecenv* env, ilsx_net* pi, ilsx_replay* rb, int max_path_length, int random_actions,
                      int deterministic, int no_terminal);
/* Exploration strategies of deterministic policies on the device (rlkit/exploration_strategies/{gaussian,ou}_strategy.py behind
 * base.py:39-60 PolicyWrappedWithExplorationStrategy), ONE process per env, float64 in the reference's order:
 *   Gaussian: act = clip(act + sigma(t) * N(0,1), low, high), sigma(t) = max_sigma - (max_sigma - min_sigma) * min(1, t / decay_period);
 *   OU      : state += theta * (mu - state) + sigma_prev * N(0,1) with the sigma of the env's PREVIOUS call, then sigma = sigma(t);
 *             act = clip(act + state, low, high).  An env at the start of an episode (its step counter is 0) first puts its state back
 *             to mu (OUStrategy.reset through the wrapper's reset()).
 * ilsx_rollout_step applies the env's strategy to the policy's actions unless the step is deterministic or random_actions; evaluation
 * rollouts never explore; runs with a strategy set do not share launches in ilsx_rollout_steps_lockstep (they step one by one). */
typedef struct {
  int32_t kind;   /* 0 none, 1 Gaussian, 2 OU */
  int32_t pad;
  double mu, theta, max_sigma, min_sigma, decay_period, low, high;
} ilsx_explore_cfg;
int ilsx_vecenv_set_exploration(ilsx_vecenv* env, const ilsx_explore_cfg* cfg);   /* (re)starts every env's process at mu, sigma at max_sigma */
int ilsx_vecenv_set_exploration_t(ilsx_vecenv* env, int64_t t);                    /* the t of the rollout's next steps (set_num_steps_total) */
/* one exploration step on act[n_env, a] (device, in place); eps: device float64 [n_env, a] N(0,1) draws or NULL = Philox */
int ilsx_vecenv_explore(ilsx_vecenv* env, float* act, const double* eps, int64_t t);
/* The epsilon-uniform branch of the Gaussian strategy — MlpGaussianAndEpsilonPolicy.get_actions (policies.py:537-552): with probability
 * epsilon an env takes a uniform action act_j = (float)(low + (high - low) * u_{1+j}) instead of the noisy one (u_0 < epsilon decides, per
 * env; the reference draws once per call for its whole batch, which is the same thing at one env).  epsilon in [0, 1], Gaussian kind only
 * (ILSX_ERR_STATE otherwise); ilsx_vecenv_set_exploration puts it back to 0, and at 0 the strategy's output is bit for bit what it is
 * without this call.  _explore_u: ilsx_vecenv_explore with explicit draws u = device float64 [n_env, 1 + a] in [0, 1) (NULL = Philox). */
int ilsx_vecenv_set_exploration_epsilon(ilsx_vecenv* env, double epsilon);
int ilsx_vecenv_explore_u(ilsx_vecenv* env, float* act, const double* eps, const double* u, int64_t t);
/* Evaluation on the device — VecPathSampler.obtain_samples / rollout (samplers/vec_sampler.py:5-93,124-142): reset all envs,
 * then every env plays ONE episode with `pi` (ilsx_net: tanh-Gaussian or noise policy) or `ppo`'s Gaussian policy; envs that
 * end (terminal or max_path_length) are frozen, not reset.  stats_host[18] (nullable, float64) accumulates what
 * eval_util.get_generic_path_information (:15-80) needs: {paths, steps, returns sum/sumsq/max/min, lengths
 * sum/sumsq/max/min, rewards sum/sumsq/max/min, actions sum/sumsq/max/min}; reset_stats = 0 keeps accumulating over calls. */
#define ILSX_EVAL_NSTATS 18
int ilsx_eval_rollout(ilsx_vecenv* env, ilsx_net* pi, ilsx_ppo* ppo, int max_path_length, int deterministic, int reset_stats,
                      double* stats_host);
/* The same for K runs at once (one small eval env per run, the lock-step loop of co-resident seeds): every run rolls whole rounds until ITS
 * statistics hold >= num_steps steps (VecPathSampler.obtain_samples, vec_sampler.py:126-146); runs of one shape step as one launch per stage, and
 * a run leaves a round at the check at which its own ilsx_eval_rollout would, so its counters and statistics are those of evaluating it alone.
 * stats_host: [n_runs][18] doubles, ilsx_eval_rollout's layout.  ILSX_ERR_UNSUPPORTED: the runs cannot share launches (evaluate them one by one). */
int ilsx_eval_rollouts_lockstep(ilsx_vecenv* const* envs, ilsx_net* const* pis, int n_runs, int max_path_length, int deterministic,
                                int64_t num_steps, double* stats_host);
/* ilsx_rollout_step in two halves, for a host that advances several runs side by side, each on its own ctx / stream (the lock-step loop of
 * co-resident seeds): _begin only enqueues the step; _end does the part that needs the host — with path mode on it waits for the step and
 * inserts the episodes that ended in it, otherwise nothing.  begin(run 0..K-1) ; end(run 0..K-1) overlaps the K runs' launches on the GPU. */
int ilsx_rollout_step_begin(ilsx_vecenv* env, ilsx_net* pi, ilsx_replay* rb, int max_path_length, int random_actions,
                            int deterministic, int no_terminal);
int ilsx_rollout_step_end(ilsx_vecenv* env);
/* n_steps lock-step iterations of n_runs runs: per iteration begin(run 0..K-1) ; end(run 0..K-1).  Run k acts at random while its ring holds
 * fewer than min_steps_before_training[k] samples (base_algorithm.py:186-188).  One call per stretch between two train triggers. */
int ilsx_rollout_steps_lockstep(ilsx_vecenv* const* envs, ilsx_net* const* pis, ilsx_replay* const* rbs, int n_runs, int n_steps,
                                int max_path_length, const int64_t* min_steps_before_training, int deterministic, int no_terminal);
/* DAgger's sampling iteration (dagger/dagger.py:45-71): the envs are driven by `pi`, the action stored in the replay record is
 * `expert`'s action for the observation acted on. */
int ilsx_rollout_step_relabel(ilsx_vecenv* env, ilsx_net* pi, ilsx_net* expert, int expert_deterministic, ilsx_replay* rb,
                              int max_path_length, int no_terminal);
/* finished episodes and the sum of their returns since the last reset of the counters */
int ilsx_rollout_stats(ilsx_vecenv* env, double* episodes, double* return_sum, int reset);


/* ---------------------------------------------------------------- MBPO: probabilistic ensemble dynamics model (ilswiss_amd/csrc/bnn.h)
 * BNN (rlkit/torch/common/networks.py:149-279): E members of n_hidden SiLU layers of `hidden` units and a head [mean | raw] of
 * 2 * out_dim, raw soft-clamped to a log-variance in [-10, 0.5]; inputs normalised by FixedNormalizer (normalizer.py:81-114).
 * BNNTrainer (mbpo/bnn_trainer.py:71-87,141-154): Adam (0.9, 0.999, 1e-8) with per-layer L2 weight decay.  Rows come from a replay
 * ring's records: inputs [obs | act], targets [reward_scale * rew | next_obs - obs], built on the device.  Parameters cross the ABI in
 * the reference's named_parameters() order, per layer weight[E, in, out] then bias[E, 1, out] (HOST fp32); padding is invisible. */
typedef struct ilsx_bnn ilsx_bnn;
#define ILSX_BNN_MAX_HID 8
typedef struct {
  int32_t ensemble;     /* num_nets */
  int32_t in_dim;       /* obs_dim + act_dim */
  int32_t out_dim;      /* obs_dim + 1 (BNN output_size; the head is 2 * out_dim wide) */
  int32_t hidden;       /* net_size (<= 400; above 256 the wide kernel runs, two column slices per wave); in_dim and 2 * out_dim <= 256 */
  int32_t n_hidden;     /* num_hidden_layers, 1..ILSX_BNN_MAX_HID */
  int32_t max_batch;    /* largest ilsx_bnn_train_batch B */
  float lr, reward_scale, init_w;
  float weight_decay[ILSX_BNN_MAX_HID + 1];   /* per layer (hidden layers, then the head), on weights and biases */
} ilsx_bnn_cfg;
int ilsx_bnn_create(ilsx_ctx* ctx, const ilsx_bnn_cfg* cfg, ilsx_bnn** out);
int ilsx_bnn_destroy(ilsx_bnn* bnn);
int ilsx_bnn_num_params(const ilsx_bnn* bnn, size_t* n);
/* hidden weights U(+-1/sqrt(in*out)) (fanin_init on [E,in,out], pytorch_util.py:20-29), hidden biases 0.1, head weight / bias
 * U(+-init_w); host RNG seeded by `seed` */
int ilsx_bnn_init(ilsx_bnn* bnn, uint64_t seed);
int ilsx_bnn_get_params(const ilsx_bnn* bnn, float* dst_host, size_t n);
int ilsx_bnn_set_params(ilsx_bnn* bnn, const float* src_host, size_t n);
/* Adam exp_avg / exp_avg_sq in the parameter layout; meta.t = the shared step count, meta.rng_step = the model-step Philox counter */
int ilsx_bnn_get_opt(const ilsx_bnn* bnn, float* m_host, float* v_host, size_t n, ilsx_opt_meta* meta);
int ilsx_bnn_set_opt(ilsx_bnn* bnn, const float* m_host, const float* v_host, size_t n, const ilsx_opt_meta* meta);
/* FixedNormalizer mean / std (HOST fp32 [in_dim]; std as stored, its 1e-8 included) */
int ilsx_bnn_set_normalizer(ilsx_bnn* bnn, const float* mean_host, const float* std_host);
int ilsx_bnn_get_normalizer(const ilsx_bnn* bnn, float* mean_host, float* std_host);
/* bnn_trainer.py:113-118: mean and unbiased std of the inputs of ring rows idx[0..n) (device int32 ring slots); std < 1e-12 -> 1;
 * then + 1e-8 (normalizer.py:101-103).  Sets the normaliser. */
int ilsx_bnn_fit_stats(ilsx_bnn* bnn, ilsx_replay* rb, const int32_t* idx, int n);
/* One BNNTrainer batch (bnn_trainer.py:136-154): member e trains on ring rows idx[e * idx_member_stride + 0..B) (device int32);
 * loss_host (nullable, [E]): each member's mean((mu - t)^2 e^-lv) + mean(lv) before the step (synchronises). */
int ilsx_bnn_train_batch(ilsx_bnn* bnn, ilsx_replay* rb, const int32_t* idx, int64_t idx_member_stride, int B, float* loss_host);
/* BNNTrainer.compute_loss (bnn_trainer.py:71-87) per member over ring rows idx[e * idx_member_stride + 0..n): add_var = 0 is the
 * holdout / train MSE; out_host[E]; fixed reduction order (deterministic).  idx_member_stride = 0: the same rows for every member. */
int ilsx_bnn_mse(ilsx_bnn* bnn, ilsx_replay* rb, const int32_t* idx, int64_t idx_member_stride, int n, int add_var, float* out_host);
/* BNN.predict(x, factored=True) (networks.py:265-275): x[n, in_dim] (device) -> mean[E, n, out_dim], var (or log-var when
 * ret_log_var) [E, n, out_dim] (device). */
int ilsx_bnn_predict(ilsx_bnn* bnn, const float* x, int n, float* mean, float* var, int ret_log_var);
/* FakeEnv.step + one step of MBPO._rollout_model (fake_env.py:30-75, mbpo.py:244-270), on the device: actions from `pi`'s stochastic
 * get_actions (or the given act[n, a]), the ensemble forward, a member per row uniform over elites_host[n_elites] by Philox (or
 * model_idx[n]), next_obs = obs + mu[1:] + sqrt(var) z, rew = mu[0] + sqrt(var) z (z: eps[n, out_dim] or Philox; none when
 * deterministic), terminals by ilsx_is_terminal(term_kind), the n rows into model_rb (nullable) followed by terminate_episode, and
 * the next observations of the non-terminal rows compacted in order into obs_next.  act_out [n, a] / model_idx_out [n] nullable.
 * *n_survivors is the one value read back. */
/* (tests only) the largest |value| over the padded entries of the internal blocks (W, Wt, b of every layer and member, and Adam's
 * m / v): 0 while the padding is intact. */
int ilsx_bnn_debug_padding(const ilsx_bnn* bnn, double* max_abs);
int ilsx_mbpo_model_step(ilsx_bnn* bnn, ilsx_net* pi, ilsx_replay* model_rb, int term_kind, const float* obs, const float* act, int n,
                         const int32_t* elites_host, int n_elites, int deterministic, const float* eps, const int32_t* model_idx,
                         float* act_out, int32_t* model_idx_out, float* obs_next, int* n_survivors);

/* ---------------------------------------------------------------- GCSL (rlkit/torch/algorithms/gcsl/)
 * HindsightHorizonReplayBuffer.random_batch (relabel_horizon_replay_buffer.py:163-270, her_ratio 1) as one gather from the ring: for the
 * host-drawn device int64 idx / idx_relabel [B], X[B, d_obs + d_goal + T] = observation | next achieved goal of the relabel record |
 * horizon row (j >= idx_relabel - idx on raw ring indices: a wrapped trajectory gives an all-ones row, as in the reference).  mode 0:
 * act[B, act_dim] floats; mode 1: label[B] = (int32) action[0] (truncated like .long()).  Rows with an index outside the ring: zeros, label -1. */
int ilsx_her_horizon_gather(ilsx_replay* rb, const int64_t* idx, const int64_t* idx_relabel, int B, int d_obs, int d_goal, int T, int mode,
                            float* X, float* act, int32_t* label);
/* The BatchNorm categorical policy (CatagorialConditionPolicy(batch_norm=True): networks.py:118-145, policies.py:759-840): n_blocks (1..3)
 * Linear -> BatchNorm1d(eps 1e-5, momentum 0.1) -> ReLU blocks of width `hidden`, then last_fc to n_classes (<= 64) logits.  Flat
 * parameters in torch's parameters() order (per block W | b | gamma | beta, then last_fc W | b); running statistics [n_blocks][hidden]. */
typedef struct ilsx_bncat ilsx_bncat;
enum { ILSX_BNCAT_PARAMS = 0, ILSX_BNCAT_RUNNING_MEAN = 1, ILSX_BNCAT_RUNNING_VAR = 2, ILSX_BNCAT_ADAM_M = 3, ILSX_BNCAT_ADAM_V = 4 };
int ilsx_bncat_create(ilsx_ctx* ctx, int in_dim, int hidden, int n_blocks, int n_classes, int max_rows, ilsx_bncat** out);
int ilsx_bncat_destroy(ilsx_bncat* b);
int ilsx_bncat_num_params(const ilsx_bncat* b, int* n);
int ilsx_bncat_get(ilsx_bncat* b, int which, float* dst_host, size_t n);          /* which: ILSX_BNCAT_*; n must match */
int ilsx_bncat_set(ilsx_bncat* b, int which, const float* src_host, size_t n);
int ilsx_bncat_get_meta(const ilsx_bncat* b, int64_t* t, uint64_t* draws);      /* Adam step count, stochastic act calls so far */
int ilsx_bncat_set_meta(ilsx_bncat* b, int64_t t, uint64_t draws);
int ilsx_bncat_input(ilsx_bncat* b, float** X, int32_t** label);               /* the device input buffer the train step reads */
/* gcsl.py:87-103 in CLASS mode on the input buffer: train-mode forward, CrossEntropyLoss, one running-statistics update, Adam(lr) over
 * every parameter.  stats2_host (nullable, syncs): {CE Loss, Accuracy}. */
int ilsx_bncat_train_step(ilsx_bncat* b, int B, float lr, float* stats2_host);
/* eval mode: act[rows] (device, float index) = first argmax of the softmax (deterministic) or a Philox Gumbel-max draw from it;
 * probs (device [rows][n_classes], nullable). */
int ilsx_bncat_act(ilsx_bncat* b, const float* x, int rows, int deterministic, float* act, float* probs);
/* GCSL.train_step (gcsl.py:58-103): CLASS mode on an ilsx_bncat; MSE mode on an ilsx_bc in ILSX_BC_MSE mode whose noise is held at
 * zero (its action is then tanh(mean): the reference's max_act * tanh(last_fc) for max_act 1; the log-std head gets no gradient). */
typedef struct ilsx_gcsl ilsx_gcsl;
enum { ILSX_GCSL_MSE = 1, ILSX_GCSL_CLASS = 2 };
typedef struct { int32_t mode; float policy_lr; int32_t max_batch, d_obs, d_goal, horizon; } ilsx_gcsl_cfg;
int ilsx_gcsl_create(ilsx_ctx* ctx, const ilsx_gcsl_cfg* cfg, ilsx_bncat* cat, ilsx_bc* bc, int act_dim, ilsx_gcsl** out);
int ilsx_gcsl_destroy(ilsx_gcsl* g);
/* gather (ilsx_her_horizon_gather) straight into the trainer's input, then one step; stats2_host (nullable, syncs): CLASS {CE Loss,
 * Accuracy}, MSE {MSE, 0} */
int ilsx_gcsl_train_from_replay(ilsx_gcsl* g, ilsx_replay* rb, const int64_t* idx, const int64_t* idx_relabel, int B, float* stats2_host);
/* one step on device X[B, d_obs + d_goal + horizon] and targets (CLASS: int32 [B]; MSE: float [B, act_dim]) */
int ilsx_gcsl_train_step(ilsx_gcsl* g, const float* X, const void* target, int B, float* stats2_host);

#ifdef __cplusplus
}
#endif
#endif /* ILSX_H */
