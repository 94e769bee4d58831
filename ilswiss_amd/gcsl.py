"""Goal-conditioned supervised learning on libilsx: the reference's `GCSL` trainer (rlkit/torch/algorithms/gcsl/gcsl.py), its horizon
relabel buffer (rlkit/data_management/relabel_horizon_replay_buffer.py), its loop (`GoalHorizonRL`, gcsl/rl.py) and its two policies
(`CatagorialConditionPolicy(batch_norm=True)` for CLASS mode, `MlpGaussianAndEpsilonConditionPolicy` for MSE mode; policies.py).

The policy input is observation | desired_goal | horizon, the horizon a 0/1 row of length T = max_path_length: `arange(T) >= T-1-t` while
acting at step t of an episode, `arange(T) >= idx_relabel - idx` in the buffer (raw ring indices: a trajectory that wraps the ring gives
an all-ones row — the reference's behaviour, kept).  `DeviceHindsightHorizonReplayBuffer` draws the reference's indices on the host and the
trainer gathers the batch on the device straight into its input (ilsx_her_horizon_gather); no batch crosses PCIe.

CLASS mode trains the device BatchNorm categorical policy (ilsx_bncat: Linear -> BatchNorm1d -> ReLU blocks, cross-entropy, Adam over every
parameter, running statistics).  MSE mode reuses behaviour cloning's MSE loss and kernels (ilsx_bc) on a tanh policy whose noise is held at
zero.  The reference's MSE policy registers BatchNorm modules that its forward never applies: the net here has none."""
import ctypes as C
import random
from collections import OrderedDict

import numpy as np

from . import _lib
from .device import as_dev, get_context, host_ptr
from .her import HER, DeviceHindsightReplayBuffer, HindsightReplayBuffer
from .networks import ReparamTanhMultivariateGaussianPolicy
from .trainer import DeviceTrainer, check_swallowed_kwargs


def horizon_row(T, t):
    """gcsl/rl.py:105-111 (and vec_sampler.py:24-27): the temperature encoding at step t of an episode."""
    return (np.arange(T) >= (T - 1 - t)).astype(np.float32)


def _flat(obs, observation_key="observation", desired_goal_key="desired_goal"):
    if isinstance(obs, dict):
        return np.concatenate([obs[observation_key], obs[desired_goal_key]], -1)
    return np.asarray(obs)


# -------------------------------------------------------------------------------------------------------------------- buffers
def _draw(buf, batch_size):
    """relabel_horizon_replay_buffer.py:177-206 (her_ratio 1: every row relabelled): the reference's RandomState call order for the
    trajectory and step draws, the GLOBAL numpy stream for `future`."""
    keys_list = list(buf._traj_endpoints.keys())
    starts = buf._np_rand_state.choice(keys_list, size=len(keys_list), replace=False)
    ends = [buf._traj_endpoints[k] for k in starts]
    traj_indice = buf._np_rand_state.randint(0, len(starts), batch_size)
    indices, indices_relabel = [], []
    for i in traj_indice:
        traj_len = (ends[i] - starts[i]) % buf._size
        step = (buf._np_rand_state.randint(0, traj_len, 1)[0] + starts[i]) % buf._size
        indices.append(step)
        fut = np.random.randint(step, traj_len + starts[i]) % buf._size     # eager dict literal: drawn whatever the relabel_type
        indices_relabel.append(ends[i] - 1 if buf.relabel_type == "final" else fut)
    return np.asarray(indices, np.int64), np.asarray(indices_relabel, np.int64)


def horizons_of(idx, idx_relabel, T):
    """relabel_horizon_replay_buffer.py:243-247: horizons[b, j] = j >= idx_relabel[b] - idx[b] (no modulo)."""
    return (np.arange(T)[None, :] >= (np.asarray(idx_relabel) - np.asarray(idx))[:, None]).astype(np.float32)


class HindsightHorizonReplayBuffer(HindsightReplayBuffer):
    """The host form: HindsightReplayBuffer with her_ratio 1.0 plus `horizons` [B, max_path_length]."""

    def __init__(self, max_path_length=50, *args, **kwargs):
        kwargs["her_ratio"] = 1.0
        super().__init__(*args, **kwargs)
        self.max_path_length = int(max_path_length)
        self.last_indices = None

    def random_batch(self, batch_size, keys=None, **kwargs):
        idx, idx_rel = _draw(self, batch_size)
        self.last_indices = (idx, idx_rel)
        b = self._gather(idx)
        goal = self._gather(idx_rel, with_all=False)["next_observations"][self.achieved_goal_key]
        b["observations"][self.desired_goal_key][:] = goal
        b["next_observations"][self.desired_goal_key][:] = goal
        b["achieved_goals"] = b["observations"][self.achieved_goal_key]
        b["desired_goals"] = b["observations"][self.desired_goal_key]
        b["next_achieved_goals"] = b["next_observations"][self.achieved_goal_key]
        b["next_desired_goals"] = b["next_observations"][self.desired_goal_key]
        b["observations"] = b["observations"][self.observation_key]
        b["next_observations"] = b["next_observations"][self.observation_key]
        b["horizons"] = horizons_of(idx, idx_rel, self.max_path_length)
        b["rewards"] = np.asarray(self.compute_reward(b["next_achieved_goals"], b["desired_goals"], info=None)).reshape(-1, 1)
        return b


class DeviceHindsightHorizonReplayBuffer(DeviceHindsightReplayBuffer):
    """The device form: rows in the HBM ring of DeviceHindsightReplayBuffer, the reference's index draws on the host; `random_batch`
    uploads the 2 x B indices and returns them — the trainer gathers obs | goal | horizon and the actions on the device
    (ilsx_gcsl_train_from_replay).  Rewards are not computed: GCSL never reads them."""

    def __init__(self, max_path_length=50, *args, **kwargs):
        kwargs["her_ratio"] = 1.0
        super().__init__(*args, **kwargs)
        self.max_path_length = int(max_path_length)
        self.last_indices = None
        self._idx = None

    def random_batch(self, batch_size, keys=None, **kwargs):
        B = int(batch_size)
        idx, idx_rel = _draw(self, B)
        self.last_indices = (idx, idx_rel)
        if self._idx is None or self._idx[0].shape[0] != B:
            self._idx = (self.ctx.empty((B,), np.int64), self.ctx.empty((B,), np.int64))
        di, dr = self._idx
        di.copy_from(idx)
        dr.copy_from(idx_rel)
        return dict(_gcsl_indices=(di, dr, B), _ring=self)

    def gather(self, batch, mode, use_horizons=True):
        """The device gather of a batch (tests): X [B, d_obs + d_goal + T] and the actions (mode 0: floats [B, a]; mode 1: int32 [B])."""
        di, dr, B = batch["_gcsl_indices"]
        T = self.max_path_length if use_horizons else 0
        X = self.ctx.empty((B, self.d_obs + self.d_goal + T))
        tgt = self.ctx.empty((B, self._action_dim)) if mode == 0 else self.ctx.empty((B,), np.int32)
        _lib.check(self.ctx.lib.ilsx_her_horizon_gather(self.h, di.ptr, dr.ptr, B, self.d_obs, self.d_goal, T, int(mode), X.ptr,
                                                        tgt.ptr if mode == 0 else None, tgt.ptr if mode == 1 else None))
        return X, tgt


# -------------------------------------------------------------------------------------------------------------------- policies
def _bn_init(rng, D, H, nblk, n, init_w=1e-3, b_init=0.1):
    """CatagorialMlp(batch_norm=True)'s initialisation (networks.py:57-83): fanin_init on the hidden weights (bound 1/sqrt(size[0]),
    pytorch_util.py:20-29), biases b_init, BatchNorm1d gamma 1 / beta 0, last_fc U(+-init_w)."""
    parts, k = [], D
    for _ in range(nblk):
        parts += [rng.uniform(-1 / np.sqrt(H), 1 / np.sqrt(H), (H, k)).ravel(), np.full(H, b_init), np.ones(H), np.zeros(H)]
        k = H
    parts += [rng.uniform(-init_w, init_w, n * H), rng.uniform(-init_w, init_w, n)]
    return np.concatenate(parts).astype(np.float32)


class CatagorialConditionPolicy:
    """policies.py:759-840 with batch_norm=True, on the device (ilsx_bncat).  Acting is always in eval mode (running statistics), as the
    reference's loop puts the policy there outside `_try_to_train`; `train()` / `eval()` keep the mode flag for callers that read it.
    get_actions returns [n, 1] class indices: torch.multinomial's distribution by a Gumbel-max draw, argmax when deterministic."""

    def __init__(self, hidden_sizes, obs_dim, condition_dim, action_dim, init_w=1e-3, batch_norm=True, max_rows=1024, ctx=None, seed=None,
                 observation_key="observation", desired_goal_key="desired_goal", achieved_goal_key="achieved_goal", **kwargs):
        if not batch_norm:
            raise NotImplementedError("CatagorialConditionPolicy(batch_norm=False): GCSL's CLASS spec turns batch norm on")
        hs = [int(h) for h in hidden_sizes]
        if len(set(hs)) != 1 or not 1 <= len(hs) <= 3:
            raise NotImplementedError(f"hidden_sizes={hs}: 1..3 blocks of one width")
        if kwargs:
            raise TypeError(f"CatagorialConditionPolicy: unexpected keyword arguments {sorted(kwargs)}")
        self.ctx = ctx or get_context()
        self.obs_dim, self.condition_dim, self.action_dim = int(obs_dim), int(condition_dim), int(action_dim)
        self.d_obs = self.obs_dim
        self.input_dim, self.hidden, self.n_blocks = self.obs_dim + self.condition_dim, hs[0], len(hs)
        self.observation_key, self.desired_goal_key, self.achieved_goal_key = observation_key, desired_goal_key, achieved_goal_key
        self.max_rows, self.training = int(max_rows), True
        self.h = C.c_void_p()
        _lib.check(self.ctx.lib.ilsx_bncat_create(self.ctx.h, self.input_dim, self.hidden, self.n_blocks, self.action_dim, self.max_rows,
                                                  C.byref(self.h)))
        n = C.c_int()
        _lib.check(self.ctx.lib.ilsx_bncat_num_params(self.h, C.byref(n)))
        self.num_params = n.value
        rng = np.random.default_rng(np.random.randint(2 ** 31) if seed is None else seed)
        self.set_flat_params(_bn_init(rng, self.input_dim, self.hidden, self.n_blocks, self.action_dim, init_w))

    def _get(self, which, n):
        out = np.empty(n, np.float32)
        _lib.check(self.ctx.lib.ilsx_bncat_get(self.h, which, host_ptr(out), out.size))
        return out

    def _set(self, which, v):
        v = np.ascontiguousarray(v, np.float32).ravel()
        _lib.check(self.ctx.lib.ilsx_bncat_set(self.h, which, host_ptr(v), v.size))

    def get_flat_params(self):
        return self._get(0, self.num_params)

    def set_flat_params(self, flat):
        self._set(0, flat)

    def get_running_stats(self):
        nr = self.n_blocks * self.hidden
        return self._get(1, nr).reshape(self.n_blocks, self.hidden), self._get(2, nr).reshape(self.n_blocks, self.hidden)

    def set_running_stats(self, mean, var):
        self._set(1, mean), self._set(2, var)

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def set_num_steps_total(self, t):
        pass

    def _rows(self, obs):
        if isinstance(obs, dict) or (len(obs) and isinstance(obs[0], dict)):
            raise ValueError("CatagorialConditionPolicy: pass observation | desired_goal | horizon rows (GoalHorizonRL builds them)")
        return np.ascontiguousarray(np.atleast_2d(obs), np.float32)

    def probs(self, obs):
        """Eval-mode softmax [n, action_dim]."""
        x = self._rows(obs)
        keep, p = as_dev(self.ctx, x)
        out = self.ctx.empty((x.shape[0], self.action_dim))
        _lib.check(self.ctx.lib.ilsx_bncat_act(self.h, p, x.shape[0], 1, None, out.ptr))
        return out.numpy()

    def get_actions_dev(self, obs_ptr, n, deterministic=False):
        act = self.ctx.empty((n,))
        _lib.check(self.ctx.lib.ilsx_bncat_act(self.h, obs_ptr, n, int(bool(deterministic)), act.ptr, None))
        return act

    def get_actions(self, obs, deterministic=False):
        x = self._rows(obs)
        keep, p = as_dev(self.ctx, x)
        return self.get_actions_dev(p, x.shape[0], deterministic).numpy().astype(np.int64).reshape(-1, 1)

    def get_action(self, obs, deterministic=False):
        return self.get_actions(np.asarray(obs)[None], deterministic)[0], {}

    def get_snapshot(self):
        t, d = C.c_int64(), C.c_uint64()
        _lib.check(self.ctx.lib.ilsx_bncat_get_meta(self.h, C.byref(t), C.byref(d)))
        rm, rv = self.get_running_stats()
        return dict(params=self.get_flat_params(), running_mean=rm, running_var=rv, adam_m=self._get(3, self.num_params),
                    adam_v=self._get(4, self.num_params), meta=np.array([t.value, d.value], np.int64))

    def load_snapshot(self, snap):
        self.set_flat_params(snap["params"])
        self.set_running_stats(snap["running_mean"], snap["running_var"])
        self._set(3, snap["adam_m"]), self._set(4, snap["adam_v"])
        t, d = [int(v) for v in snap["meta"]]
        _lib.check(self.ctx.lib.ilsx_bncat_set_meta(self.h, t, d))

    def __del__(self):
        h = getattr(self, "h", None)   # a closed context has freed the object's memory with its own: nothing to destroy then
        if h is not None and h.value and getattr(self.ctx, "h", None):
            self.ctx.lib.ilsx_bncat_destroy(h)
            self.h = C.c_void_p()


class MlpGaussianAndEpsilonConditionPolicy(ReparamTanhMultivariateGaussianPolicy):
    """policies.py:480-566 + :645-700 for GCSL's MSE mode: the deterministic action is max_act * tanh(last_fc) (max_act 1), exploration is
    the HER policy's epsilon-uniform / clipped Gaussian on the host.  On the device it is a tanh policy whose log-std head is held at zero
    and whose noise is zero, so that behaviour cloning's MSE kernels train exactly the reference's loss; `get_flat_params` /
    `set_flat_params` speak the reference's single-head layout (BatchNorm modules excluded: its forward never applies them)."""

    def __init__(self, hidden_sizes, obs_dim, condition_dim, action_dim, action_space=None, epsilon=0.3, max_sigma=0.2, min_sigma=0.2,
                 decay_period=1000000, max_act=1.0, min_act=-1.0, output_activation="tanh", batch_norm=True,
                 observation_key="observation", desired_goal_key="desired_goal", achieved_goal_key="achieved_goal", **kwargs):
        if getattr(output_activation, "__name__", output_activation) != "tanh" or max_act != 1.0 or min_act != -1.0:
            raise NotImplementedError("GCSL MSE mode runs the spec's policy: output_activation tanh, max_act 1")
        super().__init__(hidden_sizes, obs_dim + condition_dim, action_dim, max_act=max_act, **kwargs)
        self.condition_dim, self.d_obs = int(condition_dim), int(obs_dim)
        self.sigma, self._max_sigma, self._min_sigma = max_sigma, max_sigma, (max_sigma if min_sigma is None else min_sigma)
        self._epsilon, self._decay_period, self._action_space = epsilon, decay_period, action_space
        self.min_act, self.t, self.training = min_act, 0, True
        self.observation_key, self.desired_goal_key, self.achieved_goal_key = observation_key, desired_goal_key, achieved_goal_key
        self._n_head = action_dim * self.hidden_sizes[-1] + action_dim     # the log-std head's words (the tail of the 2-head layout)
        self.set_flat_params(super().get_flat_params()[:-self._n_head])

    def get_flat_params(self):
        return super().get_flat_params()[:-self._n_head]

    def set_flat_params(self, flat):
        super().set_flat_params(np.concatenate([np.asarray(flat, np.float32), np.zeros(self._n_head, np.float32)]))

    def get_device_flat_params(self):
        """The whole 2-head vector the device trainer holds (the layout of its Adam state): snapshots."""
        return super().get_flat_params()

    def set_device_flat_params(self, flat):
        super().set_flat_params(flat)

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def set_num_steps_total(self, t):
        self.t = t

    def get_actions(self, obs, deterministic=False):
        x = np.ascontiguousarray(np.atleast_2d(obs), np.float32)
        action = super().get_actions(x, deterministic=True)
        if deterministic:
            return action
        if random.random() < self._epsilon:                                   # policies.py:537-552
            return np.array([self._action_space.sample() for _ in range(x.shape[0])], np.float32)
        self.sigma = self._max_sigma - (self._max_sigma - self._min_sigma) * min(1.0, self.t * 1.0 / self._decay_period)
        return np.clip(action + np.random.normal(size=action.shape) * self.sigma, self.min_act, self.max_act).astype(np.float32)

    def get_action(self, obs, deterministic=False):
        return self.get_actions(np.asarray(obs)[None], deterministic)[0], {}


# -------------------------------------------------------------------------------------------------------------------- trainer
_MODES = dict(MSE=1, CLASS=2)


class GCSL(DeviceTrainer):
    """gcsl.py:11-118.  `reward_scale`, `discount` (and `soft_target_tau` of the specs) are accepted and unused, as in the reference.
    Statistics: CLASS {"CE Loss", "Accuracy"}, MSE {"MSE"}, from the first batch after end_epoch."""
    ABI, Stats = "gcsl", C.c_float * 2

    def __init__(self, policy, mode="MSE", reward_scale=1.0, discount=0.99, policy_lr=1e-3, optimizer_class=None, use_horizons=False,
                 goal_dim=None, max_batch=256, **kwargs):
        """goal_dim: the desired goal's width (with use_horizons the policy's condition is goal | horizon and the two must be told apart)."""
        if mode == "MLE":
            raise NotImplementedError("GCSL mode 'MLE': no spec or script of the reference selects it")
        assert mode in _MODES, "Invalid mode!"
        check_swallowed_kwargs(dict(kwargs, optimizer_class=optimizer_class), "GCSL")
        self.policy, self.mode, self.ctx = policy, mode, policy.ctx
        self.reward_scale, self.discount, self.policy_lr, self.use_horizons = reward_scale, discount, float(policy_lr), bool(use_horizons)
        if goal_dim is None:
            if use_horizons:
                raise ValueError("GCSL(use_horizons=True) needs goal_dim: the condition is desired_goal | horizon")
            goal_dim = policy.condition_dim
        self.d_obs, self.d_goal = int(policy.d_obs), int(goal_dim)
        self.horizon = int(policy.condition_dim) - self.d_goal
        if self.horizon < 0 or (self.horizon and not use_horizons):
            raise ValueError(f"GCSL: condition_dim {policy.condition_dim} does not split into goal {self.d_goal} | horizon")
        self.max_batch = int(max_batch)
        self._bc = None
        bc_h = None
        if mode == "MSE":
            from .bc import BC
            self._bc = BC("MSE", policy, batch_size=self.max_batch, lr=self.policy_lr, momentum=0.9)   # Adam(lr), betas (0.9, 0.999)
            bc_h = self._bc.h
        elif policy.max_rows < self.max_batch:
            raise ValueError(f"GCSL: policy max_rows {policy.max_rows} < max_batch {self.max_batch}")
        cfg = _lib.GcslCfg(_MODES[mode], self.policy_lr, self.max_batch, self.d_obs, self.d_goal, self.horizon)
        self._create(cfg, policy.h if mode == "CLASS" else None, bc_h, int(policy.action_dim))
        self._n_train_steps_total = 0

    def _fill_stats(self):
        st = self._stats
        if self.mode == "CLASS":
            self.eval_statistics = OrderedDict([("CE Loss", float(st[0])), ("Accuracy", float(st[1]))])
        else:
            self.eval_statistics = OrderedDict([("MSE", float(st[0]))])

    def train_step(self, batch):
        if "_gcsl_indices" in batch:          # DeviceHindsightHorizonReplayBuffer: gathered on the device into the trainer's input
            di, dr, B = batch["_gcsl_indices"]
            self._call("train_from_replay", batch["_ring"].h, di.ptr, dr.ptr, B)
        else:
            parts = [np.asarray(batch["observations"], np.float32), np.asarray(batch["desired_goals"], np.float32)]
            if self.horizon:
                parts.append(np.asarray(batch["horizons"], np.float32))
            X = np.ascontiguousarray(np.concatenate(parts, -1), np.float32)
            a = np.asarray(batch["actions"])
            tgt = (np.ascontiguousarray(a.reshape(-1).astype(np.float32).astype(np.int32)) if self.mode == "CLASS"
                   else np.ascontiguousarray(a, np.float32))
            kx, px = as_dev(self.ctx, X)
            kt, pt = as_dev(self.ctx, tgt, tgt.dtype)
            self._call("train_step", px, pt, X.shape[0], keep=(kx, kt))
        self._n_train_steps_total += 1

    @property
    def networks(self):
        return [self.policy]

    def get_snapshot(self):
        """CLASS: parameters, running statistics, Adam state and counters of the policy.  MSE: the device trainer's whole 2-head parameter
        vector (log-std head included) with its Adam state, the layout ilsx_bc_get_opt speaks."""
        if self.mode == "CLASS":
            return dict(policy=self.policy.get_snapshot())
        flat = self.policy.get_device_flat_params()
        return dict(policy=dict(params=flat, optimizer=self._bc._get_opt(flat.size)))

    def load_snapshot(self, snap):
        if self.mode == "CLASS":
            self.policy.load_snapshot(snap["policy"])
        else:
            self.policy.set_device_flat_params(snap["policy"]["params"])
            self._bc._set_opt(snap["policy"]["optimizer"])

    def close(self):
        super().close()
        if self._bc is not None:   # MSE: the behaviour-cloning trainer this one steps
            self._bc.close()

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value and getattr(self.ctx, "h", None):
            self.ctx.lib.ilsx_gcsl_destroy(h)
            self.h = C.c_void_p()


# -------------------------------------------------------------------------------------------------------------------- loop
class GoalHorizonRL(HER):
    """gcsl/rl.py:12-229 over the HER loop for ONE host-side goal env: the policy sees observation | desired_goal | horizon (the temperature
    encoding of the remaining steps); it is in eval mode while acting and evaluating and in train mode only around the train calls
    (base_algorithm.py:294-299); evaluation is deterministic.  The buffer is the device horizon buffer when the trainer lives on a
    device context.  `eval_env` is the reference's separate evaluation env (gcsl_exp_script.py passes `env` and `training_env`); without
    one, evaluation borrows the training env, and the training episode it interrupts is closed in the buffer and restarted afterwards."""

    def __init__(self, trainer, env, exploration_policy, replay_buffer=None, relabel_type="future", use_horizons=False, max_path_length=50,
                 replay_buffer_size=100000, eval_deterministic=True, eval_env=None, **kwargs):
        assert max_path_length < replay_buffer_size
        for k in ("no_terminal", "wrap_absorbing", "save_best", "freq_saving", "save_replay_buffer", "her_ratio"):
            kwargs.pop(k, None)
        if replay_buffer is None:
            cls = DeviceHindsightHorizonReplayBuffer if hasattr(trainer, "ctx") else HindsightHorizonReplayBuffer
            kw = dict(ctx=trainer.ctx) if cls is DeviceHindsightHorizonReplayBuffer else {}
            if cls is DeviceHindsightHorizonReplayBuffer and getattr(env, "reward_type", "sparse") not in ("sparse", "dense"):
                cls, kw = HindsightHorizonReplayBuffer, {}
            replay_buffer = cls(max_path_length, replay_buffer_size, env, random_seed=np.random.randint(10000), relabel_type=relabel_type, **kw)
        super().__init__(trainer, env, exploration_policy, replay_buffer=replay_buffer, relabel_type=relabel_type,
                         max_path_length=max_path_length, replay_buffer_size=replay_buffer_size, **kwargs)
        self.use_horizons, self.eval_deterministic = bool(use_horizons), bool(eval_deterministic)
        self.eval_env = env if eval_env is None else eval_env
        self.policy.eval()

    def _input(self, obs, t):
        x = _flat(obs, self.policy.observation_key, self.policy.desired_goal_key)
        if self.use_horizons:
            x = np.concatenate([x, horizon_row(self.max_path_length, t)], -1)
        return np.asarray(x, np.float32)[None]

    def evaluate(self):
        """(success rate, mean return) over num_steps_per_eval deterministic steps (vec_sampler.py:24-27's horizon encoding)."""
        env = self.eval_env
        succ, rets, ret, n, obs, k = [], [], 0.0, 0, env.reset(), 0
        while n < self.num_steps_per_eval:
            a = self.policy.get_actions(self._input(obs, k), deterministic=self.eval_deterministic)[0]
            obs, r, d, info = env.step(a)
            n, k, ret = n + 1, k + 1, ret + r
            if d or k >= self.max_path_length:
                succ.append(info["is_success"]), rets.append(ret)
                obs, k, ret = env.reset(), 0, 0.0
        return (float(np.mean(succ)) if succ else 0.0), (float(np.mean(rets)) if rets else 0.0)

    def train(self):
        history, obs, k, since = [], self.env.reset(), 0, 0
        for epoch in range(self.num_epochs):
            for _ in range(self.num_steps_per_epoch):
                self.policy.set_num_steps_total(self._n_env_steps_total)
                a = self.policy.get_actions(self._input(obs, k))[0]
                nobs, r, d, info = self.env.step(a)
                self.replay_buffer.add_sample(obs, a, r, d, nobs)
                self._n_env_steps_total, k, since, obs = self._n_env_steps_total + 1, k + 1, since + 1, nobs
                if d or k >= self.max_path_length:
                    self.replay_buffer.terminate_episode()
                    obs, k = self.env.reset(), 0
                if since >= self.between and self.replay_buffer.num_steps_can_sample() >= self.min_steps and self.replay_buffer._traj_endpoints:
                    since = 0
                    self.policy.train()
                    for _ in range(self.per_call):
                        self.trainer.train_step(self.replay_buffer.random_batch(self.batch_size))
                        self._n_train_steps_total += 1
                    self.policy.eval()
            stats = dict(self.trainer.get_eval_statistics() or {})
            self.trainer.end_epoch()
            success, ret = self.evaluate()
            if self.eval_env is self.env:       # evaluation reset and stepped the training env: end the interrupted episode there
                self.replay_buffer.terminate_episode()
                obs, k = self.env.reset(), 0
            history.append(dict(stats, success=success, ret=ret))
        return history
