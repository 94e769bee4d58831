"""DDPG over libilsx: the reference's `DDPG` trainer (rlkit/torch/algorithms/ddpg/ddpg.py:16-235), its deterministic policy `MlpPolicy`
(rlkit/torch/common/policies.py:106-127) and the exploration strategies it is driven by (rlkit/exploration_strategies/ou_strategy.py,
gaussian_strategy.py, base.py:39-72).  The strategies run on the device, ONE process per env (include/ilsx.h ilsx_vecenv_explore); the
classes here only carry their parameters to the training env.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .device import as_dev, batch_ptrs
from .td3 import MlpGaussianNoisePolicy
from .trainer import DeviceTrainer, check_swallowed_kwargs, stat_block


class MlpPolicy(MlpGaussianNoisePolicy):
    """policies.py:106-127: a deterministic Mlp, `output_activation(last_fc(h))` — the noise policy with noise 0."""

    def __init__(self, hidden_sizes, obs_dim, action_dim, init_w=1e-3, output_activation="identity", **kwargs):
        super().__init__(hidden_sizes, obs_dim, action_dim, init_w=init_w, policy_noise=0.0, policy_noise_clip=0.0, max_act=1.0,
                         output_activation=output_activation, **kwargs)


class DDPG(DeviceTrainer):
    ABI, Stats = "ddpg", _lib.DdpgStats
    WHICH = dict(qf=0, policy=1, target_qf=2, target_policy=3)
    SNAPSHOT_KEYS = ("qf", "policy", "target_policy", "target_qf")   # ddpg.py:237-246 (+ target_qf, which a resumed run needs)
    OPT = (("qf", 0), ("policy", 1))

    def __init__(self, policy, qf, policy_lr=1e-4, qf_lr=1e-3, qf_weight_decay=0, target_update_period=1000, soft_target_tau=1e-2,
                 use_soft_update=False, qf_criterion=None, residual_gradient_weight=0, epoch_discount_schedule=None,
                 eval_with_target_policy=False, policy_pre_activation_weight=0.0, optimizer_class=None, obs_normalizer=None,
                 action_normalizer=None, num_paths_for_normalization=0, min_q_value=-np.inf, max_q_value=np.inf, discount=0.99,
                 max_batch=1024, **kwargs):
        # `discount` is a keyword here: the reference reads self.discount (ddpg.py:140) and never sets it
        check_swallowed_kwargs(dict(kwargs, optimizer_class=optimizer_class, qf_criterion=qf_criterion), "DDPG")
        if residual_gradient_weight:   # ddpg.py:147-163 backpropagates through a policy that has already stepped in place
            raise NotImplementedError("DDPG(residual_gradient_weight > 0) is not implemented")
        for name, val in (("obs_normalizer", obs_normalizer), ("action_normalizer", action_normalizer),
                          ("num_paths_for_normalization", num_paths_for_normalization),
                          ("epoch_discount_schedule", epoch_discount_schedule), ("eval_with_target_policy", eval_with_target_policy)):
            if val:
                raise NotImplementedError(f"DDPG({name}={val!r}) is not implemented")
        self.policy, self.qf, self.ctx = policy, qf, policy.ctx
        self.discount = float(discount)
        cfg = _lib.DdpgCfg(float(discount), float(policy_lr), float(qf_lr), float(qf_weight_decay), float(soft_target_tau),
                           int(bool(use_soft_update)), int(target_update_period), float(policy_pre_activation_weight),
                           float(min_q_value), float(max_q_value), float(policy.max_act), int(max_batch))
        self._create(cfg, policy.h, qf.h)

    def train_step(self, batch):
        keep = []
        B, p, _ = batch_ptrs(self.ctx, batch, keep)
        self._call("train_step", *p, B, keep=keep)

    def _num_params(self, which):
        return (self.policy if which in (1, 3) else self.qf).num_params

    def _fill_stats(self):  # ddpg.py:187-225
        s, st = self._stats, OrderedDict()
        st["QF Loss"], st["Policy Loss"], st["Raw Policy Loss"] = s.qf_loss, s.policy_loss, s.raw_policy_loss
        st["Preactivation Policy Loss"] = s.preactivation_policy_loss
        for name, vals in (("Q Predictions", s.q_pred), ("Q Targets", s.q_target), ("Bellman Errors", s.bellman),
                           ("Policy Action", s.policy_action)):
            stat_block(st, name, vals)
        self.eval_statistics = st

    @property
    def networks(self):
        return [self.policy, self.qf]


# ---------------------------------------------------------------------------------------------- exploration strategies
def _uniform_bounds(action_space):
    assert len(action_space.shape) == 1   # ou_strategy.py:28, gaussian_strategy.py:16
    low, high = np.asarray(action_space.low, np.float64), np.asarray(action_space.high, np.float64)
    if np.any(low != low.flat[0]) or np.any(high != high.flat[0]):
        raise NotImplementedError("exploration strategies: the device kernel clips to one (low, high) pair for all action components")
    return float(low.flat[0]), float(high.flat[0])


class OUStrategy:
    """ou_strategy.py:8-60, the single-env form, one process per env of the vec env it is installed on: dx = theta (mu - x) + sigma N(0,1)
    with the sigma of the previous call, sigma annealed from max_sigma to min_sigma over decay_period steps of `t`, the state back at mu at
    every episode start.  (The reference's batched get_actions_from_raw_actions neither advances the state nor anneals sigma and is not
    reproduced: DESIGN.md section 6.)"""
    KIND = 2

    def __init__(self, action_space, mu=0, theta=0.15, max_sigma=0.3, min_sigma=0.3, decay_period=100000):
        if min_sigma is None:
            min_sigma = max_sigma
        self.mu, self.theta, self._max_sigma, self._min_sigma, self._decay_period = mu, theta, max_sigma, min_sigma, decay_period
        self.low, self.high = _uniform_bounds(action_space)

    def cfg(self):
        return _lib.ExploreCfg(self.KIND, 0, float(self.mu), float(self.theta), float(self._max_sigma), float(self._min_sigma),
                               float(self._decay_period), self.low, self.high)


class GaussianStrategy:
    """gaussian_strategy.py:6-33: clip(action + N(0,1) * sigma(t), low, high), sigma annealed like OUStrategy's."""
    KIND = 1

    def __init__(self, action_space, max_sigma=1.0, min_sigma=None, decay_period=1000000):
        if min_sigma is None:
            min_sigma = max_sigma
        self._max_sigma, self._min_sigma, self._decay_period = max_sigma, min_sigma, decay_period
        self.low, self.high = _uniform_bounds(action_space)

    def cfg(self):
        return _lib.ExploreCfg(self.KIND, 0, 0.0, 0.0, float(self._max_sigma), float(self._min_sigma), float(self._decay_period),
                               self.low, self.high)


class PolicyWrappedWithExplorationStrategy:
    """base.py:39-72.  `.h` is the wrapped policy's handle, so the fused rollout runs the policy as it is; the strategy is installed on
    the training env at its first rollout_step (HipVectorEnv calls `before_rollout_step`) and the library applies it to the policy's
    actions there.  Host callers of get_actions go through the same kernel on the env the strategy is installed on."""

    def __init__(self, exploration_strategy, policy):
        self.es, self.policy, self.t = exploration_strategy, policy, 0
        self.env = None

    @property
    def h(self):
        return self.policy.h

    @property
    def ctx(self):
        return self.policy.ctx

    def install(self, env):
        if self.env is not None and self.env is not env:   # installing restarts every process of the env: never done behind the caller's back
            raise RuntimeError("PolicyWrappedWithExplorationStrategy: the strategy is already installed on another vec env; one wrapper "
                               "drives one training env (build a second wrapper for a second env)")
        cfg = self.es.cfg()
        _lib.check(env.ctx.lib.ilsx_vecenv_set_exploration(env.h, C.byref(cfg)))
        self.env = env

    def before_rollout_step(self, env):
        if self.env is not env:   # first step on this env (install refuses a second one)
            self.install(env)
        _lib.check(env.ctx.lib.ilsx_vecenv_set_exploration_t(env.h, int(self.t)))

    def set_num_steps_total(self, t):
        self.t = t

    def get_actions(self, obs_np, deterministic=False):
        if deterministic:
            return self.policy.get_actions(obs_np, deterministic=True)
        obs = np.ascontiguousarray(obs_np, np.float32)
        if self.env is None or obs.shape[0] != self.env.env_num:
            raise RuntimeError("PolicyWrappedWithExplorationStrategy.get_actions: the strategy keeps one process per env of the vec env it "
                               "is installed on (install(env)); pass that env's batch of observations")
        keep, p = as_dev(self.ctx, obs)
        act = self.ctx.empty((obs.shape[0], self.policy.action_dim))
        lib = self.ctx.lib
        _lib.check(lib.ilsx_policy_act(self.policy.h, p, obs.shape[0], 1, None, act.ptr, None))
        _lib.check(lib.ilsx_vecenv_explore(self.env.h, act.ptr, None, int(self.t)))
        return act.numpy()

    def get_action(self, obs_np, deterministic=False):
        return self.get_actions(np.asarray(obs_np)[None], deterministic)[0], {}

    def reset(self):   # episode starts are the env's: a process whose env begins an episode goes back to mu on the device
        pass
