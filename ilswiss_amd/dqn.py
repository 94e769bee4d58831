"""DQN and Double DQN over libilsx: the reference's `DQN` / `DoubleDQN` (rlkit/torch/algorithms/dqn/dqn.py:16-130, double_dqn.py:11-51), its
acting policy `ArgmaxDiscretePolicy` (rlkit/policies/argmax.py) and the `EpsilonGreedy` strategy it is wrapped with
(rlkit/exploration_strategies/epsilon_greedy.py).  The reference class is trainer and loop in one (and does not import: dqn.py:13 names a
module that no longer exists); here the trainer is this class and the loop is DeviceRLAlgorithm, as for DDPG.  The step runs in HIP
(ilsx_ac.hip ilsx_dqn_*, csrc/dqn.h): these classes only move data.
"""
from collections import OrderedDict

import numpy as np

from . import _lib
from .device import as_dev, batch_ptrs
from .trainer import DeviceTrainer, check_swallowed_kwargs, stat_block


class ArgmaxDiscretePolicy:
    """argmax.py:10-21 with epsilon_greedy.py:21-24 folded in: the acting face of `qf` itself, not a copy — the trainer updates the very
    network the env acts with.  Constructing it puts the epsilon-greedy mark on the network (ilsx_net_set_epsilon_greedy): with probability
    epsilon a uniform action (which may be the greedy one), otherwise the first maximal Q-value; deterministic calls take the argmax.
    Actions are indices in an [n, 1] float column, like DiscretePolicy's."""

    def __init__(self, qf, epsilon=0.0):
        self.qf, self.epsilon = qf, float(epsilon)
        self.obs_dim, self.action_dim = qf.input_size, qf.output_size
        _lib.check(qf.ctx.lib.ilsx_net_set_epsilon_greedy(qf.h, 1, self.epsilon))

    @property
    def h(self):
        return self.qf.h

    @property
    def ctx(self):
        return self.qf.ctx

    def copy(self, ctx=None):
        return ArgmaxDiscretePolicy(self.qf.copy(ctx), self.epsilon)

    def get_flat_params(self):
        return self.qf.get_flat_params()

    def set_flat_params(self, flat):
        self.qf.set_flat_params(flat)

    def get_actions_dev(self, obs_ptr, n, deterministic=False):
        act = self.ctx.empty((n, 1))
        _lib.check(self.ctx.lib.ilsx_policy_act(self.h, obs_ptr, n, int(bool(deterministic)), None, act.ptr, None))
        return act

    def get_actions(self, obs_np, deterministic=False):
        obs_np = np.ascontiguousarray(obs_np, np.float32)
        keep, p = as_dev(self.ctx, obs_np)
        return self.get_actions_dev(p, obs_np.shape[0], deterministic).numpy()

    def get_action(self, obs_np, deterministic=False):   # argmax.py:16-21
        return self.get_actions(np.asarray(obs_np)[None], deterministic=deterministic)[0], {}

    def set_num_steps_total(self, t):
        pass


class DQN(DeviceTrainer):
    ABI, Stats = "dqn", _lib.DqnStats
    WHICH = dict(qf=0, target_qf=1)
    SNAPSHOT_KEYS = ("qf", "target_qf")
    OPT = (("qf", 0),)
    DOUBLE_Q = False

    def __init__(self, qf, policy=None, learning_rate=1e-3, use_hard_updates=False, hard_update_period=1000, tau=0.001, epsilon=0.1,
                 qf_criterion=None, optimizer_class=None, discount=0.99, max_batch=1024, **kwargs):
        # dqn.py:17-29's keywords and defaults; `discount` is TorchRLAlgorithm's (the step reads self.discount, dqn.py:80)
        check_swallowed_kwargs(dict(kwargs, optimizer_class=optimizer_class, qf_criterion=qf_criterion), type(self).__name__)
        self.qf, self.ctx = qf, qf.ctx
        # dqn.py:43-51: ONE acting object — exploration is its stochastic form, evaluation its deterministic one (MakeDeterministic); a policy
        # handed in keeps the epsilon it was built with
        self.policy = policy if policy is not None else ArgmaxDiscretePolicy(qf, epsilon)
        self.discount = float(discount)
        cfg = _lib.DqnCfg(float(discount), float(learning_rate), float(tau), int(bool(use_hard_updates)), int(hard_update_period),
                          int(self.DOUBLE_Q), int(max_batch))
        self._create(cfg, qf.h)

    def train_step(self, batch):   # dqn.py:67-105; batch["actions"]: [B, 1] action indices
        keep = []
        batch = dict(batch, actions=np.asarray(batch["actions"], np.float32).reshape(-1, 1))
        B, p, _ = batch_ptrs(self.ctx, batch, keep)
        self._call("train_step", *p, B, keep=keep)

    def _num_params(self, which):
        return self.qf.num_params

    def _fill_stats(self):   # dqn.py:97-105
        s, st = self._stats, OrderedDict()
        st["QF Loss"] = float(s.qf_loss)
        stat_block(st, "Y Predictions", s.y_pred)
        self.eval_statistics = st

    @property
    def networks(self):   # dqn.py:125-130 (the target lives inside the library: get_flat_params("target_qf"))
        return [self.qf]


class DoubleDQN(DQN):   # double_dqn.py:11-51: the target net is read at the online net's best action
    DOUBLE_Q = True
