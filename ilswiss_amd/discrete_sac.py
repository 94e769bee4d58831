"""Discrete SAC over libilsx: the reference's `DiscreteSoftActorCritic` (rlkit/torch/algorithms/discrete_sac/discrete_sac.py:13-201)
with its policy `DiscretePolicy` (networks.DiscretePolicy, policies.py:39-101).  Constructor kwargs are the YAML `sac_params` keys of
exp_specs/sac/sac_cartpole_d.yaml; unknown keys are swallowed like the reference's **kwargs.  The step runs in HIP (ilsx_ac.hip
ilsx_dsac_*, csrc/dsac.h): this class only moves data.
"""
from collections import OrderedDict

import numpy as np

from . import _lib
from .device import batch_ptrs
from .trainer import DeviceTrainer, check_swallowed_kwargs, stat_block


class DiscreteSoftActorCritic(DeviceTrainer):
    ABI, Stats = "dsac", _lib.DsacStats
    WHICH = dict(qf1=0, qf2=1, policy=2, target_qf1=3, target_qf2=4)
    SNAPSHOT_KEYS = ("qf1", "qf2", "policy", "target_qf1", "target_qf2")   # discrete_sac.py:191-198
    OPT = (("qf1", 0), ("qf2", 1), ("policy", 2))

    def __init__(self, policy, qf1, qf2, reward_scale=1.0, discount=0.99, alpha=1.0, policy_lr=1e-3, qf_lr=1e-3, vf_lr=1e-3,
                 soft_target_tau=1e-2, beta_1=0.9, max_batch=1024, **kwargs):
        # vf_lr is accepted and, as in the reference (discrete_sac.py:31 takes it, nothing reads it), unused: there is no V network
        check_swallowed_kwargs(kwargs, "DiscreteSoftActorCritic")
        self.policy, self.qf1, self.qf2, self.ctx = policy, qf1, qf2, policy.ctx
        self.reward_scale, self.discount, self.alpha = reward_scale, discount, alpha
        cfg = _lib.DsacCfg(discount, reward_scale, alpha, soft_target_tau, policy_lr, qf_lr, beta_1, int(max_batch))
        self._create(cfg, policy.h, qf1.h, qf2.h)

    def train_step(self, batch):   # discrete_sac.py:60-175; batch["actions"]: [B, 1] action indices
        keep = []
        batch = dict(batch, actions=np.asarray(batch["actions"], np.float32).reshape(-1, 1))
        B, p, _ = batch_ptrs(self.ctx, batch, keep)
        self._call("train_step", *p, B, keep=keep)

    def _fill_stats(self):   # discrete_sac.py:152-175
        s, st = self._stats, OrderedDict()
        st["Reward Scale"] = self.reward_scale
        st["QF1 Loss"], st["QF2 Loss"], st["Policy Loss"] = float(s.qf1_loss), float(s.qf2_loss), float(s.policy_loss)
        stat_block(st, "Q1 Predictions", s.q1_pred)
        stat_block(st, "Q2 Predictions", s.q2_pred)
        self.eval_statistics = st

    @property
    def networks(self):   # discrete_sac.py:177-185 (the targets live inside the library: get_flat_params("target_qf1"))
        return [self.policy, self.qf1, self.qf2]
