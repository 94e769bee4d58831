"""Discrete SAC over libilsx: the reference's `DiscreteSoftActorCritic` (rlkit/torch/algorithms/discrete_sac/discrete_sac.py:13-201)
with its policy `DiscretePolicy` (networks.DiscretePolicy, policies.py:39-101).  Constructor kwargs are the YAML `sac_params` keys of
exp_specs/sac/sac_cartpole_d.yaml; unknown keys are swallowed like the reference's **kwargs.  The step runs in HIP (ilsx_ac.hip
ilsx_dsac_*, csrc/dsac.h): this class only moves data.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .sac import Trainer, check_swallowed_kwargs
from .td3 import _batch_ptrs, _stat_block


class DiscreteSoftActorCritic(Trainer):
    WHICH = dict(qf1=0, qf2=1, policy=2, target_qf1=3, target_qf2=4)

    def __init__(self, policy, qf1, qf2, reward_scale=1.0, discount=0.99, alpha=1.0, policy_lr=1e-3, qf_lr=1e-3, vf_lr=1e-3,
                 soft_target_tau=1e-2, beta_1=0.9, max_batch=1024, **kwargs):
        # vf_lr is accepted and, as in the reference (discrete_sac.py:31 takes it, nothing reads it), unused: there is no V network
        check_swallowed_kwargs(kwargs, "DiscreteSoftActorCritic")
        self.policy, self.qf1, self.qf2, self.ctx = policy, qf1, qf2, policy.ctx
        self.reward_scale, self.discount, self.alpha = reward_scale, discount, alpha
        cfg = _lib.DsacCfg(discount, reward_scale, alpha, soft_target_tau, policy_lr, qf_lr, beta_1, int(max_batch))
        self.h = C.c_void_p()
        _lib.check(self.ctx.lib.ilsx_dsac_create(self.ctx.h, C.byref(cfg), policy.h, qf1.h, qf2.h, C.byref(self.h)))
        self.eval_statistics = None
        self._stats = _lib.DsacStats()

    def train_step(self, batch):   # discrete_sac.py:60-175; batch["actions"]: [B, 1] action indices
        keep = []
        batch = dict(batch, actions=np.asarray(batch["actions"], np.float32).reshape(-1, 1))
        B, p, _ = _batch_ptrs(self.ctx, batch, keep)
        want = self.eval_statistics is None
        _lib.check(self.ctx.lib.ilsx_dsac_train_step(self.h, *p, B, C.byref(self._stats) if want else None))
        if want:
            self._fill_stats()
        else:
            self.ctx.sync()

    def train_from_replay(self, replay_buffer, n_steps, batch_size):
        want = self.eval_statistics is None
        _lib.check(self.ctx.lib.ilsx_dsac_train_from_replay(self.h, replay_buffer.h, int(n_steps), int(batch_size),
                                                            C.byref(self._stats) if want else None))
        if want:
            self._fill_stats()

    def _fill_stats(self):   # discrete_sac.py:152-175
        s, st = self._stats, OrderedDict()
        st["Reward Scale"] = self.reward_scale
        st["QF1 Loss"], st["QF2 Loss"], st["Policy Loss"] = float(s.qf1_loss), float(s.qf2_loss), float(s.policy_loss)
        _stat_block(st, "Q1 Predictions", s.q1_pred)
        _stat_block(st, "Q2 Predictions", s.q2_pred)
        self.eval_statistics = st

    def get_eval_statistics(self):
        return self.eval_statistics

    def end_epoch(self):
        self.eval_statistics = None

    def set_num_steps_total(self, num):
        pass

    @property
    def networks(self):   # discrete_sac.py:177-185 (the targets live inside the library: get_flat_params("target_qf1"))
        return [self.policy, self.qf1, self.qf2]

    def get_flat_params(self, name):
        w = self.WHICH[name]
        out = np.empty(self.policy.num_params if w == 2 else self.qf1.num_params, np.float32)
        _lib.check(self.ctx.lib.ilsx_dsac_get_params(self.h, w, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def set_flat_params(self, name, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        _lib.check(self.ctx.lib.ilsx_dsac_set_params(self.h, self.WHICH[name], flat.ctypes.data_as(C.c_void_p), flat.size))

    def get_snapshot(self):   # discrete_sac.py:191-198, as plain arrays (+ the three optimisers' Adam state, like td3.py:185-196)
        from .snapshot import get_opt
        snap = {k: self.get_flat_params(k) for k in ("qf1", "qf2", "policy", "target_qf1", "target_qf2")}
        for k, w in (("qf1", 0), ("qf2", 1), ("policy", 2)):
            snap[k + "_optimizer"] = get_opt(self.ctx.lib, "dsac", self.h, snap[k].size, w)
        return snap

    def load_snapshot(self, snap):
        from .snapshot import set_opt
        for k in ("qf1", "qf2", "policy", "target_qf1", "target_qf2"):
            self.set_flat_params(k, snap[k])
        for k, w in (("qf1", 0), ("qf2", 1), ("policy", 2)):
            if k + "_optimizer" in snap:
                set_opt(self.ctx.lib, "dsac", self.h, snap[k + "_optimizer"], w)
