"""SAC with a state-value function over libilsx: the reference's `rlkit/torch/algorithms/sac/sac.py:13-262`
(`SoftActorCritic` of sac_exp_script.py).  Named SoftActorCriticV here because `ilswiss_amd.sac.SoftActorCritic` is
the twin-Q / learned-alpha trainer (sac_alpha.py) that the BASELINE configs use.  Constructor kwargs are the YAML
`sac_params` keys; unknown keys are swallowed like the reference's **kwargs.
"""
from collections import OrderedDict

from . import _lib
from .device import batch_ptrs
from .trainer import DeviceTrainer, check_swallowed_kwargs, stat_block


class SoftActorCriticV(DeviceTrainer):
    ABI, Stats = "sacv", _lib.SacvStats
    WHICH = dict(qf1=0, qf2=1, vf=2, policy=3, target_vf=6, q1=0, q2=1, pi=3, tvf=6)
    SNAPSHOT_KEYS = ("qf1", "qf2", "policy", "vf", "target_vf")   # sac.py:245-270
    OPT = (("qf1", 0), ("qf2", 1), ("vf", 2), ("policy", 3))

    def __init__(self, policy, qf1, qf2, vf, reward_scale=1.0, discount=0.99, alpha=1.0, policy_lr=1e-3, qf_lr=1e-3,
                 vf_lr=1e-3, soft_target_tau=1e-2, policy_mean_reg_weight=1e-3, policy_std_reg_weight=1e-3, beta_1=0.9,
                 max_batch=1024, **kwargs):
        check_swallowed_kwargs(kwargs, "SoftActorCriticV")
        self.policy, self.qf1, self.qf2, self.vf, self.ctx = policy, qf1, qf2, vf, policy.ctx
        self.reward_scale = reward_scale
        cfg = _lib.SacvCfg(reward_scale, discount, alpha, policy_lr, qf_lr, vf_lr, soft_target_tau, policy_mean_reg_weight,
                           policy_std_reg_weight, beta_1, int(max_batch))
        self._create(cfg, policy.h, qf1.h, qf2.h, vf.h)

    def train_step(self, batch, eps=None):
        keep = []
        B, p, dev = batch_ptrs(self.ctx, batch, keep)
        self._call("train_step", *p, B, dev(eps) if eps is not None else None, keep=keep)

    def _fill_stats(self):  # sac.py:181-240
        s, st = self._stats, OrderedDict()
        st["Reward Scale"] = self.reward_scale
        st["QF1 Loss"], st["QF2 Loss"], st["VF Loss"], st["Policy Loss"] = s.qf1_loss, s.qf2_loss, s.vf_loss, s.policy_loss
        for name, vals in (("Q1 Predictions", s.q1_pred), ("Q2 Predictions", s.q2_pred), ("V Predictions", s.v_pred),
                           ("Log Pis", s.log_pi), ("Policy mu", s.policy_mu), ("Policy log std", s.policy_log_std)):
            stat_block(st, name, vals)
        self.eval_statistics = st

    @property
    def networks(self):
        return [self.policy, self.qf1, self.qf2, self.vf]

    def _num_params(self, which):
        return {0: self.qf1, 1: self.qf2, 2: self.vf, 3: self.policy}[which % 4].num_params
