"""MBPO on the device: the probabilistic ensemble `BNN` (rlkit/torch/common/networks.py:149-279), its `BNNTrainer`
(rlkit/torch/algorithms/mbpo/bnn_trainer.py), `FakeEnv` (mbpo/fake_env.py) and the `MBPO` loop (mbpo/mbpo.py), with the
reference's class names and keywords.  The arithmetic is libilsx's ilsx_bnn_* / ilsx_mbpo_model_step (ilswiss_amd/csrc/bnn.h):
the dataset never leaves the replay ring, the model rollout never leaves the device, and the host reads back E floats per
training epoch and one survivor count per rollout step.

Read of the reference, kept on purpose: BNNTrainer._save_state stores `fc.weight.data` / `fc.bias.data`, aliases of the live
parameters, so _set_state loads the current weights into themselves — the trained model is the LAST epoch's weights, not the best
holdout epoch's."""
import ctypes as C
import time
from collections import OrderedDict

import numpy as np

from . import _lib
from .algorithm import DeviceRLAlgorithm, DeviceRLAlgorithmGroup
from .device import get_context, host_ptr
from .replay import EnvReplayBuffer, SimpleReplayBuffer
from .trainer import check_swallowed_kwargs

MAX_LOG_VAR, MIN_LOG_VAR = 0.5, -10.0


def default_weight_decays(num_hidden):
    """bnn_trainer.py:37-44"""
    return [2.5e-5, 5e-5] + [7.5e-5] * (num_hidden - 2) + [1e-4] if num_hidden > 2 else [2.5e-5, 1e-4]


def _off(ptr, nbytes):
    return C.c_void_p(ptr.value + int(nbytes))


class FixedNormalizer:
    """normalizer.py:81-114, its statistics held by the ensemble on the device (set_std adds eps as the reference does)."""

    def __init__(self, bnn, eps=1e-8):
        self._bnn, self.eps = bnn, eps

    def _get(self):
        n = self._bnn.input_size
        m, s = np.empty(n, np.float32), np.empty(n, np.float32)
        _lib.check(self._bnn.ctx.lib.ilsx_bnn_get_normalizer(self._bnn.h, host_ptr(m), host_ptr(s)))
        return m, s

    @property
    def mean(self):
        return self._get()[0]

    @property
    def std(self):
        return self._get()[1]

    def _set(self, mean, std):
        m = np.ascontiguousarray(mean, np.float32).reshape(-1)
        s = np.ascontiguousarray(std, np.float32).reshape(-1)
        _lib.check(self._bnn.ctx.lib.ilsx_bnn_set_normalizer(self._bnn.h, host_ptr(m), host_ptr(s)))

    def set_mean(self, mean):
        self._set(np.asarray(mean, np.float32) + np.zeros(self._bnn.input_size, np.float32), self.std)

    def set_std(self, std):
        self._set(self.mean, (np.asarray(std, np.float32) + self.eps) + np.zeros(self._bnn.input_size, np.float32))

    def normalize(self, v):
        m, s = self._get()
        return (np.asarray(v, np.float32) - m) / s


class BNN:
    """BNN(hidden_sizes, output_size, input_size, init_w=3e-3, num_nets=1): E members of SiLU layers on the device.  The trainer's
    optimiser settings live in the same library object (`_configure`, called by BNNTrainer)."""

    def __init__(self, hidden_sizes, output_size, input_size, init_w=3e-3, hidden_activation=None, output_activation=None,
                 hidden_init=None, b_init_value=0.1, layer_norm=False, layer_norm_kwargs=None, batch_norm=False,
                 batch_norm_before_output_activation=False, num_nets=1, ctx=None, seed=None):
        hidden_sizes = list(hidden_sizes)
        if not hidden_sizes or len(set(hidden_sizes)) != 1:
            raise NotImplementedError(f"BNN(hidden_sizes={hidden_sizes}): libilsx's ensemble has equal hidden widths")
        name = getattr(hidden_activation, "__name__", "silu") if hidden_activation is not None else "silu"
        if name != "silu" or output_activation not in (None,) and getattr(output_activation, "__name__", "") != "identity":
            raise NotImplementedError("BNN: libilsx implements SiLU hidden layers and an identity mean head (networks.py:174-175)")
        if layer_norm or batch_norm or batch_norm_before_output_activation or b_init_value != 0.1 or hidden_init is not None:
            raise NotImplementedError("BNN: layer / batch norm and other inits than fanin_init + 0.1 biases are not implemented")
        self.ctx = ctx or get_context()
        self.hidden_sizes, self.input_size, self.output_size = hidden_sizes, int(input_size), int(output_size)
        self.num_nets, self.init_w = int(num_nets), float(init_w)
        self.h = None
        self._cfg = dict(lr=1e-3, reward_scale=1.0, weight_decays=default_weight_decays(len(hidden_sizes)), max_batch=256)
        self._create()
        seed = int(np.random.randint(2**31)) if seed is None else int(seed)
        _lib.check(self.ctx.lib.ilsx_bnn_init(self.h, C.c_uint64(seed)))
        self.normalizer = FixedNormalizer(self)

    def _create(self):
        c = self._cfg
        wd = list(c["weight_decays"]) + [0.0] * (9 - len(c["weight_decays"]))
        cfg = _lib.BnnCfg(self.num_nets, self.input_size, self.output_size, self.hidden_sizes[0], len(self.hidden_sizes),
                          int(c["max_batch"]), float(c["lr"]), float(c["reward_scale"]), self.init_w, (C.c_float * 9)(*wd))
        h = C.c_void_p()
        _lib.check(self.ctx.lib.ilsx_bnn_create(self.ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def _configure(self, **kw):
        """a new library object with the trainer's settings; parameters, optimiser state and normaliser carry over"""
        p, (m, v, meta), (mu, sd) = self.get_flat_params(), self.get_opt(), self.normalizer._get()
        old = self.h
        self._cfg.update(kw)
        self._create()
        _lib.check(self.ctx.lib.ilsx_bnn_destroy(old))
        self.set_flat_params(p)
        self.set_opt(m, v, meta)
        self.normalizer._set(mu, sd)

    @property
    def num_layers(self):
        return len(self.hidden_sizes) + 1

    def num_params(self):
        n = C.c_size_t()
        _lib.check(self.ctx.lib.ilsx_bnn_num_params(self.h, C.byref(n)))
        return n.value

    def param_shapes(self):
        """named_parameters() order: fc{i}.weight [E, in, out], fc{i}.bias [E, 1, out], ..., last_fc.weight, last_fc.bias"""
        E, sizes = self.num_nets, [self.input_size] + self.hidden_sizes + [2 * self.output_size]
        out = []
        for i in range(len(sizes) - 1):
            out += [(E, sizes[i], sizes[i + 1]), (E, 1, sizes[i + 1])]
        return out

    def get_flat_params(self):
        p = np.empty(self.num_params(), np.float32)
        _lib.check(self.ctx.lib.ilsx_bnn_get_params(self.h, host_ptr(p), p.size))
        return p

    def set_flat_params(self, p):
        p = np.ascontiguousarray(p, np.float32).reshape(-1)
        _lib.check(self.ctx.lib.ilsx_bnn_set_params(self.h, host_ptr(p), p.size))

    def get_params(self):
        flat, out, f = self.get_flat_params(), [], 0
        for s in self.param_shapes():
            n = int(np.prod(s))
            out.append(flat[f:f + n].reshape(s))
            f += n
        return out

    def set_params(self, arrays):
        self.set_flat_params(np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in arrays]))

    def get_opt(self):
        n = self.num_params()
        m, v, meta = np.empty(n, np.float32), np.empty(n, np.float32), _lib.OptMeta()
        _lib.check(self.ctx.lib.ilsx_bnn_get_opt(self.h, host_ptr(m), host_ptr(v), n, C.byref(meta)))
        return m, v, dict(t=meta.t, rng_step=meta.rng_step)

    def set_opt(self, m, v, meta):
        m, v = np.ascontiguousarray(m, np.float32), np.ascontiguousarray(v, np.float32)
        om = _lib.OptMeta(int(meta["t"]), int(meta["rng_step"]), int(meta["t"]))
        _lib.check(self.ctx.lib.ilsx_bnn_set_opt(self.h, host_ptr(m), host_ptr(v), m.size, C.byref(om)))

    def forward(self, inputs, ret_log_var=False):
        """inputs [n, in] (numpy) -> (mean [E, n, D], log-var or var [E, n, D])"""
        x = self.ctx.from_numpy(np.asarray(inputs, np.float32).reshape(-1, self.input_size))
        n = x.shape[0]
        mean, var = self.ctx.empty((self.num_nets, n, self.output_size)), self.ctx.empty((self.num_nets, n, self.output_size))
        _lib.check(self.ctx.lib.ilsx_bnn_predict(self.h, x.ptr, n, mean.ptr, var.ptr, int(bool(ret_log_var))))
        return mean.numpy(), var.numpy()

    __call__ = forward

    def predict(self, inputs, factored=False):
        """networks.py:265-275"""
        mean_fac, var_fac = self.forward(inputs)
        if np.ndim(inputs) == 2 and not factored:
            mean = np.mean(mean_fac, axis=0)
            return mean, np.mean(var_fac, axis=0) + np.mean((mean_fac - mean) ** 2, axis=0)
        return mean_fac, var_fac

    def close(self):
        if self.h is not None and self.ctx.h:
            self.ctx.lib.ilsx_bnn_destroy(self.h)
        self.h = None


class BNNTrainer:
    """BNNTrainer(bnn, lr, fc_weight_decays, num_elites, reward_scale, batch_size, max_epochs, max_epochs_since_update, max_grad_steps,
    holdout_ratio, max_holdout, log_freq, timer, max_t) — bnn_trainer.py:16-69; other keys (net_size, num_nets, ...) are swallowed as
    there."""

    def __init__(self, bnn, lr=1e-3, optimizer_class=None, fc_weight_decays=None, num_elites=None, reward_scale=1.0, batch_size=32,
                 max_epochs=None, max_epochs_since_update=5, max_grad_steps=None, holdout_ratio=0.0, max_holdout=5000, log_freq=100,
                 timer=None, max_t=None, logger=None, **kwargs):
        check_swallowed_kwargs(dict(kwargs, optimizer_class=optimizer_class), type(self).__name__)
        self.bnn = bnn
        num_hidden = bnn.num_layers - 1
        if fc_weight_decays is None:
            fc_weight_decays = default_weight_decays(num_hidden)
        elif isinstance(fc_weight_decays, float):
            fc_weight_decays = [fc_weight_decays] * (num_hidden + 1)
        assert len(fc_weight_decays) == num_hidden + 1
        self.fc_weight_decays = list(fc_weight_decays)
        self.num_elites = min(bnn.num_nets if num_elites is None else num_elites, bnn.num_nets)
        self.reward_scale, self.batch_size = reward_scale, int(batch_size)
        self.max_epochs, self.max_epochs_since_update, self.max_grad_steps = max_epochs, max_epochs_since_update, max_grad_steps
        self.holdout_ratio, self.max_holdout, self.log_freq, self.timer, self.max_t = holdout_ratio, int(max_holdout), log_freq, timer, max_t
        self.logger = logger
        self.eval_statistics = None
        self._model_idx = list(range(self.num_elites))
        bnn._configure(lr=lr, reward_scale=reward_scale, weight_decays=self.fc_weight_decays, max_batch=self.batch_size)
        self.ctx = bnn.ctx

    def _log(self, s):
        (self.logger.log if self.logger is not None else print)(s)

    @property
    def normalizer(self):
        return self.bnn.normalizer

    # ---- the arithmetic entry points (device rows of a replay ring)
    def _mse(self, rb, table, stride, n, add_var=False):
        if n == 0:   # torch.mean over no rows (an empty holdout): NaN, as compute_loss gives in the reference
            return np.full(self.bnn.num_nets, np.nan, np.float32)
        out = np.empty(self.bnn.num_nets, np.float32)
        _lib.check(self.ctx.lib.ilsx_bnn_mse(self.bnn.h, rb.h, table.ptr, int(stride), int(n), int(add_var), host_ptr(out)))
        return out

    def _train_batch(self, rb, table, col, stride, B, want_loss=False):
        out = np.empty(self.bnn.num_nets, np.float32) if want_loss else None
        _lib.check(self.ctx.lib.ilsx_bnn_train_batch(self.bnn.h, rb.h, _off(table.ptr, 4 * col), int(stride), int(B),
                                                      host_ptr(out) if want_loss else None))
        return out

    def train_step(self, batch):
        """bnn_trainer.py:89-219.  batch: a device replay buffer (its rows [0, size) are the dataset, get_all()) or a dict of host arrays."""
        rb, tmp = batch, None
        if not isinstance(batch, SimpleReplayBuffer):
            n = len(batch["rewards"])
            tmp = rb = SimpleReplayBuffer(n, batch["observations"].shape[1], batch["actions"].shape[1], ctx=self.ctx)
            rb.add_rows(batch["observations"], batch["actions"], np.asarray(batch["rewards"]).reshape(n),
                        np.asarray(batch.get("terminals", np.zeros(n))).reshape(n), batch["next_observations"])
        self._epochs_since_update = 0
        self._state = {}
        self._snapshots = {i: (None, 1e10) for i in range(self.bnn.num_nets)}
        E, ctx = self.bnn.num_nets, self.ctx
        N = rb._size
        num_holdout = min(int(N * self.holdout_ratio), self.max_holdout)
        perm = np.random.permutation(N)
        ho_rows, tr_rows = perm[:num_holdout].astype(np.int32), perm[num_holdout:].astype(np.int32)
        n_tr = len(tr_rows)
        self._log(f"BNN | Training ({E}, {n_tr}, {self.bnn.input_size}) | Holdout: ({E}, {num_holdout}, {self.bnn.input_size})")
        d_tr = ctx.from_numpy(tr_rows, np.int32)
        d_ho = ctx.from_numpy(ho_rows if num_holdout else np.zeros(1, np.int32), np.int32)
        _lib.check(ctx.lib.ilsx_bnn_fit_stats(self.bnn.h, rb.h, d_tr.ptr, n_tr))
        idxs = np.random.randint(n_tr, size=[E, n_tr])
        t_start, grad_updates = time.time(), 0
        epoch, epochs_run = 0, 0
        while not self.max_epochs or epoch < self.max_epochs:   # range(max_epochs) if max_epochs else count() (:123)
            table = ctx.from_numpy(tr_rows[idxs], np.int32)   # [E, n_tr] ring slots, uploaded once per epoch
            num_batches = int(np.ceil(n_tr / self.batch_size))
            for b in range(num_batches):
                lo = b * self.batch_size
                self._train_batch(rb, table, lo, n_tr, min(self.batch_size, n_tr - lo))
                grad_updates += 1
            epochs_run += 1
            idxs = self._shuffle_rows(idxs)
            if epoch % self.log_freq == 0:   # the train MSE is only logged (bnn_trainer.py:167-174)
                k = min(self.max_holdout, n_tr)
                ev = ctx.from_numpy(np.ascontiguousarray(tr_rows[idxs[:, :k]]), np.int32)
                self._log(f"BNN | epoch {epoch} | BNN Train MSE: {np.mean(self._mse(rb, ev, k, k))}")
            break_train = False
            if self.holdout_ratio > 1e-8:
                holdout_mse = self._mse(rb, d_ho, 0, num_holdout)
                if epoch % self.log_freq == 0:
                    self._log(f"BNN | epoch {epoch} | BNN Holdout MSE: {np.mean(holdout_mse)}")
                break_train = self._save_best(epoch, holdout_mse)
            t = time.time() - t_start
            if break_train or (self.max_grad_steps and grad_updates > self.max_grad_steps):
                break
            if self.max_t and t > self.max_t:
                self._log(f"BNN | epoch {epoch} | Breaking because of timeout: {t} (max {self.max_t})")
                break
            epoch += 1
        self._set_state()
        final_holdout_mse = self._mse(rb, d_ho, 0, num_holdout)
        ho_idx = np.argsort(final_holdout_mse)
        self._model_idx = ho_idx[: self.num_elites].tolist()
        self._log(f"BNN | Using {self.num_elites}/{E} models: {self._model_idx}")
        final_holdout_mse.sort()
        val_loss = np.mean(final_holdout_mse[: self.num_elites])
        self._log(f"BNN | Holdout loss {final_holdout_mse} | Validation loss: {val_loss}")
        if self.eval_statistics is None:
            self.eval_statistics = OrderedDict()
            self.eval_statistics["BNN Loss"] = val_loss
        if tmp is not None:
            tmp.ctx.sync()
        return dict(epochs=epochs_run, grad_updates=grad_updates, holdout_mse=final_holdout_mse)

    def _shuffle_rows(self, a):   # bnn_trainer.py:239-241
        new_idx = np.argsort(np.random.uniform(size=a.shape), axis=-1)
        return a[np.arange(a.shape[0])[:, None], new_idx]

    def _save_state(self, net_id):
        """bnn_trainer.py:243-247: the reference stores fc.weight.data / fc.bias.data — ALIASES of the live parameters, not copies"""
        self._state[net_id] = "live"

    def _set_state(self):
        """bnn_trainer.py:249-253: loads those aliases, i.e. the live weights into themselves: a no-op.  A member that never improved has
        no entry, where the reference raises KeyError too."""
        for net_id in range(self.bnn.num_nets):
            self._state[net_id]

    def _save_best(self, epoch, holdout_mse):   # bnn_trainer.py:255-272
        upd = False
        for net_id in range(len(holdout_mse)):
            cur = holdout_mse[net_id]
            _, best = self._snapshots[net_id]
            imp = (best - cur) / best
            if imp > 0.01:
                self._snapshots[net_id] = (epoch, cur)
                self._save_state(net_id)
                upd = True
        self._epochs_since_update = 0 if upd else self._epochs_since_update + 1
        return self._epochs_since_update > self.max_epochs_since_update

    def get_random_model_index(self, batch_size):   # :274-275
        return np.random.choice(self._model_idx, size=batch_size)

    def predict(self, inputs, factored=False):
        return self.bnn.predict(inputs, factored)

    def get_eval_statistics(self):
        return self.eval_statistics

    def end_epoch(self):
        self.eval_statistics = None

    def get_snapshot(self):
        m, v, meta = self.bnn.get_opt()
        mu, sd = self.bnn.normalizer._get()
        return dict(bnn=self.bnn.get_flat_params(), bnn_optimizer=dict(exp_avg=m, exp_avg_sq=v, **meta), bnn_normalizer=dict(mean=mu, std=sd),
                    bnn_elites=list(self._model_idx))

    def load_snapshot(self, snap):
        self.bnn.set_flat_params(snap["bnn"])
        o = snap["bnn_optimizer"]
        self.bnn.set_opt(o["exp_avg"], o["exp_avg_sq"], o)
        self.bnn.normalizer._set(snap["bnn_normalizer"]["mean"], snap["bnn_normalizer"]["std"])
        self._model_idx = [int(i) for i in snap["bnn_elites"]]


def terminal_kind(is_terminal):
    """the ILSX_TERM_* kind of an ilswiss_amd.envs.terminals predicate (get_terminal_func(env_name))"""
    owner = getattr(is_terminal, "__self__", None)
    kind = getattr(owner, "kind", None)
    if kind is None:
        raise NotImplementedError(f"MBPO: the model rollout labels terminals on the device; {is_terminal!r} is not a device predicate")
    return int(kind)


class FakeEnv:
    """fake_env.py:9-75.  step() takes host arrays and draws the sample noise with np.random.normal over [E, n, D] and the members with
    gen_model_idx, in the reference's order; MBPO's rollout uses the fused device step (ilsx_mbpo_model_step) instead."""

    def __init__(self, model, is_terminal, gen_model_idx):
        self.model, self.is_terminal, self.gen_model_idx = model, is_terminal, gen_model_idx
        self.kind = terminal_kind(is_terminal)

    def step(self, obs, act, deterministic=False):
        bnn = self.model.bnn if hasattr(self.model, "bnn") else self.model
        obs, act = np.asarray(obs, np.float32), np.asarray(act, np.float32)
        single = obs.ndim == 1
        if single:
            obs, act = obs[None], act[None]
        n, E, D = obs.shape[0], bnn.num_nets, bnn.output_size
        noise = None if deterministic else np.random.normal(size=(E, n, D))
        midx = np.asarray(self.gen_model_idx(n), np.int32)
        ctx = bnn.ctx
        eps = None if noise is None else ctx.from_numpy(noise[midx, np.arange(n)], np.float32)
        ring = SimpleReplayBuffer(max(n, 1), obs.shape[1], act.shape[1], ctx=ctx)
        d_obs, d_act, d_mid = ctx.from_numpy(obs), ctx.from_numpy(act), ctx.from_numpy(midx, np.int32)
        nxt, ns = ctx.empty(obs.shape), C.c_int()
        _lib.check(ctx.lib.ilsx_mbpo_model_step(bnn.h, None, ring.h, self.kind, d_obs.ptr, d_act.ptr, n, None, 0, int(bool(deterministic)),
                                                eps.ptr if eps is not None else None, d_mid.ptr, None, None, nxt.ptr, C.byref(ns)))
        rows = ring.get_all(keys=("rewards", "terminals", "next_observations"))
        next_obs, rewards, terminals = rows["next_observations"], rows["rewards"], rows["terminals"].astype(bool)
        if single:
            return next_obs[0], rewards[0], terminals[0], {}
        return next_obs, rewards, terminals, {}

    def close(self):
        pass


class _MBPOTrainer:
    """the trainer face DeviceRLAlgorithm sees: SAC's context and statistics plus the model's (mbpo.py:164-168)"""

    def __init__(self, mbpo):
        self._m = mbpo
        self.ctx = mbpo.algo.ctx

    def get_eval_statistics(self):
        st = OrderedDict()
        for s in (self._m.model.get_eval_statistics(), self._m.algo.get_eval_statistics(), self._m._rollout_stat):
            if s:
                st.update(s)
        return st

    def end_epoch(self):
        self._m.model.end_epoch()
        self._m.algo.end_epoch()

    def get_snapshot(self):
        return dict(self._m.algo.get_snapshot(), **self._m.model.get_snapshot())

    def load_snapshot(self, snap):
        self._m.algo.load_snapshot(snap)
        self._m.model.load_snapshot(snap)


class MBPO(DeviceRLAlgorithm):
    """MBPO(env, model: BNNTrainer, algo: SoftActorCritic, is_terminal, ...) — mbpo.py:23-68; the rest of the keys are
    DeviceRLAlgorithm's (training_env, eval_env, exploration_policy, batch_size, ...)."""

    EVAL_BETWEEN_EPOCHS = "MBPO's epoch loop does not overlap the evaluation with the next epoch"

    def __init__(self, env, model, algo, is_terminal, model_replay_buffer=None, model_replay_buffer_size=10000, deterministic=False,
                 model_train_freq=250, model_retrain_epochs=1, rollout_batch_size=int(1e5), real_ratio=0.1, rollout_schedule=None,
                 max_model_t=None, target_update_interval=1, **kwargs):
        if int(target_update_interval) != 1:
            raise NotImplementedError("MBPO(target_update_interval != 1): libilsx's SAC updates its targets every step")
        if getattr(kwargs.get("training_env"), "norm_obs", False):
            raise NotImplementedError("MBPO with a norm_obs training env: the device termination predicates and the model rollouts read "
                                      "observation columns as raw quantities")
        self.model, self.algo, self.is_terminal = model, algo, is_terminal
        self._rollout_stat = OrderedDict()
        super().__init__(trainer=_MBPOTrainer(self), env=env, **kwargs)
        self.term_kind = terminal_kind(is_terminal)
        self.fake_env = FakeEnv(model, is_terminal, model.get_random_model_index)
        if model_replay_buffer is None:
            assert self.max_path_length < model_replay_buffer_size
            model_replay_buffer = EnvReplayBuffer(model_replay_buffer_size, env, random_seed=int(np.random.randint(10000)), ctx=algo.ctx)
        self.model_replay_buffer = model_replay_buffer
        self.deterministic, self.model_train_freq, self.model_retrain_epochs = bool(deterministic), int(model_train_freq), int(model_retrain_epochs)
        self.rollout_batch_size, self.real_ratio = int(rollout_batch_size), float(real_ratio)
        self.rollout_schedule, self.max_model_t = rollout_schedule, max_model_t
        self.rollout_length = 1
        if max_model_t is not None:
            model.max_t = max_model_t
        self._staging = None
        self.logger.log(f"MBPO | Target entropy: {algo.target_entropy}")

    # ---- mbpo.py:194-205
    def _set_rollout_length(self, epoch):
        self.rollout_length = rollout_length_at(self.rollout_schedule, epoch)
        self.logger.log(f"Model Rollout | Epoch {epoch} | Length: {self.rollout_length}")

    # ---- mbpo.py:207-232
    def _extend_model_replay_buffer(self):
        new_pool_size = model_pool_size(self.model_retrain_epochs, self.rollout_length, self.rollout_batch_size, self.max_path_length,
                                        self.model_train_freq)
        old = self.model_replay_buffer
        if old._max_replay_buffer_size < new_pool_size:
            self.logger.log(f"Extend model replay buffer | {old._max_replay_buffer_size:.2e} -> {new_pool_size:.2e}")
            new = EnvReplayBuffer(new_pool_size, self.env, int(np.random.randint(10000)), ctx=self.algo.ctx)
            if old._size > 0:
                new.add_path(old.get_all(keys=("observations", "actions", "rewards", "terminals", "next_observations")))
            self.model_replay_buffer = new
        return True

    # ---- mbpo.py:234-272, every step on the device
    def _rollout_model(self, deterministic=False):
        ctx, lib, n = self.algo.ctx, self.algo.ctx.lib, self.rollout_batch_size
        o, a = self.training_env.obs_dim, self.training_env.act_dim
        self.logger.log(f"Model Rollout | Rollout length: {self.rollout_length} | Batch size: {n}")
        cur, nxt = ctx.empty((n, o)), ctx.empty((n, o))
        act, rew, done, nob = ctx.empty((n, a)), ctx.empty((n,)), ctx.empty((n,)), ctx.empty((n, o))
        _lib.check(lib.ilsx_replay_sample(self.replay_buffer.h, n, None, cur.ptr, act.ptr, rew.ptr, done.ptr, nob.ptr, None))
        elites = np.ascontiguousarray(self.model._model_idx, np.int32)
        steps, rows = [], n
        for i in range(self.rollout_length):
            ns = C.c_int()
            _lib.check(lib.ilsx_mbpo_model_step(self.model.bnn.h, self.algo.policy.h, self.model_replay_buffer.h, self.term_kind, cur.ptr,
                                                None, rows, host_ptr(elites), len(elites), int(deterministic), None, None,
                                                None, None, nxt.ptr, C.byref(ns)))
            steps.append(rows)
            if ns.value == 0:
                self.logger.log(f"Model Rollout | Breaking early at {i}: all episodes terminate")
                break
            rows = ns.value
            cur, nxt = nxt, cur
        mean_len = float(np.sum(steps)) / n
        self.logger.log(f"Model Rollout | Added: {np.sum(steps):.1e} | Model pool: {self.model_replay_buffer._size:.1e} | Mean length: {mean_len}")
        return OrderedDict(mean_rollout_length=mean_len)

    def _train_model(self):   # mbpo.py:185-188
        assert self.replay_buffer._size >= self.min_steps_before_training
        self.model.train_step(self.replay_buffer)

    # ---- mbpo.py:170-183 + 190-192: two device samples into one staging batch, then one SAC step
    def get_batch_sizes(self):
        return batch_split(self.batch_size, self.real_ratio, self.model_replay_buffer._size)

    def _do_training(self):
        ctx, lib, B = self.algo.ctx, self.algo.ctx.lib, self.batch_size
        o, a = self.training_env.obs_dim, self.training_env.act_dim
        if self._staging is None:
            self._staging = [ctx.empty((B, o)), ctx.empty((B, a)), ctx.empty((B,)), ctx.empty((B,)), ctx.empty((B, o))]
        st = self._staging
        for _ in range(self.num_train_steps_per_train_call):
            real, model = self.get_batch_sizes()
            for rb, lo, cnt in ((self.replay_buffer, 0, real), (self.model_replay_buffer, real, model)):
                if cnt > 0:
                    ptrs = [_off(x.ptr, 4 * lo * (x.shape[1] if len(x.shape) > 1 else 1)) for x in st]
                    _lib.check(lib.ilsx_replay_sample(rb.h, cnt, None, *ptrs, None))
            self.algo._call("train_step", *[x.ptr for x in st], B, None, None)

    def _train_call(self):
        self._do_training()

    # ---- mbpo.py:70-162: the model-training block and the step count that ends an epoch; the rest is the shared loop's
    def train(self, start_epoch=0):
        loop = DeviceRLAlgorithmGroup([self])
        self.logger.log(f"MBPO | Presampling for {self.min_steps_before_training} steps")
        for epoch in range(start_epoch, self.num_epochs):   # MBPO.start_training: range(start_epoch, num_epochs)
            loop.begin_epoch()
            start_env_steps, last_block = self._n_env_steps_total, None
            while True:
                t0 = time.perf_counter()
                if self._can_train():
                    cur = self._n_env_steps_total - start_env_steps - self.env_num
                    if cur >= self.num_env_steps_per_epoch:
                        break
                    # the reference trains the model when cur % model_train_freq == 0 with one env; with env_num envs the count moves
                    # env_num at a time, so the model trains when it enters a new multiple of model_train_freq
                    block = cur // self.model_train_freq if cur >= 0 else None
                    if block is not None and block != last_block and self.real_ratio < 1.0:
                        last_block = block
                        loop.sync()
                        self._train_model()
                        self._set_rollout_length(epoch)
                        self._extend_model_replay_buffer()
                        self._rollout_stat = self._rollout_model(self.deterministic)
                        loop.sync()
                        loop.t_train += time.perf_counter() - t0
                        t0 = time.perf_counter()
                else:
                    start_env_steps = self._n_env_steps_total
                loop.sample_then_train(t0)
            loop.end_epoch(epoch)


def rollout_length_at(schedule, epoch):
    """mbpo.py:194-205"""
    min_epoch, max_epoch, min_length, max_length = schedule
    if epoch < min_epoch:
        length = min_length
    else:
        dx = min((epoch - min_epoch) / (max_epoch - min_epoch), 1)
        length = dx * (max_length - min_length) + min_length
    return int(length)


def model_pool_size(model_retrain_epochs, rollout_length, rollout_batch_size, max_path_length, model_train_freq):
    """mbpo.py:207-212"""
    rollout_per_epoch = rollout_batch_size * max_path_length / model_train_freq
    return model_retrain_epochs * int(rollout_length * rollout_per_epoch)


def batch_split(batch_size, real_ratio, model_size):
    """mbpo.py:170-173: (real rows, model rows) of one SAC batch"""
    r = real_ratio if model_size > 0 else 1.0
    real = int(batch_size * r)
    return real, batch_size - real
