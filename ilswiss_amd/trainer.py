"""The trainers' shared base: the reference's abstract `Trainer` (rlkit/core/trainer.py:4-28) and `DeviceTrainer`, the part every libilsx
trainer repeats — create the library object, call it with or without a statistics block, keep staged host batches alive, read and write
flat parameters, snapshot parameters and Adam state.  A trainer over `ilsx_<ABI>_*` is a subclass with five tables (ABI, Stats, WHICH,
SNAPSHOT_KEYS, OPT), a constructor that fills the cfg struct, `_fill_stats` and `networks`.
"""
import abc
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .device import host_ptr
from .snapshot import get_opt, set_opt


def check_swallowed_kwargs(kwargs, who):
    """The reference's trainers take **kwargs and ignore what they do not know; two of the keys they DO read select something libilsx
    does not have — another optimiser than Adam (`optimizer_class`, e.g. sac_alpha.py:35) or another critic criterion than MSE
    (`qf_criterion`, td3.py:36): those fail loudly, everything else is swallowed as in the reference."""
    oc = kwargs.get("optimizer_class")
    if oc is not None and getattr(oc, "__name__", oc) != "Adam":
        raise NotImplementedError(f"{who}(optimizer_class={getattr(oc, '__name__', oc)}): libilsx implements torch.optim.Adam")
    qc = kwargs.get("qf_criterion")
    if qc is not None:   # an nn.MSELoss instance, the class itself, or its name; anything else (L1Loss, "huber", ...) is refused, not trained as MSE
        name = qc if isinstance(qc, str) else (getattr(qc, "__name__", None) or type(qc).__name__)
        if name.lower() not in ("mseloss", "mse"):
            raise NotImplementedError(f"{who}(qf_criterion={qc!r}): libilsx implements the MSE criterion")


def create_stats_ordered_dict(name, data):  # rlkit/core/eval_util.py:create_stats_ordered_dict (Mean/Std/Max/Min)
    data = np.asarray(data, dtype=np.float64)
    if data.size == 1:
        return OrderedDict({name: float(data.ravel()[0])})
    return OrderedDict([(name + " Mean", np.mean(data)), (name + " Std", np.std(data)),
                        (name + " Max", np.max(data)), (name + " Min", np.min(data))])


def stat_block(st, name, vals):
    """The library's {Mean, Std, Max, Min} value list of one statistic (include/ilsx.h) under create_stats_ordered_dict's keys."""
    for k, v in zip(("Mean", "Std", "Max", "Min"), vals):
        st[f"{name} {k}"] = float(v)


class Trainer(metaclass=abc.ABCMeta):  # rlkit/core/trainer.py:4-28
    @abc.abstractmethod
    def train_step(self, batch):
        pass

    def get_eval_statistics(self):
        return None

    def get_snapshot(self):
        return {}

    def end_epoch(self):
        pass

    @property
    @abc.abstractmethod
    def networks(self):
        pass


class DeviceTrainer(Trainer):
    """A trainer whose step is the library object `ilsx_<ABI>_*`.  Subclasses set `self.ctx` and their networks, then call `_create`."""
    ABI = None            # symbol infix: ilsx_<ABI>_create / _train_step / _train_from_replay / _get_params / _set_params / _get_opt / _set_opt
    Stats = C.c_float     # what the library's step calls write through their last argument: a ctypes struct, or one float
    WHICH = {}            # parameter block name (aliases included) -> the library's index
    SNAPSHOT_KEYS = ()    # the parameter blocks get_snapshot emits, in order
    OPT = ()              # (key, which): blocks with an Adam state, saved as key + "_optimizer"
    PARAMS_TAIL = ()      # arguments of ilsx_<ABI>_{get,set}_params behind (which, pointer, count)

    def _fn(self, name):
        return getattr(self.ctx.lib, f"ilsx_{self.ABI}_{name}")

    def _create(self, cfg, *handles):
        self.h = C.c_void_p()
        _lib.check(self._fn("create")(self.ctx.h, C.byref(cfg), *handles, C.byref(self.h)))
        self.eval_statistics = None
        self._stats = self.Stats()

    def close(self):
        """ilsx_<ABI>_destroy, once: the object's device memory goes back to the context and the networks it adopted get storage of their
        own again, so they stay usable.  Nothing to do when the context is closed already: it has freed the memory with its own."""
        if self.h and self.ctx.h:
            _lib.check(self._fn("destroy")(self.h))
        self.h = None

    def _call(self, name, *args, keep=()):
        """ilsx_<ABI>_<name>(handle, *args, statistics): the statistics of the first step of the call are asked for and recorded when none
        are held since the last end_epoch.  `keep`: the staged device copies of host arrays among `args`; the call is asynchronous and only
        reading the statistics waits for it, so without them it is waited for here, before `keep` can be freed."""
        want = self.eval_statistics is None
        _lib.check(self._fn(name)(self.h, *args, C.byref(self._stats) if want else None))
        if want:
            self._fill_stats()
        elif keep:
            self.ctx.sync()

    @abc.abstractmethod
    def _fill_stats(self):
        """self._stats -> self.eval_statistics"""

    # ---- Trainer API
    def train_from_replay(self, replay_buffer, n_steps, batch_size):
        """TorchRLAlgorithm._do_training (torch_rl_algorithm.py:28-34) with on-device sampling."""
        self._call("train_from_replay", replay_buffer.h, int(n_steps), int(batch_size))

    def get_eval_statistics(self):
        return self.eval_statistics

    def end_epoch(self):
        self.eval_statistics = None

    def to(self, device=None):   # the networks already live on the library's device
        return self

    def set_num_steps_total(self, num):
        pass

    # ---- parameter / optimiser access (snapshots, parity tests)
    def _num_params(self, which):
        pol = (self.WHICH["policy"], self.WHICH.get("target_policy"))
        return (self.policy if which in pol else self.qf1).num_params

    def _read(self, what, name):
        w = self.WHICH[name]
        out = np.empty(self._num_params(w), np.float32)
        _lib.check(self._fn(what)(self.h, w, host_ptr(out), out.size, *self.PARAMS_TAIL))
        return out

    def get_flat_params(self, name):
        return self._read("get_params", name)

    def set_flat_params(self, name, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        _lib.check(self._fn("set_params")(self.h, self.WHICH[name], host_ptr(flat), flat.size, *self.PARAMS_TAIL))

    def _get_opt(self, n, which=None):
        return get_opt(self.ctx.lib, self.ABI, self.h, n, which)

    def _set_opt(self, state, which=None):
        set_opt(self.ctx.lib, self.ABI, self.h, state, which)

    def get_snapshot(self):   # the reference's get_snapshot keys as plain arrays, plus each optimiser's Adam state
        snap = {k: self.get_flat_params(k) for k in self.SNAPSHOT_KEYS}
        for k, w in self.OPT:
            snap[k + "_optimizer"] = self._get_opt(snap[k].size, w)
        return snap

    def load_snapshot(self, snap):
        for k in self.SNAPSHOT_KEYS:
            self.set_flat_params(k, snap[k])
        for k, w in self.OPT:
            if k + "_optimizer" in snap:
                self._set_opt(snap[k + "_optimizer"], w)
