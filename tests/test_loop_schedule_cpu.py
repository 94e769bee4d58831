"""The host schedule of the epoch loops (off-policy group, on-policy, MBPO) on stub runs: no device, no library.

Every stub appends to one event list (`trace`); evaluations that run on a worker thread append to a list of their own (`side`), so the
main trace is deterministic.  The expected traces and rows below were produced by this module on the commit BEFORE the single off-policy
loop became a group of one, where cases (a)-(f) passed as written except that (d) showed the first run's context waited on twice at every
group sync (`sync:c0 sync:c1 sync:c2 sync:c0`): the one difference `_once_per_context` removes.  Case (g) is the MBPO eval_async fallback.

Events: `step<k>:rand|pi[+kwarg]`, `stepend<k>`, `sync:<ctx>`, `train<k>(ring size,n,B)`, `eval<k>`, `stats<k>` (rollout_stats), `snap<k>`,
`end<k>` (end_epoch), `row<k>=<epoch>` (the row is written), `rms<k>` (statistics sync), `freeze<k>`, `extra<k>`, `rollout<k>(horizon)`,
and MBPO's `model` / `length` / `extend` / `modelrollout` / `sac`.  `x*N` is x repeated N times."""
import csv
import os
import pickle
import threading
from collections import OrderedDict
from types import SimpleNamespace

from ilswiss_amd.algorithm import DeviceRLAlgorithm, DeviceRLAlgorithmGroup
from ilswiss_amd.mbpo import MBPO
from ilswiss_amd.samplers import DeviceEvalSampler


class Ctx:
    def __init__(self, trace, name):
        self.trace, self.name, self.stream = trace, name, name

    def sync(self):
        self.trace.append(f"sync:{self.name}")


class Ring:
    size = 0

    def num_steps_can_sample(self):
        return self.size


class Trainer:
    on_policy = False

    def __init__(self, trace, k, ctx):
        self.trace, self.k, self.ctx, self.calls = trace, k, ctx, 0

    def train_from_replay(self, rb, n, B):
        self.trace.append(f"train{self.k}({rb.size},{n},{B})")
        self.calls += 1

    def get_eval_statistics(self):
        return OrderedDict(Loss=float(self.calls))

    def end_epoch(self):
        self.trace.append(f"end{self.k}")

    def get_snapshot(self):
        self.trace.append(f"snap{self.k}")
        return dict(calls=self.calls)


class OnPolicyTrainer(Trainer):
    on_policy = True

    def train_from_rollout(self, env, horizon, max_path_length, bootstrap=True):
        self.trace.append(f"rollout{self.k}({horizon})")
        env.since += horizon
        self.calls += 1
        return horizon * len(env)


class Env:
    """the ring fills as the env steps, from `fills_after` env steps on (insert_at_episode_end: when ITS first episode ends)"""

    def __init__(self, trace, k, fills_after=0, norm_obs=False):
        self.trace, self.k, self.fills_after, self.norm_obs, self.total, self.since = trace, k, fills_after, norm_obs, 0, 0

    def __len__(self):
        return 4

    def rollout_step(self, policy, rb, max_path_length, random_actions=False, no_terminal=False, label_policy=None, **kw):
        self.trace.append(f"step{self.k}:{'rand' if random_actions else 'pi'}" + "".join(f"+{x}" for x in sorted(kw)))
        self.total, self.since = self.total + len(self), self.since + 1
        if self.total >= self.fills_after:
            rb.size = self.total

    def rollout_stats(self, reset=True):
        self.trace.append(f"stats{self.k}")
        out = (self.since, 1.5 * self.since)
        if reset:
            self.since = 0
        return out


class EnvWithEnd(Env):
    def rollout_step_end(self):
        self.trace.append(f"stepend{self.k}")


class EvalEnv:
    def __init__(self, trace, k):
        self.trace, self.k = trace, k

    def sync_obs_rms(self):
        self.trace.append(f"rms{self.k}")


class Sampler(DeviceEvalSampler):
    """value(): what the evaluated policy is worth now; on a worker thread the event goes to `side` with the main trace's length then"""

    def __init__(self, trace, side, k, value):
        super().__init__(None, None, 8, 5)
        self.trace, self.side, self.k, self.value = trace, side, k, value

    def obtain_statistics(self, stat_prefix="Test"):
        if threading.current_thread() is threading.main_thread():
            self.trace.append(f"eval{self.k}")
        else:
            self.side.append((f"eval{self.k}", len(self.trace)))
        v = float(self.value())
        return OrderedDict([("Test Returns Mean", v), ("AverageReturn", v)])


class Frozen:
    def __init__(self, trace, k):
        self.trace, self.k, self.p = trace, k, None

    def set_flat_params(self, p):
        self.trace.append(f"freeze{self.k}")
        self.p = p


SCHEDULE = dict(num_epochs=1, num_steps_per_epoch=40, num_steps_between_train_calls=12, num_train_steps_per_train_call=3, batch_size=8,
                max_path_length=5, min_steps_before_training=8, freq_saving=1, save_best=True)


def make_run(tmp_path, trace, side, k=0, *, env_cls=Env, trainer_cls=Trainer, cls=DeviceRLAlgorithm, use_async=False, fills_after=0,
             norm_obs=False, **kw):
    ctx = Ctx(trace, f"c{k}")
    trainer, env = trainer_cls(trace, k, ctx), env_cls(trace, k, fills_after, norm_obs)
    sampler = Sampler(trace, side, k, lambda: trainer.calls)
    alg = cls.__new__(cls)
    DeviceRLAlgorithm.__init__(alg, trainer, None, env, EvalEnv(trace, k), object(), replay_buffer=None if trainer.on_policy else Ring(),
                               eval_sampler=sampler, log_dir=str(tmp_path / f"run{k}"), **dict(SCHEDULE, **kw))
    if use_async:
        frozen = Frozen(trace, k)
        alg.eval_async = dict(live=SimpleNamespace(get_flat_params=lambda: trainer.calls), frozen=frozen,
                              sampler=Sampler(trace, side, k, lambda: frozen.p))
    extra, dump = alg.get_extra_data_to_save, alg.logger.dump_tabular

    def get_extra(epoch):
        trace.append(f"extra{k}")
        return extra(epoch)

    def dump_tabular():
        trace.append(f"row{k}={alg.logger.row['Epoch']}")
        dump()
    alg.get_extra_data_to_save, alg.logger.dump_tabular = get_extra, dump_tabular
    return alg


def fold(trace):
    out = []
    for ev in trace:
        if out and out[-1][0] == ev:
            out[-1][1] += 1
        else:
            out.append([ev, 1])
    return " ".join(ev if n == 1 else f"{ev}*{n}" for ev, n in out)


def rows(alg):
    with open(os.path.join(alg.logger.log_dir, "progress.csv"), newline="") as f:
        return [" ".join(f"{k}={v}" for k, v in r.items() if "Time" not in k) for r in csv.DictReader(f)]


def saved(alg, name="params.pkl"):
    with open(os.path.join(alg.logger.log_dir, name), "rb") as f:
        return pickle.load(f)


COLS = "Number of train calls total={} Number of gradient steps total={} Number of env steps total={} Number of rollouts total={} Epoch={}"


def row(loss, test, expl, n_paths, calls, env_steps, rollouts, epoch):
    return (f"Loss={loss} Test Returns Mean={test} Exploration Returns Mean={expl} Exploration Num Paths={n_paths} AverageReturn={test} " +
            COLS.format(calls, 3 * calls, env_steps, rollouts, epoch))


# ---- (a), (b): one blocking run.  The first two vec steps act at random (ring below min_steps_before_training = 8), the rest do not; the train
# trigger comes every 12 env steps = 3 vec steps; freq_saving=1 and a new best in epoch 0 and 1: two snapshots per row.
SINGLE = ("stats0 step0:rand*2 step0:pi sync:c0 train0(12,3,8) sync:c0 step0:pi*3 sync:c0 train0(24,3,8) sync:c0 step0:pi*3 sync:c0 "
          "train0(36,3,8) sync:c0 step0:pi sync:c0 eval0 stats0 row0=0 snap0*2 extra0 end0 "
          "stats0 step0:pi*2 sync:c0 train0(48,3,8) sync:c0 step0:pi*3 sync:c0 train0(60,3,8) sync:c0 step0:pi*3 sync:c0 train0(72,3,8) "
          "sync:c0 step0:pi*2 sync:c0 eval0 stats0 row0=1 snap0*2 extra0 end0")
SINGLE_ROWS = [row(3.0, 3.0, 1.5, 10.0, 3, 40, 10, 0), row(6.0, 6.0, 1.5, 10.0, 6, 80, 20, 1)]


def test_single_blocking_run(tmp_path):
    trace = []
    alg = make_run(tmp_path, trace, None)
    alg.train()
    assert fold(trace) == SINGLE
    assert rows(alg) == SINGLE_ROWS
    assert saved(alg) == dict(epoch=1, statistics=saved(alg)["statistics"], calls=6) and saved(alg, "best.pkl")["calls"] == 6
    assert saved(alg, "extra_data.pkl")["best_statistic_so_far"] == 6.0


def test_single_run_takes_plain_steps_on_an_env_that_offers_a_split_step(tmp_path):
    trace = []
    alg = make_run(tmp_path, trace, None, env_cls=EnvWithEnd)
    alg.train()
    assert fold(trace) == SINGLE and rows(alg) == SINGLE_ROWS


def test_blocking_run_without_saving_takes_no_snapshot(tmp_path):
    """freq_saving=0, no save_epoch, save_best off: nothing is downloaded for an epoch's row"""
    trace = []
    alg = make_run(tmp_path, trace, None, freq_saving=0, save_best=False)
    alg.train()
    assert "snap0" not in trace and fold(trace) == SINGLE.replace(" snap0*2", "") and rows(alg) == SINGLE_ROWS


# ---- (c): one run with eval_async.  End of epoch e: join (row e-1 is written), statistics sync, freeze, row inputs (stats), snapshot, extra,
# submit; the last row is written after the loop.
ASYNC = ("stats0 step0:rand*2 step0:pi sync:c0 train0(12,3,8) sync:c0 step0:pi*3 sync:c0 train0(24,3,8) sync:c0 step0:pi*3 sync:c0 "
         "train0(36,3,8) sync:c0 step0:pi sync:c0 rms0 freeze0 stats0 snap0 extra0 end0 "
         "stats0 step0:pi*2 sync:c0 train0(48,3,8) sync:c0 step0:pi*3 sync:c0 train0(60,3,8) sync:c0 step0:pi*3 sync:c0 train0(72,3,8) "
         "sync:c0 step0:pi*2 sync:c0 row0=0 rms0 freeze0 stats0 snap0 extra0 end0 row0=1")


def check_submitted_after(trace, side, k, epochs=2):
    """every evaluation job started after its epoch's extra data was taken (it was submitted last) and before the next epoch's freeze"""
    jobs = [n for name, n in side if name == f"eval{k}"]
    assert len(jobs) == epochs
    for e, n in enumerate(jobs):
        assert trace[:n].count(f"extra{k}") == e + 1 and trace[:n].count(f"freeze{k}") == e + 1, (e, n)


def test_single_run_with_eval_async(tmp_path):
    trace, side = [], []
    alg = make_run(tmp_path, trace, side, use_async=True, norm_obs=True)
    alg.train()
    assert fold(trace) == ASYNC
    check_submitted_after(trace, side, 0)
    assert rows(alg) == SINGLE_ROWS                      # the row of epoch e carries the value frozen at the end of epoch e ...
    assert saved(alg)["calls"] == 6 and saved(alg)["epoch"] == 1      # ... and the snapshot taken then
    assert saved(alg, "extra_data.pkl")["best_statistic_so_far"] == 6.0


# ---- (d): three runs in lock-step whose rings fill after 0, 20 and 8 env steps.  Run 1 cannot train at the first trigger (its ring is empty), its
# gate stays open, and it trains alone one vec step after its ring fills; from then on its trigger is its own.  The trace is the parent's.
GROUP_SYNC = "sync:c0 sync:c1 sync:c2 sync:c0"
GROUP_STEPS = "step0:{0}+begin_only step1:{1}+begin_only step2:{2}+begin_only stepend0 stepend1 stepend2"


def _once_per_context(trace):
    """the one permitted difference: a group sync used to wait on the first run's context a second time"""
    return trace.replace(GROUP_SYNC, "sync:c0 sync:c1 sync:c2")


def group_case(tmp_path, use_async):
    trace, side = [], []
    runs = [make_run(tmp_path, trace, side, k, env_cls=EnvWithEnd, fills_after=f, use_async=use_async, norm_obs=True)
            for k, f in enumerate((0, 20, 8))]
    grp = DeviceRLAlgorithmGroup(runs)
    assert grp._lockstep_args is None
    grp.train()
    return runs, trace, side


def _steps(kinds, n=1):
    return " ".join([GROUP_STEPS.format(*kinds)] * n)


GROUP_EPOCH0 = " ".join([
    "stats0 stats1 stats2", _steps(("rand", "rand", "rand"), 2), _steps(("pi", "rand", "pi")),
    GROUP_SYNC, "train0(12,3,8) train2(12,3,8)", GROUP_SYNC,
    _steps(("pi", "rand", "pi")), GROUP_SYNC,       # run 1 is due and cannot train
    _steps(("pi", "rand", "pi")), GROUP_SYNC, "train1(20,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC, "train0(24,3,8) train2(24,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi"), 2), GROUP_SYNC, "train1(32,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC, "train0(36,3,8) train2(36,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC])
GROUP_EPOCH1 = " ".join([
    "stats0 stats1 stats2", _steps(("pi", "pi", "pi")), GROUP_SYNC, "train1(44,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC, "train0(48,3,8) train2(48,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi"), 2), GROUP_SYNC, "train1(56,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC, "train0(60,3,8) train2(60,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi"), 2), GROUP_SYNC, "train1(68,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi")), GROUP_SYNC, "train0(72,3,8) train2(72,3,8)", GROUP_SYNC,
    _steps(("pi", "pi", "pi"), 2), GROUP_SYNC, "train1(80,3,8)", GROUP_SYNC, GROUP_SYNC])
GROUP_ROWS = {0: SINGLE_ROWS, 2: SINGLE_ROWS, 1: [row(2.0, 2.0, 1.5, 10.0, 2, 40, 10, 0), row(6.0, 6.0, 1.5, 10.0, 6, 80, 20, 1)]}


def test_three_grouped_runs_blocking(tmp_path):
    runs, trace, side = group_case(tmp_path, use_async=False)
    ends = " ".join(f"stats{k} row{k}={{0}} snap{k} snap{k} extra{k} end{k}" for k in range(3))
    want = " ".join([GROUP_EPOCH0, "rms0 rms1 rms2", ends.format(0), GROUP_EPOCH1, "rms0 rms1 rms2", ends.format(1)])
    assert " ".join(trace) == _once_per_context(want)
    assert sorted(side_ev for side_ev, _ in side) == ["eval0", "eval0", "eval1", "eval1", "eval2", "eval2"]   # one thread per run
    for k, r in enumerate(runs):
        assert rows(r) == GROUP_ROWS[k], k


def test_three_grouped_runs_with_eval_async(tmp_path):
    runs, trace, side = group_case(tmp_path, use_async=True)
    take = " ".join(f"freeze{k} stats{k} snap{k} extra{k} end{k}" for k in range(3))
    want = " ".join([GROUP_EPOCH0, "rms0 rms1 rms2", take, GROUP_EPOCH1, "row0=0 row1=0 row2=0", "rms0 rms1 rms2", take,
                     "row0=1 row1=1 row2=1"])
    assert " ".join(trace) == _once_per_context(want)
    for k, r in enumerate(runs):
        check_submitted_after(trace, side, k)
        assert rows(r) == GROUP_ROWS[k], k
        assert saved(r)["calls"] == 6 and saved(r)["epoch"] == 1


# ---- (e): the on-policy loop: horizon = 12 // 4 = 3 vec steps per rollout, four rollouts reach the epoch's 40 steps
ON_POLICY = ("stats0 rollout0(3)*4 sync:c0 rms0 eval0 stats0 row0=0 snap0*2 extra0 end0 "
             "stats0 rollout0(3)*4 sync:c0 rms0 eval0 stats0 row0=1 snap0*2 extra0 end0")
ON_POLICY_ROWS = [row(4.0, 4.0, 1.5, 12.0, 4, 48, 12, 0), row(8.0, 8.0, 1.5, 12.0, 8, 96, 24, 1)]


def test_on_policy_run(tmp_path):
    trace = []
    alg = make_run(tmp_path, trace, None, trainer_cls=OnPolicyTrainer, norm_obs=True)
    alg.train()
    assert fold(trace) == ON_POLICY and rows(alg) == ON_POLICY_ROWS


# ---- (f): MBPO.  real_ratio < 1: the model block (train the model, set the rollout length, extend the pool, roll the model out) runs when the
# epoch's step count enters a new multiple of model_train_freq = 16; an epoch ends by MBPO's own step-count rule; range(num_epochs) epochs.
class StubMBPO(MBPO):
    def _train_model(self):
        self.trainer.trace.append("model")

    def _set_rollout_length(self, epoch):
        self.trainer.trace.append("length")

    def _extend_model_replay_buffer(self):
        self.trainer.trace.append("extend")

    def _rollout_model(self, deterministic=False):
        self.trainer.trace.append("modelrollout")
        return OrderedDict(mean_rollout_length=1.0)

    def _do_training(self):
        self.trainer.trace.append(f"sac({self.replay_buffer.size})")
        self.trainer.calls += 1


def make_mbpo(tmp_path, trace, **kw):
    alg = make_run(tmp_path, trace, None, cls=StubMBPO, **kw)
    alg.algo = SimpleNamespace(ctx=alg.trainer.ctx)
    alg.model_train_freq, alg.real_ratio, alg.deterministic, alg._rollout_stat = 16, 0.5, False, OrderedDict()
    return alg


MBPO_TRACE = ("stats0 step0:rand*2 sync:c0 model length extend modelrollout sync:c0 step0:pi sync:c0 sac(12) sync:c0 step0:pi*3 sync:c0 "
              "sac(24) sync:c0*2 model length extend modelrollout sync:c0 step0:pi*3 sync:c0 sac(36) sync:c0 step0:pi sync:c0 model length "
              "extend modelrollout sync:c0 step0:pi*2 sync:c0 sac(48) sync:c0*2 eval0 stats0 row0=0 snap0*2 extra0 end0 "
              "stats0 step0:pi sync:c0 model length extend modelrollout sync:c0 step0:pi*2 sync:c0 sac(60) sync:c0 step0:pi*2 sync:c0 "
              "model length extend modelrollout sync:c0 step0:pi sync:c0 sac(72) sync:c0 step0:pi*3 sync:c0 sac(84) sync:c0*2 model length "
              "extend modelrollout sync:c0 step0:pi*2 sync:c0 eval0 stats0 row0=1 snap0*2 extra0 end0")
MBPO_ROWS = [row(4.0, 4.0, 1.5, 12.0, 4, 48, 12, 0), row(7.0, 7.0, 1.5, 11.0, 7, 92, 23, 1)]


def test_mbpo(tmp_path):
    trace = []
    alg = make_mbpo(tmp_path, trace, num_epochs=2)
    alg.train()
    assert fold(trace) == MBPO_TRACE
    assert rows(alg) == MBPO_ROWS


# ---- (g): MBPO given eval_async evaluates between epochs, says so, and builds neither a frozen copy nor a second sampler
def test_mbpo_given_eval_async_takes_the_fallback(tmp_path, capsys):
    trace, copies = [], []
    ctx, ectx = Ctx(trace, "c0"), Ctx(trace, "eval")
    policy = SimpleNamespace(h=1, copy=lambda ctx: copies.append(ctx) or policy)
    sampler = DeviceEvalSampler(SimpleNamespace(ctx=ectx), SimpleNamespace(stochastic_policy=policy), 8, 5)
    assert sampler._handles() == (1, None, True)          # a deterministic device evaluation on a stream of its own: a plain run overlaps it
    alg = StubMBPO.__new__(StubMBPO)
    DeviceRLAlgorithm.__init__(alg, Trainer(trace, 0, ctx), None, Env(trace, 0), EvalEnv(trace, 0), object(), replay_buffer=Ring(),
                               eval_sampler=sampler, log_dir=str(tmp_path / "run"), eval_async=True, **SCHEDULE)
    out = capsys.readouterr().out
    assert alg.eval_async is None and not copies
    assert out.count("evaluating between epochs") == 1 and "MBPO" in out
