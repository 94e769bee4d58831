#!/usr/bin/env python
"""DQN / Double DQN experiment script on the MI355X engine: `python run_scripts/dqn_exp_script.py -e <variant.yaml> -g <gpu>`, variant
keys env_specs / net_size / num_hidden_layers / double_dqn / dqn_params / rl_alg_params / seed.  The reference ships no DQN script (its
rlkit/torch/algorithms/dqn/dqn.py does not import); the contract is that of its discrete_sac_exp_script.py with `dqn_params` = the keywords
of DQN.__init__ (dqn.py:17-29).  The action space must be Discrete.  The exploration policy is ArgmaxDiscretePolicy(qf, epsilon) — the
trained network itself under epsilon-greedy —, evaluation its deterministic form.  Several runs per process (`-e a.yaml b.yaml`,
run_experiment.py --group) and split runs (rl_alg_params.split_ranks > 1) are refused: there is no grouped or split DQN step."""
import argparse

import yaml
from _common import flatten_spec, ia, main, make_envs, split_ranks_of, start, train, vec_env_kwargs_of  # noqa: F401

from ilswiss_amd.algorithm import DeviceRLAlgorithm
from ilswiss_amd.envs.vecenv import Discrete


def experiment(variant, gpu=0, log_dir=None):
    if split_ranks_of(variant):
        raise SystemExit("DQN: rl_alg_params.split_ranks > 1 is not supported (no split DQN step)")
    vec_kwargs = vec_env_kwargs_of(variant)   # env_specs.vec_env_kwargs: norm_obs / update_obs_rms
    ctx = start(variant, gpu)
    training_env, eval_env, env = make_envs(variant, ctx, **vec_kwargs)
    if not isinstance(env.action_space, Discrete):
        raise SystemExit(f"DQN needs a Discrete action space; {variant['env_specs']['env_name']} has {type(env.action_space).__name__}")
    hid = variant["num_hidden_layers"] * [variant["net_size"]]
    qf = ia.FlattenMlp(hidden_sizes=hid, input_size=training_env.obs_dim, output_size=env.action_space.n, ctx=ctx)
    alg, params = dict(variant["rl_alg_params"]), dict(variant["dqn_params"])
    policy = ia.ArgmaxDiscretePolicy(qf, params.get("epsilon", 0.1))
    cls = ia.DoubleDQN if variant.get("double_dqn") else ia.DQN
    trainer = cls(qf, policy=policy, max_batch=alg.get("batch_size", 256), **params)
    algorithm = DeviceRLAlgorithm(trainer=trainer, env=env, training_env=training_env, eval_env=eval_env,
                                  exploration_policy=policy, log_dir=log_dir, **alg)
    train(algorithm, variant)
    return algorithm


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("-e", "--experiment", nargs="+", default=[])
    files = ap.parse_known_args()[0].experiment
    if len(files) > 1:   # `-e a.yaml b.yaml`: what run_experiment.py --group K starts
        raise SystemExit("DQN: several runs per process (--group K) are not supported; start one process per run")
    for path in files:   # before main(), which would start the ranks of a split run
        with open(path) as f:
            if split_ranks_of(flatten_spec(yaml.safe_load(f))):
                raise SystemExit("DQN: rl_alg_params.split_ranks > 1 is not supported (no split DQN step)")
    main(experiment, "dqn")
