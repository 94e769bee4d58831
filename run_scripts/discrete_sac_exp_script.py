#!/usr/bin/env python
"""Discrete SAC experiment script on the MI355X engine — same contract as the reference's run_scripts/discrete_sac_exp_script.py:
`python run_scripts/discrete_sac_exp_script.py -e <variant.yaml> -g <gpu>`, variant keys env_specs / net_size / num_hidden_layers /
sac_params / rl_alg_params / seed.  The action space must be Discrete (the env is wrapped in ProxyEnv, not NormalizedBoxEnv,
discrete_sac_exp_script.py:43-49).  Several runs per process (`-e a.yaml b.yaml`, run_experiment.py --group) and split runs
(rl_alg_params.split_ranks > 1) are refused: there is no grouped or split discrete SAC step."""
import argparse

import yaml
from _common import flatten_spec, ia, main, make_envs, split_ranks_of, start, train, vec_env_kwargs_of  # noqa: F401

from ilswiss_amd.algorithm import DeviceRLAlgorithm
from ilswiss_amd.discrete_sac import DiscreteSoftActorCritic
from ilswiss_amd.envs.vecenv import Discrete


def experiment(variant, gpu=0, log_dir=None):
    if split_ranks_of(variant):
        raise SystemExit("discrete SAC: rl_alg_params.split_ranks > 1 is not supported (no split discrete SAC step)")
    vec_kwargs = vec_env_kwargs_of(variant)   # env_specs.vec_env_kwargs: norm_obs / update_obs_rms
    ctx = start(variant, gpu)
    training_env, eval_env, env = make_envs(variant, ctx, **vec_kwargs)
    if not isinstance(env.action_space, Discrete):   # discrete_sac_exp_script.py:41
        raise SystemExit(f"discrete SAC needs a Discrete action space; {variant['env_specs']['env_name']} has {type(env.action_space).__name__}")
    obs_dim, action_dim = training_env.obs_dim, env.action_space.n
    hid = variant["num_hidden_layers"] * [variant["net_size"]]
    qf1 = ia.FlattenMlp(hidden_sizes=hid, input_size=obs_dim, output_size=action_dim, ctx=ctx)
    qf2 = ia.FlattenMlp(hidden_sizes=hid, input_size=obs_dim, output_size=action_dim, ctx=ctx)
    policy = ia.DiscretePolicy(hidden_sizes=hid, obs_dim=obs_dim, action_dim=action_dim, ctx=ctx)
    alg = dict(variant["rl_alg_params"])
    trainer = DiscreteSoftActorCritic(policy=policy, qf1=qf1, qf2=qf2, max_batch=alg.get("batch_size", 256), **variant["sac_params"])
    algorithm = DeviceRLAlgorithm(trainer=trainer, env=env, training_env=training_env, eval_env=eval_env,
                                  exploration_policy=policy, log_dir=log_dir, **alg)
    train(algorithm, variant)
    return algorithm


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("-e", "--experiment", nargs="+", default=[])
    files = ap.parse_known_args()[0].experiment
    if len(files) > 1:   # `-e a.yaml b.yaml`: what run_experiment.py --group K starts
        raise SystemExit("discrete SAC: several runs per process (--group K) are not supported; start one process per run")
    for path in files:   # before main(), which would start the ranks of a split run
        with open(path) as f:
            if split_ranks_of(flatten_spec(yaml.safe_load(f))):
                raise SystemExit("discrete SAC: rl_alg_params.split_ranks > 1 is not supported (no split discrete SAC step)")
    main(experiment, "discrete_sac")
