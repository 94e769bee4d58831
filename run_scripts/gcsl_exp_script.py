#!/usr/bin/env python
"""GCSL experiment script — contract of the reference's run_scripts/gcsl_exp_script.py: `-e <variant.yaml> -g <gpu>`, variant keys
env_specs (incl. discretize / discret_kwargs) / net_size / num_hidden_layers / gcsl_params (mode) / rl_alg_params (incl. use_horizons,
relabel_type) / seed.  The reference's goal envs are gym's Fetch robots (MuJoCo); here `env_name: point-reach` selects the stand-in of
ilswiss_amd/her.py.  Writes progress.csv with the per-epoch success rate and return of the deterministic evaluation."""
from _common import ia, main, start  # noqa: F401

from ilswiss_amd import gcsl, her
from ilswiss_amd.algorithm import TabularLogger
from ilswiss_amd.envs import DiscretEnv


def experiment(variant, gpu=0, log_dir=None):
    ctx = start(variant, gpu)
    specs = variant["env_specs"]
    if specs["env_name"] != "point-reach":
        raise NotImplementedError(f"goal env {specs['env_name']!r}: the reference's Fetch envs need MuJoCo; only the stand-in 'point-reach' exists here")
    mode = variant["gcsl_params"]["mode"]
    discretize = bool(specs.get("discretize", False))
    if discretize != (mode == "CLASS"):                   # gcsl_exp_script.py:73-74 (and MSE needs the continuous actions)
        raise ValueError(f"GCSL mode {mode!r} with discretize={discretize}: CLASS needs a discretised env, MSE a continuous one")
    # the reference builds the evaluation env and the training env separately, both seeded with the variant's seed (gcsl_exp_script.py)
    env = her.PointReachEnv(seed=int(variant.get("seed", 0)), **specs.get("env_kwargs", {}))
    eval_env = her.PointReachEnv(seed=int(variant.get("seed", 0)), **specs.get("env_kwargs", {}))
    sp = env.observation_space.spaces
    obs_dim, goal_dim, raw_act = sp["observation"].shape[0], sp["desired_goal"].shape[0], env.action_space.shape[0]
    alg = dict(variant["rl_alg_params"])
    T = alg["max_path_length"] if alg.get("use_horizons") else 0
    hid = variant["num_hidden_layers"] * [variant["net_size"]]
    B = alg.get("batch_size", 128)
    if discretize:
        env = DiscretEnv(env, **specs.get("discret_kwargs", {}))
        eval_env = DiscretEnv(eval_env, **specs.get("discret_kwargs", {}))
        policy = gcsl.CatagorialConditionPolicy(hidden_sizes=hid, obs_dim=obs_dim, condition_dim=goal_dim + T, action_dim=env.action_space.n,
                                                batch_norm=True, max_rows=max(B, 64), ctx=ctx)
    else:
        policy = gcsl.MlpGaussianAndEpsilonConditionPolicy(hidden_sizes=hid, obs_dim=obs_dim, condition_dim=goal_dim + T, action_dim=raw_act,
                                                           action_space=env.action_space, output_activation="tanh", batch_norm=True, ctx=ctx)
    trainer = gcsl.GCSL(policy, use_horizons=alg.get("use_horizons", False), goal_dim=goal_dim, max_batch=B, **variant["gcsl_params"])
    algorithm = gcsl.GoalHorizonRL(trainer, env, policy, eval_env=eval_env, **alg)
    logger = TabularLogger(log_dir)
    for epoch, rec in enumerate(algorithm.train()):
        logger.record_tabular("Epoch", epoch)
        logger.record_tabular("Success Rate", rec["success"])
        logger.record_tabular("AverageReturn", rec["ret"])
        for k in ("CE Loss", "Accuracy", "MSE"):
            if k in rec:
                logger.record_tabular(k, rec[k])
        logger.record_tabular("Number of env steps total", (epoch + 1) * algorithm.num_steps_per_epoch)
        logger.dump_tabular()
    return algorithm


if __name__ == "__main__":
    main(experiment, "gcsl")
