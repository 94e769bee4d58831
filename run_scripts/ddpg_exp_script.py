#!/usr/bin/env python
"""DDPG experiment script on the MI355X engine, in the shape of run_scripts/td3_exp_script.py (the reference ships the trainer,
rlkit/torch/algorithms/ddpg/ddpg.py, and the exploration strategies, but no DDPG run script or spec):
`python run_scripts/ddpg_exp_script.py -e <variant.yaml> -g <gpu>`, variant keys env_specs / net_size / num_hidden_layers /
ddpg_params / exploration (type: ou | gaussian, plus the strategy's constructor keywords) / rl_alg_params / seed."""
from _common import ia, main, make_envs, start, train, vec_env_kwargs_of  # noqa: F401

from ilswiss_amd.algorithm import DeviceRLAlgorithm
from ilswiss_amd.ddpg import DDPG, GaussianStrategy, MlpPolicy, OUStrategy, PolicyWrappedWithExplorationStrategy

STRATEGIES = dict(ou=OUStrategy, gaussian=GaussianStrategy)


def experiment(variant, gpu=0, log_dir=None):
    vec_kwargs = vec_env_kwargs_of(variant)   # env_specs.vec_env_kwargs: norm_obs / update_obs_rms (refusals come before the device is opened)
    ctx = start(variant, gpu)
    training_env, eval_env, env = make_envs(variant, ctx, **vec_kwargs)
    obs_dim, action_dim = training_env.obs_dim, training_env.act_dim
    hid = variant["num_hidden_layers"] * [variant["net_size"]]
    qf = ia.FlattenMlp(hidden_sizes=hid, input_size=obs_dim + action_dim, output_size=1, ctx=ctx)
    policy = MlpPolicy(hidden_sizes=hid, obs_dim=obs_dim, action_dim=action_dim, output_activation="tanh", ctx=ctx)
    expl = dict(variant["exploration"])
    es = STRATEGIES[expl.pop("type")](training_env.single_action_space, **expl)
    exploration_policy = PolicyWrappedWithExplorationStrategy(exploration_strategy=es, policy=policy)
    alg = dict(variant["rl_alg_params"])
    trainer = DDPG(policy=policy, qf=qf, max_batch=alg.get("batch_size", 256), **variant["ddpg_params"])
    algorithm = DeviceRLAlgorithm(trainer=trainer, env=env, training_env=training_env, eval_env=eval_env,
                                  exploration_policy=exploration_policy, log_dir=log_dir, **alg)
    train(algorithm, variant)
    return algorithm


if __name__ == "__main__":
    main(experiment, "ddpg")
