#!/usr/bin/env python
"""MBPO experiment script on the MI355X engine — the contract of the reference's run_scripts/mbpo_exp_script.py:
`python run_scripts/mbpo_exp_script.py -e <spec.yaml> -g <gpu>`, variant keys env_specs / mbpo_params / bnn_params / sac_params /
seed / exp_name / exp_id (load_params resumes).  The planar tasks (hopper, walker, halfcheetah) and the truncated-observation 3-D
tasks of the reference's Ant / Humanoid specs (ant_trunc_obs, humanoid_trunc_obs: qpos[2:] | qvel), at any BNN width up to 400.
Plain `ant` / `humanoid` are refused: the terminal predicates are written for the truncated layout, and a model over the 111- /
376-wide observations is not wanted."""
from _common import flatten_spec, ia, main, make_envs, start, train, vec_env_kwargs_of  # noqa: F401

from ilswiss_amd.envs.terminals import get_terminal_func
from ilswiss_amd.mbpo import BNN, MBPO, BNNTrainer

# env_name -> the terminal predicate's name (rlkit/envs/terminals.py): the planar tasks and the truncated-observation 3-D tasks
TERMINALS = dict(hopper="hopper", walker="walker2d", walker2d="walker2d", halfcheetah="halfcheetah", half_cheetah="halfcheetah",
                 ant_trunc_obs="ant", humanoid_trunc_obs="humanoid")


def experiment(variant, gpu=0, log_dir=None):
    name = variant["env_specs"]["env_name"]
    if name not in TERMINALS:
        hint = f" (use {name}_trunc_obs, the task the reference's MBPO spec names)" if name in ("ant", "humanoid") else ""
        raise NotImplementedError(f"MBPO on env_name={name!r}: the device model rollout covers {sorted(TERMINALS)}{hint}")
    vec_kwargs = vec_env_kwargs_of(variant, "MBPO", "its device termination predicates and model rollouts read observation columns as raw quantities")
    ctx = start(variant, gpu)
    training_env, eval_env, env = make_envs(variant, ctx, **vec_kwargs)
    obs_dim, action_dim = training_env.obs_dim, training_env.act_dim
    sac_params = dict(variant["sac_params"])
    net_size, num_hidden = sac_params.pop("net_size"), sac_params.pop("num_hidden_layers")
    sac_params.pop("vf_lr", None)   # SAC-alpha has no value net (the reference's SoftActorCritic swallows it)
    alg = dict(variant["mbpo_params"])
    qf1 = ia.FlattenMlp(hidden_sizes=num_hidden * [net_size], input_size=obs_dim + action_dim, output_size=1, ctx=ctx)
    qf2 = ia.FlattenMlp(hidden_sizes=num_hidden * [net_size], input_size=obs_dim + action_dim, output_size=1, ctx=ctx)
    policy = ia.ReparamTanhMultivariateGaussianPolicy(hidden_sizes=num_hidden * [net_size], obs_dim=obs_dim, action_dim=action_dim, ctx=ctx)
    sac_trainer = ia.SoftActorCritic(policy=policy, qf1=qf1, qf2=qf2, env=env, max_batch=alg.get("batch_size", 256), **sac_params)
    bnn_params = dict(variant["bnn_params"])
    bnn = BNN(hidden_sizes=bnn_params["num_hidden_layers"] * [bnn_params["net_size"]], input_size=obs_dim + action_dim,
              output_size=obs_dim + 1, num_nets=bnn_params["num_nets"], ctx=ctx)
    bnn_trainer = BNNTrainer(bnn=bnn, **bnn_params)
    algorithm = MBPO(env=env, training_env=training_env, eval_env=eval_env, model=bnn_trainer, algo=sac_trainer,
                     exploration_policy=policy, is_terminal=get_terminal_func(TERMINALS[name]), log_dir=log_dir, **alg)
    bnn_trainer.logger = algorithm.logger
    train(algorithm, variant)
    return algorithm


if __name__ == "__main__":
    main(experiment, "mbpo")
