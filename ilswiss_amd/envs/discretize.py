"""rlkit/envs/wrappers.py:400-446: `Discretized` (a Discrete space that remembers its grid) and `DiscretEnv`, which turns a Box-action env
into a discrete one over the grid of `granularity` points per action dimension (np.meshgrid in its default 'xy' order, as the reference
builds it), or over an explicit list of `possible_actions`.  Used by GCSL's CLASS mode on the point-reach stand-in."""
import numpy as np

from .vecenv import Discrete


class Discretized(Discrete):
    def __init__(self, n, n_dims, granularity):
        self.n_dims, self.granularity = n_dims, granularity
        assert n == granularity ** n_dims
        super().__init__(n)


class DiscretEnv:
    def __init__(self, env, granularity=10, possible_actions=None):
        self._wrapped_env = env
        self.raw_action_space = env.action_space
        assert not isinstance(self.raw_action_space, Discrete), "already discrete"
        if possible_actions is not None:
            self.base_actions = np.asarray(possible_actions)
            n_dims, granularity = 1, len(self.base_actions)
        else:
            meshed = np.meshgrid(*[np.linspace(lo, hi, granularity) for lo, hi in zip(env.action_space.low, env.action_space.high)])
            self.base_actions = np.array([m.flat[:] for m in meshed]).T
            n_dims = env.action_space.shape[0]
        self.action_space = Discretized(len(self.base_actions), n_dims, granularity)
        self.observation_space = env.observation_space

    @property
    def wrapped_env(self):
        return self._wrapped_env

    def reset(self, **kwargs):
        return self._wrapped_env.reset(**kwargs)

    def step(self, action):
        """`action`: an index, or an array holding one (what CatagorialPolicy.get_actions returns per row)."""
        i = int(np.asarray(action).reshape(-1)[0])
        return self._wrapped_env.step(self.base_actions[i])

    def __getattr__(self, name):     # compute_reward, tol, reward_type, ... of the wrapped goal env
        if name == "_wrapped_env":
            raise AttributeError(name)
        return getattr(self._wrapped_env, name)
