"""Vectorised environments on the device: `vecenv.HipVectorEnv` / `get_envs` (the BaseVectorEnv protocol over libilsx's batched
planar, 3-D and classic-control steppers, CartPole's `Discrete` action space) and `models` (the articulated-body descriptions of Hopper, Walker2d and HalfCheetah), `envpool` (the reference's EnvpoolEnv surface)
`terminals` (batched terminal predicates) and `discretize` (DiscretEnv over a Box-action env)."""
from .models_goal import MODELS_GOAL  # noqa: F401
from .models_lunar import MODELS_LUNAR  # noqa: F401
from .models_swimmer import MODELS_SWIMMER  # noqa: F401
from .vecenv import CARTCHAIN, CLASSIC, CLASSIC_KINDS, GOAL, GYM_CLASSIC, LUNAR, SWIMMER, Discrete, HipVectorEnv, MinmaxEnv, ProxyEnv, ScaledEnv, get_env, get_envs  # noqa: F401
from .envpool import EnvpoolEnv, HipEnvPool  # noqa: F401,E402
from .terminals import get_terminal_func  # noqa: F401,E402
from .discretize import DiscretEnv, Discretized  # noqa: F401,E402
