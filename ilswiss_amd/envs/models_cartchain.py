"""Cart-and-poles models for the classic-control engine's k_cartchain_step (csrc/classic_env.h): plain data.

The reference builds `invertedpendulum` / `inverteddoublependulum` (rlkit/envs/envs_dict.py) from gym 0.22's MuJoCo XML models
`inverted_pendulum.xml` / `inverted_double_pendulum.xml`; neither gym nor MuJoCo nor the XML files exist in this environment, so the
constants below are authored from public knowledge of those files and are UNVERIFIED against MuJoCo.  Task rules (observation, reward,
termination, reset noise) are gym 0.22's InvertedPendulumEnv / InvertedDoublePendulumEnv and live in the kernel, not here.

Conventions: planar (x along the rail, z up).  DoF 0 is the cart's slide along x; DoF k >= 1 is a hinge carrying pole k, its angle
relative to the parent.  A pole's absolute angle is phi_k = jsign * (q_1 + ... + q_k), counter-clockwise in the (x, z) plane; jsign = -1
is MuJoCo's positive rotation about the y axis these hinges use (a positive angle tips the pole towards +x).  Bodies: 0 = cart, k = pole k.
`anchor[k]` is hinge k's position in its parent's frame, `com[k]` the centre of mass in the body's own frame, `tip` the site the
InvertedDoublePendulum reward reads, in the last pole's frame.  Capsule mass / inertia follow models.capsule_mass_inertia (density 1000).
"""
import math

from .models import capsule_mass_inertia

LIMIT_SOLREF = (0.02, 1.0)           # MuJoCo's default solreflimit
LIMIT_SOLIMP = (0.9, 0.95, 0.001)    # MuJoCo's default solimplimit


def _chain(capsules, anchors, tip, timestep, frame_skip, damping, limited, ranges, gear, ctrl_range):
    """capsules: (p1, p2, radius) per body in its own frame, the cart first."""
    mass, inertia, com = [], [], []
    for p1, p2, rad in capsules:
        m, i = capsule_mass_inertia(p1, p2, rad)
        mass.append(m)
        inertia.append(i)
        com.append((0.5 * (p1[0] + p2[0]), 0.5 * (p1[1] + p2[1])))
    n = len(capsules)
    return dict(n_pole=n - 1, timestep=timestep, frame_skip=frame_skip, pgs_iters=30, gravity=9.81, jsign=-1.0,
                mass=mass, inertia=inertia, com=com, anchor=list(anchors), tip=tuple(tip),
                armature=[0.0] * n, damping=list(damping), limited=list(limited), range=[tuple(r) for r in ranges],
                gear=gear, ctrl_range=tuple(ctrl_range), limit_solref=LIMIT_SOLREF, limit_solimp=LIMIT_SOLIMP)


CART = ((-0.1, 0.0), (0.1, 0.0), 0.1)   # capsule of radius 0.1 and half-length 0.1 along x


def inverted_pendulum():
    """gym 0.22 inverted_pendulum.xml: timestep 0.02 (frame_skip 2 in InvertedPendulumEnv), joint damping 1, both joints limited."""
    return _chain(capsules=[CART, ((0.0, 0.0), (0.001, 0.6), 0.049)], anchors=[(0.0, 0.0), (0.0, 0.0)], tip=(0.001, 0.6),
                  timestep=0.02, frame_skip=2, damping=[1.0, 1.0], limited=[1, 1],
                  ranges=[(-1.0, 1.0), (math.radians(-90.0), math.radians(90.0))], gear=100.0, ctrl_range=(-3.0, 3.0))


def inverted_double_pendulum():
    """gym 0.22 inverted_double_pendulum.xml: timestep 0.01 (frame_skip 5), joint damping 0.05, only the slide limited."""
    pole = ((0.0, 0.0), (0.0, 0.6), 0.045)
    return _chain(capsules=[CART, pole, pole], anchors=[(0.0, 0.0), (0.0, 0.0), (0.0, 0.6)], tip=(0.0, 0.6),
                  timestep=0.01, frame_skip=5, damping=[0.05, 0.05, 0.05], limited=[1, 0, 0],
                  ranges=[(-1.0, 1.0), (0.0, 0.0), (0.0, 0.0)], gear=500.0, ctrl_range=(-1.0, 1.0))


MODELS_CARTCHAIN = {"invertedpendulum": inverted_pendulum, "inverteddoublependulum": inverted_double_pendulum}
