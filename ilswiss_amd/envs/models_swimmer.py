"""Swimmer model for k_swimmer_step (csrc/swimmer_env.h): plain data.

The reference builds `swimmer` (rlkit/envs/envs_dict.py) from gym 0.22's MuJoCo XML model `swimmer.xml`; neither gym nor MuJoCo nor the
XML file exists in this environment, so the constants below are authored from public knowledge of that file and are UNVERIFIED against
MuJoCo (DESIGN.md section 20 lists the doubts).  Task rules (observation, reward, reset noise) are gym 0.22's SwimmerEnv and live in the
kernel, not here.

Conventions: the plane is (x, y), angles counter-clockwise about its normal z.  Link 0 is the torso; it carries the root joints at its
origin: DoF 0 slide x, DoF 1 slide y, DoF 2 hinge.  Link k >= 1 hinges on link k - 1 (DoF 2 + k, angle relative to the parent); a link's
absolute angle is the sum of the hinge angles up to it.  `anchor[k]` is link k's hinge in its parent's frame, `com[k]` the centre of mass
in the link's own frame.  `inertia[k]` = (I_x, I_y, I_z) about the centre of mass, x along the link and z normal to the plane; `box[k]`
the full sides of the box of equal inertia, which the drag model uses.  The lists indexed by DoF (armature, damping, limited, range,
gear, init_qpos) have n_link + 2 entries.  Capsule mass and in-plane inertia follow models.capsule_mass_inertia (density 1000).
"""
import math

from .models import capsule_axial_inertia, capsule_mass_inertia
from .models_cartchain import LIMIT_SOLIMP, LIMIT_SOLREF


def inertia_box(mass, inertia):
    """Full sides of the solid box with this mass and these principal inertias (MuJoCo's equivalent inertia box)."""
    ix, iy, iz = inertia
    return (math.sqrt(6.0 * (iy + iz - ix) / mass), math.sqrt(6.0 * (ix + iz - iy) / mass), math.sqrt(6.0 * (ix + iy - iz) / mass))


def _free_chain(capsules, anchors, timestep, frame_skip, armature, hinge_range, gear, ctrl_range, density, viscosity):
    """capsules: (p1, p2, radius) per link in its own frame, along its x axis, the torso first."""
    mass, inertia, com, box = [], [], [], []
    for p1, p2, rad in capsules:
        assert p1[1] == 0.0 and p2[1] == 0.0, "a link's capsule lies along its own x axis"
        m, iz = capsule_mass_inertia(p1, p2, rad)
        ix = capsule_axial_inertia(p1, p2, rad)
        mass.append(m)
        inertia.append((ix, iz, iz))      # a capsule along x: I_y = I_z
        box.append(inertia_box(m, inertia[-1]))
        com.append((0.5 * (p1[0] + p2[0]), 0.5 * (p1[1] + p2[1])))
    nl = len(capsules)
    n = nl + 2
    return dict(n_link=nl, timestep=timestep, frame_skip=frame_skip, pgs_iters=30, density=density, viscosity=viscosity,
                mass=mass, inertia=inertia, box=box, com=com, anchor=list(anchors),
                armature=[armature] * n, damping=[0.0] * n, limited=[0, 0, 0] + [1] * (nl - 1),
                range=[(0.0, 0.0)] * 3 + [tuple(hinge_range)] * (nl - 1), gear=[0.0] * 3 + [gear] * (nl - 1), init_qpos=[0.0] * n,
                ctrl_range=tuple(ctrl_range), limit_solref=LIMIT_SOLREF, limit_solimp=LIMIT_SOLIMP)


def swimmer():
    """gym 0.22 swimmer.xml: timestep 0.01, RK4 (frame_skip 4 in SwimmerEnv), medium density 4000 and viscosity 0.1, three capsule links
    of length 1 and radius 0.1, armature 0.1 on every joint, both hinges limited to +-100 degrees, motors of gear 150."""
    link_back = ((0.0, 0.0), (-1.0, 0.0), 0.1)      # mid and back extend 1 backwards from their hinge
    return _free_chain(capsules=[((1.5, 0.0), (0.5, 0.0), 0.1), link_back, link_back],
                       anchors=[(0.0, 0.0), (0.5, 0.0), (-1.0, 0.0)], timestep=0.01, frame_skip=4, armature=0.1,
                       hinge_range=(math.radians(-100.0), math.radians(100.0)), gear=150.0, ctrl_range=(-1.0, 1.0),
                       density=4000.0, viscosity=0.1)


MODELS_SWIMMER = {"swimmer": swimmer}
