"""LunarLanderContinuous model for k_lunar_step (csrc/lunar_env.h): plain data.

The reference builds `lunarlandercont` (rlkit/envs/envs_dict.py) from gym 0.22's `lunar_lander.py` on Box2D; neither gym nor Box2D
exists in this environment, so the constants below are authored from public knowledge of that file and are UNVERIFIED against it
(DESIGN.md section 23 lists the doubts).  Task rules (engines, observation, shaping, termination, reset) are gym 0.22's and live in the
kernel; the dynamics are this repository's own: ONE rigid body (hull plus two legs held at their spring-rest angle), soft contacts at
the two foot points only.  Everything the kernel needs beyond the task constants is derived here, on the host.

Conventions: the plane is (x, y), y up, angles counter-clockwise; lengths in metres (gym's pixels / SCALE).  The hull frame's origin is
the hull body's origin (the point gym's `lander.position` reports); `hull_poly`, `foot` and `com` are in that frame.  Foot 0 is the
left one (x < 0, gym's i = +1), foot 1 the right one.
"""
import math

FPS = 50.0
SCALE = 30.0
VIEWPORT_W, VIEWPORT_H = 600.0, 400.0
CHUNKS = 11
LANDER_POLY = [(-14.0, 17.0), (-17.0, 0.0), (-17.0, -10.0), (17.0, -10.0), (17.0, 0.0), (14.0, 17.0)]   # pixels
LEG_AWAY, LEG_DOWN, LEG_W, LEG_H = 20.0, 18.0, 2.0, 8.0
LEG_REST_ANGLE = 0.4                  # the leg joints' springs rest at -+0.4 (gym's lowerAngle / upperAngle of the revolute joints)
HULL_DENSITY, LEG_DENSITY = 5.0, 1.0
# this repository's soft-row rule, critically damped, with a time constant of 0.1 s: the feet stand in for gym's sprung legs.  A
# touchdown at speed v sinks v * dmax * tc / e before it stops, and the hull's bottom is 0.205 above the feet, so the hull reaches the
# ground, and the episode ends, above about 5.9 m/s; at rest the feet sink g (dmax tc)^2 = 0.015.  (MuJoCo's default 0.02 s would stop
# a 29 m/s fall inside the legs' length: a lander that cannot crash on its feet.)
CONTACT_SOLREF = (0.1, 1.0)
CONTACT_SOLIMP = (0.9, 0.95, 0.001)


def polygon_mass_properties(poly, density):
    """(mass, (cx, cy), inertia about the centroid) of a simple polygon by the shoelace formulas; the vertex order may be either way."""
    a = cx = cy = j = 0.0
    n = len(poly)
    for k in range(n):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % n]
        cr = x0 * y1 - x1 * y0
        a += cr
        cx += (x0 + x1) * cr
        cy += (y0 + y1) * cr
        j += cr * (x0 * x0 + x0 * x1 + x1 * x1 + y0 * y0 + y0 * y1 + y1 * y1)
    a *= 0.5
    cx, cy = cx / (6.0 * a), cy / (6.0 * a)
    j /= 12.0                              # second moment about the origin, signed like the area
    mass = density * abs(a)
    inertia = density * abs(j) - mass * (cx * cx + cy * cy)
    return mass, (cx, cy), inertia


def _rot(phi, p):
    c, s = math.cos(phi), math.sin(phi)
    return (c * p[0] - s * p[1], s * p[0] + c * p[1])


def leg_polygon(i):
    """Leg i (= +1 left, -1 right) in the hull frame: a box of half-extents (LEG_W, LEG_H) / SCALE whose frame is turned by
    phi = -0.4 i and whose point (i LEG_AWAY, LEG_DOWN) / SCALE sits on the hull's origin."""
    phi = -LEG_REST_ANGLE * i
    hw, hh = LEG_W / SCALE, LEG_H / SCALE
    centre = (-i * LEG_AWAY / SCALE, -LEG_DOWN / SCALE)
    return [_rot(phi, (centre[0] + sx * hw, centre[1] + sy * hh)) for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def foot_point(i):
    """The middle of leg i's lower edge: R(phi_i) (-i LEG_AWAY, -(LEG_DOWN + LEG_H)) / SCALE."""
    return _rot(-LEG_REST_ANGLE * i, (-i * LEG_AWAY / SCALE, -(LEG_DOWN + LEG_H) / SCALE))


def lunar():
    """gym 0.22 LunarLanderContinuous: 50 frames per second, 30 pixels per metre, a 600 x 400 viewport (W = 20, H = 40 / 3), gravity
    -10; main engine 13, side engines 0.6; terrain of 11 chunks with a flat helipad at H / 4."""
    w, h = VIEWPORT_W / SCALE, VIEWPORT_H / SCALE
    hull = [(x / SCALE, y / SCALE) for x, y in LANDER_POLY]
    parts = [polygon_mass_properties(hull, HULL_DENSITY)] + [polygon_mass_properties(leg_polygon(i), LEG_DENSITY) for i in (1, -1)]
    mass = sum(p[0] for p in parts)
    com = (sum(p[0] * p[1][0] for p in parts) / mass, sum(p[0] * p[1][1] for p in parts) / mass)
    assert abs(com[0]) < 1e-12, "hull and legs are mirror images about the hull's y axis"
    com = (0.0, com[1])                    # exactly on the axis: the main engine, which fires along it, gives no torque
    inertia = sum(p[2] + p[0] * ((p[1][0] - com[0]) ** 2 + (p[1][1] - com[1]) ** 2) for p in parts)
    return dict(fps=FPS, scale=SCALE, viewport_w=VIEWPORT_W, viewport_h=VIEWPORT_H, w=w, h=h, gravity=-10.0,
                main_engine_power=13.0, side_engine_power=0.6, initial_random=1000.0,
                side_engine_height=14.0, side_engine_away=12.0, leg_away=LEG_AWAY, leg_down=LEG_DOWN, leg_w=LEG_W, leg_h=LEG_H,
                leg_rest_angle=LEG_REST_ANGLE, hull_density=HULL_DENSITY, leg_density=LEG_DENSITY,
                chunks=CHUNKS, helipad_y=h / 4.0, hull_poly=hull,
                mass=mass, com=com, inertia=inertia, foot=[foot_point(1), foot_point(-1)],
                # solver: substeps per env step, Gauss-Seidel sweeps, Box2D's friction mix sqrt(0.2 * 0.1) of leg and ground
                frame_skip=4, pgs_iters=30, friction=math.sqrt(0.2 * 0.1),
                contact_solref=CONTACT_SOLREF, contact_solimp=CONTACT_SOLIMP,
                # Box2D's public sleep defaults: b2_linearSleepTolerance, b2_angularSleepTolerance, b2_timeToSleep
                sleep_lin_tol=0.01, sleep_ang_tol=math.radians(2.0), sleep_time=0.5)


MODELS_LUNAR = {"lunarlandercont": lunar}
