"""numpy float64 statement of the Swimmer stepper (the thing k_swimmer_step of csrc/swimmer_env.h must reproduce), batched over envs,
with generic linear algebra: Jacobians by recursion over the parent chain, np.linalg.solve for every solve, projected Gauss-Seidel as a
loop over a row list, the fluid model written once from its formulas INCLUDING the box sides computed from the inertias (so the host-side
box computation of models_swimmer.py is checked too).  Written without the kernel's closed forms, so that agreement means something.
Test infrastructure; the constants come from ilswiss_amd/envs/models_swimmer.py.

Model: link 0 carries DoF 0 (slide x), 1 (slide y) and 2 (hinge) at its origin; link k >= 1 hinges on link k - 1 (DoF 2 + k).  phi_b is a
link's absolute angle, counter-clockwise in (x, y).
    M(q) qdd + c(q, qd) = tau + J^T f,   M = sum_b m_b Jc_b^T Jc_b + I_b Jphi_b^T Jphi_b + diag(armature)
    tau = gear * ctrl - damping * qd + sum_b (Jc_b^T R(phi_b) f_b + Jphi_b^T t_b)      (no gravity in the plane, no contacts)
Fluid (inertia-box model): b_x = sqrt(6 (I_y + I_z - I_x) / m), b_y, b_z likewise, d = (b_x + b_y + b_z) / 3; with (v_x, v_y) the velocity
of the link's centre of mass in the link's axes and w its angular rate,
    f_x = -3 pi beta d v_x - 1/2 rho b_y b_z |v_x| v_x,   f_y = -3 pi beta d v_y - 1/2 rho b_x b_z |v_y| v_y,
    t_z = -pi beta d^3 w - rho b_z (b_x^4 + b_y^4) |w| w / 64
Constraints: one unilateral soft row per violated joint limit, in DoF order:
    (A + R) f = aref - J qacc0,  A = J M^-1 J^T,  R_i = (1 - d_i) / d_i A_ii,  aref_i = -b v_i - k d_i r_i,
    b = 2 / (dmax tc),  k = 1 / (dmax^2 tc^2 dr^2),  d = impedance(|r|)
Integrator: classic RK4 on (q, qd) with the constraint solve inside every stage, frame_skip substeps.
Task rules: gym 0.22's SwimmerEnv behind NormalizedBoxEnv."""
import numpy as np


def rot(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def drot(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([np.stack([-s, -c], -1), np.stack([c, -s], -1)], -2)


def impedance(r_abs, solimp):
    d0, dmax, width = solimp
    x = np.minimum(r_abs / width, 1.0) if width > 0 else np.ones_like(r_abs)
    y = np.where(x < 0.5, 2.0 * x * x, 1.0 - 2.0 * (1.0 - x) ** 2)
    return d0 + y * (dmax - d0)


def mv(A, x):
    """[B, i, j] @ [j] or [B, j] -> [B, i]"""
    return np.einsum("bij,...j->bi", A, x)


class Swimmer:
    def __init__(self, model):
        self.m = model
        self.nl = model["n_link"]
        self.n = self.nl + 2
        self.obs_dim = 2 * self.n - 2
        self.act_dim = self.nl - 1
        self.parent = [-1] + list(range(self.nl - 1))
        self.act_dofs = [i for i in range(self.n) if model["gear"][i] != 0.0]

    # ---------------------------------------------------------------- kinematics ([B, ...] arrays)
    def kin(self, q, v):
        """Per link: COM Jacobian [B, 2, n], COM bias acceleration [B, 2], COM [B, 2], angular Jacobian [B, n], angle, angular rate."""
        m, n, nl, B = self.m, self.n, self.nl, q.shape[0]
        phi = np.zeros((B, nl)); Jphi = np.zeros((B, nl, n)); Jo = np.zeros((B, nl, 2, n))
        o = np.zeros((B, nl, 2)); ao = np.zeros((B, nl, 2))
        out = []
        for b in range(nl):
            p = self.parent[b]
            if p < 0:
                o[:, b] = q[:, :2]
                Jo[:, b, 0, 0] = 1.0; Jo[:, b, 1, 1] = 1.0
                phi[:, b] = q[:, 2]
                Jphi[:, b, 2] = 1.0
            else:
                a = np.asarray(m["anchor"][b], np.float64)
                wp = np.einsum("bj,bj->b", Jphi[:, p], v)
                o[:, b] = o[:, p] + mv(rot(phi[:, p]), a)
                Jo[:, b] = Jo[:, p] + np.einsum("bi,bj->bij", mv(drot(phi[:, p]), a), Jphi[:, p])
                ao[:, b] = ao[:, p] - (wp ** 2)[:, None] * mv(rot(phi[:, p]), a)
                phi[:, b] = phi[:, p] + q[:, 2 + b]
                Jphi[:, b] = Jphi[:, p]; Jphi[:, b, 2 + b] += 1.0
            r = np.asarray(m["com"][b], np.float64)
            w = np.einsum("bj,bj->b", Jphi[:, b], v)
            Jc = Jo[:, b] + np.einsum("bi,bj->bij", mv(drot(phi[:, b]), r), Jphi[:, b])
            ac = ao[:, b] - (w ** 2)[:, None] * mv(rot(phi[:, b]), r)
            c = o[:, b] + mv(rot(phi[:, b]), r)
            out.append((Jc, ac, c, Jphi[:, b].copy(), phi[:, b].copy(), w))
        return out

    def box(self, b):
        ix, iy, iz = self.m["inertia"][b]
        mass = self.m["mass"][b]
        return np.sqrt(6.0 * (iy + iz - ix) / mass), np.sqrt(6.0 * (ix + iz - iy) / mass), np.sqrt(6.0 * (ix + iy - iz) / mass)

    def fluid(self, b, vloc, w):
        """Force in the link's axes [B, 2] and torque [B] on link b."""
        rho, beta = self.m["density"], self.m["viscosity"]
        bx, by, bz = self.box(b)
        d = (bx + by + bz) / 3.0
        fx = -3.0 * np.pi * beta * d * vloc[:, 0] - 0.5 * rho * by * bz * np.abs(vloc[:, 0]) * vloc[:, 0]
        fy = -3.0 * np.pi * beta * d * vloc[:, 1] - 0.5 * rho * bx * bz * np.abs(vloc[:, 1]) * vloc[:, 1]
        tz = -np.pi * beta * d ** 3 * w - rho * bz * (bx ** 4 + by ** 4) * np.abs(w) * w / 64.0
        return np.stack([fx, fy], -1), tz

    def passive(self, q, v):
        """The fluid's generalised force [B, n]."""
        out = np.zeros_like(v)
        for b, (Jc, _ac, _c, Jp, phi, w) in enumerate(self.kin(q, v)):
            R = rot(phi)
            vc = np.einsum("bki,bi->bk", Jc, v)
            vloc = np.einsum("bki,bk->bi", R, vc)        # R^T vc
            f, tz = self.fluid(b, vloc, w)
            fw = np.einsum("bki,bi->bk", R, f)
            out += np.einsum("bki,bk->bi", Jc, fw) + Jp * tz[:, None]
        return out

    def dynamics(self, q, v, ctrl):
        """ctrl [B, act_dim] -> (qacc [B, n], rows active [B, n_rows] (bool), row forces [B, n_rows])."""
        m, n, B = self.m, self.n, q.shape[0]
        M = np.zeros((B, n, n)); rhs = np.zeros((B, n))
        for b, (Jc, ac, _c, Jp, _phi, _w) in enumerate(self.kin(q, v)):
            M += m["mass"][b] * np.einsum("bki,bkj->bij", Jc, Jc) + m["inertia"][b][2] * np.einsum("bi,bj->bij", Jp, Jp)
            rhs += m["mass"][b] * np.einsum("bki,bk->bi", Jc, -ac)
        M += np.diag(np.asarray(m["armature"], np.float64))
        rhs -= np.asarray(m["damping"], np.float64) * v
        rhs += self.passive(q, v)
        for k, i in enumerate(self.act_dofs):
            rhs[:, i] += m["gear"][i] * ctrl[:, k]
        qacc0 = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
        # ---- row list: one per limited DoF, in DoF order; sg = 0 where the limit is not violated
        rows = []
        for j in range(n):
            if not m["limited"][j]:
                continue
            lo, hi = m["range"][j]
            below = q[:, j] - lo < 0.0
            above = ~below & (hi - q[:, j] < 0.0)
            rows.append((j, np.where(below, 1.0, np.where(above, -1.0, 0.0)), np.where(below, q[:, j] - lo, np.where(above, hi - q[:, j], 0.0))))
        nr = len(rows)
        act_all = np.zeros((B, nr), bool); f_all = np.zeros((B, nr))
        if not rows:
            return qacc0, act_all, f_all
        idx = np.nonzero(np.any([sg != 0.0 for _j, sg, _r in rows], axis=0))[0]
        if idx.size == 0:
            return qacc0, act_all, f_all
        J = np.zeros((idx.size, nr, n)); r = np.zeros((idx.size, nr))
        for i, (j, sg, rr) in enumerate(rows):
            J[:, i, j] = sg[idx]; r[:, i] = rr[idx]
        active = np.any(J != 0.0, axis=2)
        Ms, vs, a0 = M[idx], v[idx], qacc0[idx]
        MinvJT = np.linalg.solve(Ms, J.transpose(0, 2, 1))
        A = J @ MinvJT
        tc, dr = m["limit_solref"]
        d0, dmax, width = m["limit_solimp"]
        d = impedance(np.abs(r), m["limit_solimp"])
        bdamp = 2.0 / (dmax * tc)
        kstiff = 1.0 / (dmax * dmax * tc * tc * dr * dr)
        Jv = np.einsum("brj,bj->br", J, vs)
        aref = -bdamp * Jv - kstiff * d * r
        diag = np.einsum("brr->br", A)
        R = (1.0 - d) / d * diag
        rhs_c = aref - np.einsum("brj,bj->br", J, a0)
        den = np.where(active, diag + R, 1.0)
        f = np.zeros((idx.size, nr))
        for _ in range(m["pgs_iters"]):
            for i in range(nr):
                res = rhs_c[:, i] - np.einsum("br,br->b", A[:, i], f) + A[:, i, i] * f[:, i]
                f[:, i] = np.where(active[:, i], np.maximum(res / den[:, i], 0.0), 0.0)
        qacc = qacc0.copy()
        qacc[idx] = a0 + (MinvJT @ f[:, :, None])[:, :, 0]
        act_all[idx] = active; f_all[idx] = f
        return qacc, act_all, f_all

    # ---------------------------------------------------------------- integrator
    def substep(self, q, v, ctrl):
        h = self.m["timestep"]
        a1, *_ = self.dynamics(q, v, ctrl)
        q2, v2 = q + 0.5 * h * v, v + 0.5 * h * a1
        a2, *_ = self.dynamics(q2, v2, ctrl)
        q3, v3 = q + 0.5 * h * v2, v + 0.5 * h * a2
        a3, *_ = self.dynamics(q3, v3, ctrl)
        q4, v4 = q + h * v3, v + h * a3
        a4, *_ = self.dynamics(q4, v4, ctrl)
        return q + h / 6.0 * (v + 2 * v2 + 2 * v3 + v4), v + h / 6.0 * (a1 + 2 * a2 + 2 * a3 + a4)

    # ---------------------------------------------------------------- task rules
    def ctrl(self, action):
        """NormalizedBoxEnv.step on float32 arrays (rlkit/envs/wrappers.py:342-346): lb + (a + 1.0) * 0.5 * (ub - lb), then np.clip."""
        lb, ub = np.float32(self.m["ctrl_range"][0]), np.float32(self.m["ctrl_range"][1])
        a = np.asarray(action, np.float32).reshape(-1, self.act_dim)
        scaled = lb + (a + np.float32(1.0)) * np.float32(0.5) * (ub - lb)
        assert scaled.dtype == np.float32
        return np.clip(scaled, lb, ub)

    def observe(self, q, v):
        return np.concatenate([q[:, 2:], v], 1).astype(np.float32)

    def step(self, q, v, action):
        """-> q', v', float32 observation, float64 reward"""
        q, v = np.array(q, np.float64), np.array(v, np.float64)
        c = self.ctrl(action).astype(np.float64)
        x0 = q[:, 0].copy()
        for _ in range(self.m["frame_skip"]):
            q, v = self.substep(q, v, c)
        reward = (q[:, 0] - x0) / (self.m["frame_skip"] * self.m["timestep"]) - 1e-4 * np.sum(c * c, 1)
        return q, v, self.observe(q, v), reward

    def reset(self, rng, B):
        """SwimmerEnv.reset_model: init + U(+-0.1) on qpos, U(+-0.1) on qvel."""
        init = np.asarray(self.m["init_qpos"], np.float64)
        return init + rng.uniform(-0.1, 0.1, (B, self.n)), rng.uniform(-0.1, 0.1, (B, self.n))

    # ---------------------------------------------------------------- conserved quantities (tests)
    def com(self, q):
        tot = sum(self.m["mass"])
        return sum(self.m["mass"][b] * k[2] for b, k in enumerate(self.kin(q, np.zeros_like(q)))) / tot

    def momenta(self, q, v):
        """Linear momentum [B, 2], angular momentum about the world origin [B], kinetic energy [B]; armature counts as rotor inertia
        turning with the joint rate, which carries energy but, on the hinges between links, no net momentum."""
        m = self.m
        P = np.zeros((q.shape[0], 2)); Lz = np.zeros(q.shape[0]); E = np.zeros(q.shape[0])
        for b, (Jc, _ac, c, _Jp, _phi, w) in enumerate(self.kin(q, v)):
            vc = np.einsum("bki,bi->bk", Jc, v)
            P += m["mass"][b] * vc
            Lz += m["mass"][b] * (c[:, 0] * vc[:, 1] - c[:, 1] * vc[:, 0]) + m["inertia"][b][2] * w
            E += 0.5 * m["mass"][b] * np.einsum("bk,bk->b", vc, vc) + 0.5 * m["inertia"][b][2] * w ** 2
        E += 0.5 * np.einsum("j,bj->b", np.asarray(m["armature"], np.float64), v ** 2)
        return P, Lz, E
