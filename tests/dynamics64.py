"""float64 reference forward dynamics for articulations (test helper).

The principle of virtual power on top of kinematics64 — no spatial algebra, no
recursion, nothing shared with the engine's ABA / RNEA / CRBA code. For the
generalized velocities u (the DOF rates; for a floating base preceded by the
root's linear velocity at the base-link origin and its world angular velocity)

    bias(q, u) = sum_links Jv^T m (a - g) + Jw^T (I_w alpha + w x I_w w) - sum J^T (external wrenches)
    a, alpha   = (J u)' at fixed u: a central difference of Jv(q(t)) u, Jw(q(t)) u along the flow q' = u
    qdd        = solve(M(q) + diag(armature), tau - bias)

Jv, Jw are the rows of a link's COM Jacobian (kinematics64.point_jacobian[_fb]),
M its mass matrix. A ball joint's three rates are quasi-velocities (the child's
angular velocity in the child frame), for which the virtual-power form holds as
it stands; its flow is th <- log(exp(th) exp(eps w)), a floating root's
p <- p + eps v, quat <- exp(eps w) (x) quat.

Reads the packed model arrays of Sim.build_model (mg_model, include/migym.h).
"""
import numpy as np

from kinematics64 import Articulation, qmul, qmat

EPS = 1e-6      # flow step of the central difference (test_dynamics_kat.py: halving it moves qdd < 1e-8 relative)


def qexp(v):
    """Unit quaternion (xyzw) of the rotation vector v."""
    v = np.asarray(v, np.float64)
    t = np.linalg.norm(v)
    if t < 1e-12:
        q = np.array([*(0.5 * v), 1.0])
        return q / np.linalg.norm(q)
    return np.array([*(v / t * np.sin(0.5 * t)), np.cos(0.5 * t)])


def qlog(q):
    """Rotation vector of a unit quaternion, angle in [0, pi]."""
    q = np.asarray(q, np.float64)
    if q[3] < 0:
        q = -q
    s = np.linalg.norm(q[0:3])
    if s < 1e-12:
        return 2.0 * q[0:3]
    return q[0:3] / s * (2.0 * np.arctan2(s, q[3]))


class Dynamics:
    """Forward dynamics of one articulation instance of a packed model.

    A: the model arrays; artic: its row of A["artic_i"]; gravity: world (3,)."""

    def __init__(self, A, artic=0, gravity=(0.0, 0.0, 0.0)):
        fb, fd, tmpl = (int(x) for x in A["artic_i"][artic][0:3])
        self.A, self.first_body, self.first_dof = A, fb, fd
        self.art = Articulation(A, tmpl)
        self.D = self.art.D
        self.floating = int(A["artic_tmpl_i"][tmpl][3]) == 0
        self.nu = self.D + (6 if self.floating else 0)
        self.g = np.asarray(gravity, np.float64)
        li, lf = self.art.li, self.art.lf
        # first DOF of every ball joint (its links are marked 1, 2, 3 in tmpl_link_f[10])
        self.balls = [int(li[l, 2]) for l in range(self.art.L) if int(round(lf[l, 10])) == 1]
        self.armature = A["dof_props"][fd:fd + self.D, 8].astype(np.float64)
        self.links = []             # (link, mass, com, principal frame, principal inertia, gravity on)
        for l, b in (self.art.bodies() if self.floating else self.art.bodies()[1:]):
            row = A["body_mass"][fb + b].astype(np.float64)
            Ip = np.array([1.0 / x if x > 0 else 0.0 for x in row[1:4]])
            gon = float(A["tmpl_body_f"][int(A["body_tmpl"][fb + b]), 4])
            self.links.append((l, b, row[11], row[8:11], qmat(row[4:8]), Ip, gon))

    # ------------------------------------------------------------ kinematics
    def _jac(self, ps, zs, l, pt):
        return self.art.point_jacobian_fb(ps, zs, l, pt) if self.floating else self.art.point_jacobian(ps, zs, l, pt)

    def mass_matrix(self, base, q):
        M = (self.art.mass_matrix_fb if self.floating else self.art.mass_matrix)(base, q, self.first_body)
        M = M.copy()
        off = self.nu - self.D
        M[off:, off:] += np.diag(self.armature)
        return M

    def flow(self, base, q, u, eps):
        """(base pose, q) moved for a time eps at the constant generalized velocity u."""
        base = np.array(base[0:7], np.float64)
        q = np.array(q, np.float64)
        ud = u[self.nu - self.D:]
        qn = q + eps * ud
        for d in self.balls:
            qn[d:d + 3] = qlog(qmul(qexp(q[d:d + 3]), qexp(eps * ud[d:d + 3])))
        if self.floating:
            base[0:3] += eps * u[0:3]
            base[3:7] = qmul(qexp(eps * u[3:6]), base[3:7])
            base[3:7] /= np.linalg.norm(base[3:7])
        return base, qn

    def _link_velocities(self, base, q, u):
        """(n_links, 6): COM velocity and angular velocity of every massive link."""
        ps, Rs, zs = self.art.fk(base, q)
        return np.stack([self._jac(ps, zs, l, ps[l] + Rs[l] @ com) @ u for l, _, _, com, _, _, _ in self.links])

    # -------------------------------------------------------------- dynamics
    def bias(self, base, q, u, ext=None, ext_at=None, eps=EPS, gravity=None, omit=()):
        """Generalized bias force. ext: {local body: (F, T)} world wrench, F at the
        COM; ext_at: {local body: (F, world point)}. omit: names of terms left out
        ("Jdot_u", "gyro") — for a test to show that it would notice."""
        g = self.g if gravity is None else np.asarray(gravity, np.float64)
        u = np.asarray(u, np.float64)
        vp = self._link_velocities(*self.flow(base, q, u, eps), u)
        vm = self._link_velocities(*self.flow(base, q, u, -eps), u)
        acc = (vp - vm) / (2.0 * eps)
        if "Jdot_u" in omit:
            acc = np.zeros_like(acc)
        ps, Rs, zs = self.art.fk(base, q)
        out = np.zeros(self.nu)
        for k, (l, b, m, com, Rp, Ip, gon) in enumerate(self.links):
            c = ps[l] + Rs[l] @ com
            J = self._jac(ps, zs, l, c)
            Rl = Rs[l] @ Rp
            Iw = Rl @ np.diag(Ip) @ Rl.T
            w = J[3:6] @ u
            gyro = np.zeros(3) if "gyro" in omit else np.cross(w, Iw @ w)
            out += J[0:3].T @ (m * (acc[k, 0:3] - gon * g)) + J[3:6].T @ (Iw @ acc[k, 3:6] + gyro)
            if ext is not None and b in ext:
                F, T = (np.asarray(x, np.float64) for x in ext[b])
                out -= J[0:3].T @ F + J[3:6].T @ T
            if ext_at is not None and b in ext_at:
                F, pt = (np.asarray(x, np.float64) for x in ext_at[b])
                out -= self._jac(ps, zs, l, pt)[0:3].T @ F
        return out

    def qdd(self, base, q, u, tau, **kw):
        """Generalized accelerations (nu,); tau (D,) the DOF efforts (root rows get 0)."""
        rhs = -self.bias(base, q, u, **kw)
        rhs[self.nu - self.D:] += np.asarray(tau, np.float64)
        return np.linalg.solve(self.mass_matrix(base, q), rhs)

    def step(self, base, q, u, tau, h, **kw):
        """One semi-implicit Euler step: u' = u + h qdd(q, u), then the flow of u'
        for h. Returns (base', q', u', qdd)."""
        u = np.asarray(u, np.float64)
        a = self.qdd(base, q, u, tau, **kw)
        un = u + h * a
        base, qn = self.flow(base, q, un, h)
        return base, qn, un, a
