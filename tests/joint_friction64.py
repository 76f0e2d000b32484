"""float64 reference stepper for joint friction (test helper).

One substep of an articulation with revolute and prismatic DOFs, on
dynamics64.Dynamics (its mass matrix and bias; nothing shared with the engine):

  1. u* = u + h (M + diag(armature + imp))^-1 (tau0 - bias), the implicit drives
     of §3.3: POS tau0 = kp (q* - q - h u) + kd (u* - u), imp = h kd + h^2 kp;
     VEL tau0 = kd (u* - u), imp = h kd; EFFORT tau0 = the effort; NONE 0.
  2. one row per DOF with tau_f > 0: Jacobian the unit vector of its slot,
     response that column of M_eff^-1,
         lam_d <- clamp(lam_d + (0 - u_d) / (M_eff^-1)_dd, +-h tau_f),
         u += M_eff^-1[:, d] dlam.
  3. npos + nvel Gauss-Seidel sweeps over the rows in DOF order, lam from 0,
     dpos += u h / npos after each of the first npos; q' = q + dpos (a floating
     root moves by its slots of dpos).

No effort limits, speed limits or joint limits: the scenes that use it stay
clear of them.
"""
import numpy as np

MODE_NONE, MODE_POS, MODE_VEL, MODE_EFFORT = 0, 1, 2, 3


def hinge_chain_urdf(n, length=0.25, mass=0.4):
    """A fixed base and n hinged rods in series, axes alternating between y and a
    skew axis, COM half-way along each rod (which hangs along -z at q = 0),
    masses falling off along the chain: a pendulum whose DOFs are coupled
    through the mass matrix. Continuous joints: no limit rows."""
    out = ['<robot name="hinge%d"><link name="base"/>' % n]
    for k in range(n):
        m = mass * (0.85 ** k)
        i = m * length * length / 12.0
        out.append('<link name="r%d"><inertial><origin xyz="0 0 %g"/><mass value="%g"/><inertia ixx="%g" iyy="%g" '
                   'izz="%g" ixy="0" ixz="0" iyz="0"/></inertial></link>' % (k, -0.5 * length, m, i, i, 0.1 * i))
        out.append('<joint name="h%d" type="continuous"><parent link="%s"/><child link="r%d"/><origin xyz="0 0 %g"/>'
                   '<axis xyz="%s"/></joint>' % (k, "base" if k == 0 else "r%d" % (k - 1), k,
                                               0.0 if k == 0 else -length, "0 1 0" if k % 2 == 0 else "0.6 0.8 0"))
    out.append("</robot>")
    return "".join(out)


class FrictionStepper:
    """dyn: a dynamics64.Dynamics; h: the substep; tau_f (D,): Coulomb limits."""

    def __init__(self, dyn, h, npos, nvel, tau_f, mode=None, kp=None, kd=None):
        D = dyn.D
        self.dyn, self.h, self.npos, self.nvel = dyn, float(h), int(npos), int(nvel)
        self.tau_f = np.zeros(D) + np.asarray(tau_f, np.float64)
        self.mode = np.zeros(D, int) + (MODE_NONE if mode is None else np.asarray(mode, int))
        self.kp = np.zeros(D) + (0.0 if kp is None else np.asarray(kp, np.float64))
        self.kd = np.zeros(D) + (0.0 if kd is None else np.asarray(kd, np.float64))

    def drive(self, q, ud, tpos, tvel, effort):
        """(tau0, imp) of the DOFs, §3.3."""
        h = self.h
        tau0, imp = np.zeros(self.dyn.D), np.zeros(self.dyn.D)
        for d in range(self.dyn.D):
            if self.mode[d] == MODE_POS:
                tau0[d] = self.kp[d] * (tpos[d] - q[d] - h * ud[d]) + self.kd[d] * (tvel[d] - ud[d])
                imp[d] = h * self.kd[d] + h * h * self.kp[d]
            elif self.mode[d] == MODE_VEL:
                tau0[d] = self.kd[d] * (tvel[d] - ud[d])
                imp[d] = h * self.kd[d]
            elif self.mode[d] == MODE_EFFORT:
                tau0[d] = effort[d]
        return tau0, imp

    def substep(self, base, q, u, tpos=None, tvel=None, effort=None):
        """(base', q', u', lam): one substep from (base, q, u); u in Dynamics'
        order (a floating root's six slots first, then the DOFs)."""
        dyn, h, D = self.dyn, self.h, self.dyn.D
        off = dyn.nu - D
        z = np.zeros(D)
        q, u = np.array(q, np.float64), np.array(u, np.float64)
        tau0, imp = self.drive(q, u[off:], z if tpos is None else tpos, z if tvel is None else tvel,
                               z if effort is None else effort)
        Meff = dyn.mass_matrix(base, q)
        Meff[off:, off:] += np.diag(imp)
        rhs = -dyn.bias(base, q, u)
        rhs[off:] += tau0
        u = u + h * np.linalg.solve(Meff, rhs)
        Minv = np.linalg.inv(Meff)
        lam = np.zeros(D)
        dpos = np.zeros(dyn.nu)
        sub = h / self.npos
        for it in range(self.npos + self.nvel):
            for d in range(D):
                if self.tau_f[d] <= 0.0:
                    continue
                s = off + d
                lim = h * self.tau_f[d]
                new = min(max(lam[d] + (0.0 - u[s]) / Minv[s, s], -lim), lim)
                u = u + Minv[:, s] * (new - lam[d])
                lam[d] = new
            if it < self.npos:
                dpos = dpos + u * sub
        base, q = dyn.flow(base, q, dpos, 1.0)
        return base, q, u, lam

    def run(self, base, q, u, substeps, **kw):
        """States after each substep: arrays (substeps, D) of q and (substeps, nu) of u."""
        qs, us = [], []
        for _ in range(substeps):
            base, q, u, _ = self.substep(base, q, u, **kw)
            qs.append(q.copy())
            us.append(u.copy())
        return np.array(qs), np.array(us), base


def scalar_recurrence(h, m_eff, C, tau0_fn, tau_f, q, u, n):
    """The closed recurrence of one decoupled DOF over n substeps,
        u* = u + h (tau0 - C) / m_eff; lam = clamp(-m_eff u*, +-h tau_f);
        u+ = u* + lam / m_eff; q+ = q + h u+.
    tau0_fn(q, u): the drive's tau0 (m_eff includes its h kd + h^2 kp).
    Returns (q after each substep, u after each substep)."""
    qs, us = [], []
    for _ in range(n):
        ustar = u + h * (tau0_fn(q, u) - C) / m_eff
        lam = min(max(-m_eff * ustar, -h * tau_f), h * tau_f)
        u = ustar + lam / m_eff
        q = q + h * u
        qs.append(q)
        us.append(u)
    return np.array(qs), np.array(us)


def total_energy(dyn, base, q, u):
    """Kinetic plus gravitational energy of the massive links (armature has none
    here: the scenes that ask for energy use armature 0)."""
    ps, Rs, zs = dyn.art.fk(base, q)
    u = np.asarray(u, np.float64)
    E = 0.0
    for l, b, m, com, Rp, Ip, gon in dyn.links:
        c = ps[l] + Rs[l] @ com
        J = dyn._jac(ps, zs, l, c)
        v, w = J[0:3] @ u, J[3:6] @ u
        Rl = Rs[l] @ Rp
        E += 0.5 * m * v @ v + 0.5 * w @ (Rl @ np.diag(Ip) @ Rl.T) @ w - gon * m * (dyn.g @ c)
    return E
