"""float64 restatement of the force sensor's definition (test
helper), from public tensors only: the rigid-body state before and after one
step, get_actor_rigid_body_properties, the applied wrenches, the net contact
force (and, where a test has one, a contact moment), with the subtrees walked
by kinematics64.Articulation's link table.

Per body k of the sensor body's subtree, wrenches about k's COM:
    N_k = (m (v+ - v-) / dt, (I_w+ w+ - I_w- w-) / dt),  I_w = R I_body R^T
    G_k = (m g, 0)          E_k = the applied wrench          C_k = the contact wrench
    J   = sum_k (F_k, T_k + (c_k+ - o_s) x F_k),  (F_k, T_k) = N_k - G_k - E_k - C_k
about the sensor origin o_s at the end of the frame, rotated into the sensor
frame unless use_world_frame. Forward-dynamics part: N - G - E; constraint
part: -C.

Beside each reading the functions return S, the sum of the magnitudes of every
term that enters it (the lever arms' own terms multiply the force terms in the
torque rows): the scale of the recursive-summation bound K 2^-23 S.
"""
import numpy as np

from kinematics64 import qmat, qmul


def rounding_count(nbodies):
    """K: fp32 roundings on k_force_sensor's longest dependency chain for a
    subtree of `nbodies` bodies, counted from csrc/mg_sensor.hip (u = 2^-24
    each, so K 2^-23 bounds twice the first-order sum):
      angular momentum R diag(I_p) R^T w: the mass row's I_p = 1 / fl(1 / I)
        (2) and its principal frame in fp32, applied twice (4); qmul (4) and
        qmat (3), applied twice with the rotation's doubling (2 x 11);
        mtmul (3), the product (1), mmul (3)                              -> 35
      N_k: the difference (1), 1 / dt and dt in fp32 (2), the product (1) ->  4
      - E_k (1), the lever arm (x + R com) - (x_s + R_s p_s) (10), the
        cross product (2), T_k + r x F_k (1)                              -> 14
      the subtree's sum, two additions per body                           -> 2 n
      forward + constraint part (1); into the sensor frame: the host's
        normalised local rotation (3), qmul (4, doubled: 8), qrot (7)     -> 19
    The force rows' chain is shorter (m v: 2, N_k: 4, G_k: 3, E_k: 1, n, 19)."""
    return 72 + 2 * nbodies


def subtree(art, body):
    """Local bodies of the subtree of local body `body`, in link order
    (virtual links pass the subtree through)."""
    link = [l for l, b in art.bodies() if b == body][0]
    inside = {link}
    out = []
    for l in range(link, art.L):
        if l != link and int(art.li[l, 0]) in inside:
            inside.add(l)
        if l in inside and int(art.li[l, 3]) >= 0:
            out.append(int(art.li[l, 3]))
    return out


def body_props(props):
    """(mass, com[3], inertia[3][3]) in float64 from RigidBodyProperties."""
    out = []
    for p in props:
        I = np.array([[p.inertia.x.x, p.inertia.x.y, p.inertia.x.z],
                      [p.inertia.y.x, p.inertia.y.y, p.inertia.y.z],
                      [p.inertia.z.x, p.inertia.z.y, p.inertia.z.z]], np.float64)
        out.append((float(p.mass), np.array([p.com.x, p.com.y, p.com.z], np.float64), I))
    return out


def _qrot(q, v):
    return qmat(np.asarray(q, np.float64) / np.linalg.norm(q)) @ v


def reading(bodies, props, rb0, rb1, dt, gravity, pose_p, pose_q, sensor_body,
            ext_f=None, ext_t=None, cf=None, ct=None, fd=True, cs=True, world=False):
    """The reading of one sensor. bodies: the subtree's local bodies (subtree());
    props: body_props of the actor; rb0 / rb1: the actor's (nb, 13) rigid-body
    rows before / after the step; gravity: (3,) or None for a gravity-free
    asset; ext_f / ext_t / cf / ct: (nb, 3) applied force / torque, net contact
    force / contact moment about the COM (None: zero). Returns (F, T, S_F, S_T)."""
    rb0 = np.asarray(rb0, np.float64)
    rb1 = np.asarray(rb1, np.float64)
    nb = rb1.shape[0]
    z = np.zeros((nb, 3))
    ext_f = z if ext_f is None else np.asarray(ext_f, np.float64)
    ext_t = z if ext_t is None else np.asarray(ext_t, np.float64)
    cf = z if cf is None else np.asarray(cf, np.float64)
    ct = z if ct is None else np.asarray(ct, np.float64)
    g = np.zeros(3) if gravity is None else np.asarray(gravity, np.float64)
    pose_p = np.asarray(pose_p, np.float64)
    xs, qs = rb1[sensor_body, 0:3], rb1[sensor_body, 3:7]
    o_s = xs + _qrot(qs, pose_p)
    Ff, Tf, Fc, Tc = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    SF = ST = 0.0
    norm = np.linalg.norm
    for k in bodies:
        m, com, I = props[k]
        R0, R1 = qmat(rb0[k, 3:7] / norm(rb0[k, 3:7])), qmat(rb1[k, 3:7] / norm(rb1[k, 3:7]))
        p0, p1 = m * rb0[k, 7:10], m * rb1[k, 7:10]
        L0, L1 = R0 @ I @ R0.T @ rb0[k, 10:13], R1 @ I @ R1.T @ rb1[k, 10:13]
        F = (p1 - p0) / dt - m * g - ext_f[k]
        T = (L1 - L0) / dt - ext_t[k]
        r = rb1[k, 0:3] + R1 @ com - o_s
        Ff += F
        Tf += T + np.cross(r, F)
        Fc -= cf[k]
        Tc -= ct[k] + np.cross(r, cf[k])
        sF_fd = (norm(p1) + norm(p0)) / dt + m * norm(g) + norm(ext_f[k])
        sF_cs = norm(cf[k])
        lever = norm(rb1[k, 0:3]) + norm(com) + norm(xs) + norm(pose_p)
        sT_fd = (norm(L1) + norm(L0)) / dt + norm(ext_t[k]) + lever * sF_fd
        sT_cs = norm(ct[k]) + lever * sF_cs
        SF += (sF_fd if fd else 0.0) + (sF_cs if cs else 0.0)
        ST += (sT_fd if fd else 0.0) + (sT_cs if cs else 0.0)
    F = (Ff if fd else 0.0) + (Fc if cs else 0.0)
    T = (Tf if fd else 0.0) + (Tc if cs else 0.0)
    F, T = np.asarray(F, np.float64) * np.ones(3), np.asarray(T, np.float64) * np.ones(3)
    if not world:
        qw = qmul(qs / norm(qs), np.asarray(pose_q, np.float64) / norm(pose_q))
        Rw = qmat(qw / norm(qw))
        F, T = Rw.T @ F, Rw.T @ T
    return F, T, SF, ST
