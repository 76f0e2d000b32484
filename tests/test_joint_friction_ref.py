"""The float64 joint-friction stepper (joint_friction64.py)
checked three ways before the GPU tests rely on it: against the closed
recurrence of a decoupled prismatic chain, against plain semi-implicit stepping
when every tau_f is 0, and for never raising the energy of an undriven
pendulum."""
import numpy as np

from isaacgym import gymapi

from dynamics64 import Dynamics
from joint_friction64 import FrictionStepper, hinge_chain_urdf, scalar_recurrence, total_energy, MODE_EFFORT, MODE_POS
from test_attractor_gpu import CART_URDF, CART_M

H = 1.0 / 120.0
G = 9.81


def _model(gym, tmp_path, name, urdf, gravity):
    (tmp_path / name).write_text(urdf)
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(*gravity)
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    sp.physx.num_position_iterations, sp.physx.num_velocity_iterations = 4, 1
    sp.use_gpu_pipeline = False
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.armature = 0.0
    asset = gym.load_asset(sim, str(tmp_path), name, opts)
    env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 1)
    h = gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 1)), "a", 0, 1)
    props = gym.get_actor_dof_properties(env, h)
    props["driveMode"][:] = gymapi.DOF_MODE_NONE
    for k in ("stiffness", "damping", "armature", "friction", "effort", "velocity"):
        props[k][:] = 0.0
    gym.set_actor_dof_properties(env, h, props)
    A = sim.build_model()
    return Dynamics(A, 0, gravity), A["body_state0"][0, 0:7].astype(np.float64)


def cart_recurrence(m_eff, C, tau0_fn, tau_f, q, u, n):
    qs, us = scalar_recurrence(H, m_eff, C, tau0_fn, tau_f, q, u, n)
    return qs, us[-1]


def test_cart_chain_equals_closed_recurrence(gym, tmp_path):
    dyn, base = _model(gym, tmp_path, "cart3.urdf", CART_URDF, (0.0, 0.0, -G))
    assert np.allclose(np.diag(dyn.mass_matrix(base, np.zeros(3))), CART_M)
    # x slides to a stop; y is pushed below its limit; z slides down against friction below m g
    tau_f = np.array([11.0, 4.0, 2.0])
    effort = np.array([0.0, 3.0, 0.0])
    st = FrictionStepper(dyn, H, 4, 1, tau_f, mode=MODE_EFFORT)
    qs, us, _ = st.run(base, np.zeros(3), np.array([1.0, 0.0, 0.0]), 240, effort=effort)
    C = np.array([0.0, 0.0, 0.5 * G])
    for d in range(3):
        ref, uend = cart_recurrence(CART_M[d], C[d], lambda q, u: effort[d], tau_f[d], 0.0, [1.0, 0.0, 0.0][d], 240)
        assert np.abs(qs[:, d] - ref).max() < 1e-12, d
        assert abs(us[-1, d] - uend) < 1e-12
    assert us[-1, 0] == 0.0 and 0.2 < qs[-1, 0] < 0.3          # stopped after v^2 m / (2 tau_f) = 0.25 m
    assert np.all(qs[:, 1] == 0.0)                              # stuck
    assert abs(us[-1, 2] + (0.5 * G - 2.0) / 0.5 * 2.0) < 1e-9  # (m g - tau_f) / m for 2 s
    # a POS drive: m_eff = m + h kd + h^2 kp, and it parks inside the dead band
    kp, kd, tgt = 400.0, 10.0, 0.05
    st = FrictionStepper(dyn, H, 4, 1, [6.0, 0.0, 0.0], mode=[MODE_POS, 0, 0], kp=kp, kd=kd)
    z = np.zeros(3)
    hold = np.array([0.0, 0.0, 0.5 * G])                        # carries z, so the chain stays put
    st.mode[2] = MODE_EFFORT
    qs, us, _ = st.run(base, z, z, 480, tpos=np.array([tgt, 0.0, 0.0]), effort=hold)
    ref, _ = cart_recurrence(CART_M[0] + H * kd + H * H * kp, 0.0,
                             lambda q, u: kp * (tgt - q - H * u) + kd * (0.0 - u), 6.0, 0.0, 0.0, 480)
    assert np.abs(qs[:, 0] - ref).max() < 1e-12
    assert us[-1, 0] == 0.0 and 0.0 < abs(tgt - qs[-1, 0]) <= 6.0 / kp


def test_zero_friction_is_plain_semi_implicit_stepping(gym, tmp_path):
    dyn, base = _model(gym, tmp_path, "hinge3.urdf", hinge_chain_urdf(3), (0.0, 0.0, -G))
    st = FrictionStepper(dyn, H, 4, 1, 0.0, mode=MODE_EFFORT)
    tau = np.array([0.3, -0.2, 0.1])
    q, u = np.array([0.4, -0.7, 1.1]), np.array([1.0, -2.0, 0.5])
    b2, q2, u2 = base, q.copy(), u.copy()
    for _ in range(60):
        _, q, u, lam = st.substep(base, q, u, effort=tau)
        b2, q2, u2, _ = dyn.step(b2, q2, u2, tau, H)
        assert np.all(lam == 0.0)
        assert np.abs(q - q2).max() < 1e-12 and np.abs(u - u2).max() < 1e-12
    assert np.abs(u).max() > 1.0


def test_friction_never_raises_the_energy(gym, tmp_path):
    dyn, base = _model(gym, tmp_path, "hinge2.urdf", hinge_chain_urdf(2), (0.0, 0.0, -G))
    st = FrictionStepper(dyn, H, 4, 1, [0.25, 0.12])
    q, u = np.array([1.4, -0.6]), np.array([0.5, 3.0])
    E = [total_energy(dyn, base, q, u)]
    for _ in range(480):
        _, q, u, _ = st.substep(base, q, u)
        E.append(total_energy(dyn, base, q, u))
    E = np.array(E)
    print("energy %.6f -> %.6f J, largest rise %.3g J" % (E[0], E[-1], np.diff(E).max()))
    assert np.diff(E).max() <= 0.0
    # it came to rest held by friction (coupled rows: five sweeps leave a Gauss-Seidel residual, not 0)
    assert E[-1] < E[0] - 0.5 and np.abs(u).max() < 1e-3
