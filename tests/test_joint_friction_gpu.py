"""Joint friction on the GPU: the DOF `friction` property as
an implicit Coulomb row per DOF in the joint-friction builds of k_artic_lanes
and k_env_step. Every scene asserts mg_joint_friction_stats, so the intended
kernel is the one that ran.

All scenes: dt 1/60, 2 substeps (h = 1/120), 4 position and 1 velocity sweeps.

1. the three-prismatic chain against the closed scalar recurrence, tolerance
   2e-5 m + 1e-4 |displacement| (the attractor tests' bound);
2. hinge chains (2, 6, 18 hinges: the 4-link, 16-link and wide builds) against
   the float64 stepper of joint_friction64.py; the tolerance is 4x the error the
   same scene shows with tau_f = 0, the friction-free kernels' own distance
   from the stepper, measured in the same test;
3. the third law on a floating two-box hinge: momentum drift within 4x that of
   the tau_f = 0 run;
4. refusals and re-routing.

Measured on an MI355X (DESIGN.md §3.15 has the table): max |q - float64| with
friction / without, uncoupled: 2 hinges 2.5e-7 / 4.5e-7 rad, 6 hinges 1.2e-6 /
1.7e-6, 18 hinges 3.1e-6 / 5.1e-6; momentum drift over 120 frames with friction
/ without: P 0.011 / 0.020 kg m/s, L 0.0019 / 0.0034 kg m^2/s.
"""
import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N

from dynamics64 import Dynamics
from joint_friction64 import FrictionStepper, hinge_chain_urdf, scalar_recurrence
from test_attractor_gpu import CART_URDF, CART_M, CART_POSE, attractor, close, sim_params

pytestmark = pytest.mark.gpu

H = 1.0 / 120.0
G = 9.81
FRAMES = 120


def stats(sim):
    """(friction DOFs, instances in the lanes friction launch, envs of coupled friction groups)"""
    out = sim.joint_friction_stats()
    if out[0]:
        assert N.lib.mg_step_out_supported(sim.native) == 0
    return out


def far_box(gym, sim):
    bopts = gymapi.AssetOptions()
    bopts.fix_base_link = True
    return gym.create_box(sim, 0.1, 0.1, 0.1, bopts)


def add_far_box(gym, env, box, group):
    bpose = gymapi.Transform()
    bpose.p = gymapi.Vec3(0.0, 0.0, -5.0)
    gym.create_actor(env, box, bpose, "box", group, 0)


def run(gym, sim, frames, effort=None):
    """DOF positions and velocities after each frame [frames, nd], last rigid-body state."""
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    eff = None if effort is None else torch.tensor(effort, dtype=torch.float32, device="cuda:0")
    pos, vel = [], []
    for _ in range(frames):
        if eff is not None:
            assert gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(eff))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_dof_state_tensor(sim)
        d = dof.cpu().numpy()
        pos.append(d[:, 0].copy())
        vel.append(d[:, 1].copy())
    gym.refresh_rigid_body_state_tensor(sim)
    return np.array(pos), np.array(vel), rb.cpu().numpy().copy()


# ----------------------------------------------------------------- 1. cart chain
# env -> per-DOF (x, y, z) friction; the other envs carry none
CART_FRIC = {1: (11.0, 4.0, 6.0), 3: (6.0, 0.0, 2.0)}
KP, KD, TGT = 400.0, 10.0, 0.05          # env 3's POS drive on x
Y_PUSH = 3.0                             # effort on y, below env 1's 4 N
X_V0 = 1.0


def cart_scene(gym, tmp_path, fric, coupled, num_envs=5):
    """The attractor tests' three-prismatic chain (no ground, gravity on z). Every
    env: y in EFFORT mode; x starts at 1 m/s, except env 3 whose x is a POS
    drive towards 0.05 m from rest. coupled: a fixed box 5 m away in the chain's
    collision group makes each env a coupled one."""
    (tmp_path / "cart3.urdf").write_text(CART_URDF)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.armature = 0.0
    asset = gym.load_asset(sim, str(tmp_path), "cart3.urdf", opts)
    box = far_box(gym, sim) if coupled else None
    handles = []
    for i in range(num_envs):
        env = gym.create_env(sim, gymapi.Vec3(-1.0, -1.0, 0.0), gymapi.Vec3(1.0, 1.0, 2.0), 3)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(*CART_POSE)
        h = gym.create_actor(env, asset, pose, "cart", i, 0 if coupled else 1)
        if coupled:
            add_far_box(gym, env, box, i)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = (gymapi.DOF_MODE_NONE, gymapi.DOF_MODE_EFFORT, gymapi.DOF_MODE_NONE)
        for k in ("stiffness", "damping", "armature", "friction"):
            props[k][:] = 0.0
        props["velocity"][:] = 100.0
        props["lower"][:], props["upper"][:] = -100.0, 100.0
        if i == 3:
            props["driveMode"][0], props["stiffness"][0], props["damping"][0] = gymapi.DOF_MODE_POS, KP, KD
        props["friction"][:] = fric.get(i, (0.0, 0.0, 0.0))
        gym.set_actor_dof_properties(env, h, props)
        if i == 3:
            tg = np.array([TGT, 0.0, 0.0], dtype=np.float32)
            gym.set_actor_dof_position_targets(env, h, tg)
        else:
            st = gym.get_actor_dof_states(env, h, gymapi.STATE_ALL)
            st["vel"][0] = X_V0
            gym.set_actor_dof_states(env, h, st, gymapi.STATE_ALL)
        handles.append((env, h))
    gym.prepare_sim(sim)
    return sim, handles


def cart_effort(num_envs=5):
    e = np.zeros((num_envs, 3), dtype=np.float32)
    e[:, 1] = Y_PUSH
    return e.reshape(-1)


def cart_reference(e, fric, frames):
    """Per-frame (q, u) [frames, 3] of env e by the closed recurrence."""
    n = 2 * frames
    f = fric.get(e, (0.0, 0.0, 0.0))
    if e == 3:
        qx, ux = scalar_recurrence(H, CART_M[0] + H * KD + H * H * KP, 0.0,
                                   lambda q, u: KP * (TGT - q - H * u) + KD * (0.0 - u), f[0], 0.0, 0.0, n)
    else:
        qx, ux = scalar_recurrence(H, CART_M[0], 0.0, lambda q, u: 0.0, f[0], 0.0, X_V0, n)
    qy, uy = scalar_recurrence(H, CART_M[1], 0.0, lambda q, u: Y_PUSH, f[1], 0.0, 0.0, n)
    qz, uz = scalar_recurrence(H, CART_M[2], CART_M[2] * G, lambda q, u: 0.0, f[2], 0.0, 0.0, n)
    return np.stack([qx, qy, qz], 1)[1::2], np.stack([ux, uy, uz], 1)[1::2]


@pytest.fixture(scope="module", params=[False, True], ids=["uncoupled", "coupled"])
def cart_runs(request, tmp_path_factory):
    """(coupled, the friction run, the friction-free run) of the 5-env scene, shared."""
    gym = gymapi.acquire_gym()
    coupled = request.param
    out = []
    for fric in (CART_FRIC, {}):
        sim, _ = cart_scene(gym, tmp_path_factory.mktemp("cart"), fric, coupled)
        st = stats(sim)
        if fric:
            # friction DOFs 3 + 2; the lanes launch takes the two instances out of the chain group,
            # the coupled group moves to the friction build as a whole
            assert st == ((5, 0, 5) if coupled else (5, 2, 0)), st
            assert N.lib.mg_step_out_supported(sim.native) == 0
        else:
            assert st == (0, 0, 0), st
        out.append(run(gym, sim, FRAMES, effort=cart_effort()))
        gym.destroy_sim(sim)
    return coupled, out[0], out[1]


def test_cart_x_stops_in_the_recurrence_frame(cart_runs):
    """x starts at 1 m/s against 11 N on 5.5 kg: it stops after 0.5 s, in the frame
    the recurrence says, and stays. Fails without the feature (the joint slides on)."""
    _, (pos, vel, _), _ = cart_runs
    q, u = cart_reference(1, CART_FRIC, FRAMES)
    stop = int(np.argmax(u[:, 0] == 0.0))
    assert 25 <= stop <= 35 and u[stop - 1, 0] > 0.0
    gq, gu = pos[:, 3], vel[:, 3]
    print("x stops in frame %d at %.6f m (recurrence %.6f m), |u| after %.3g" % (stop, gq[stop], q[stop, 0],
                                                                               np.abs(gu[stop:]).max()))
    assert gu[stop - 1] > 1e-3 and np.all(np.abs(gu[stop:]) <= 1e-6 * X_V0)
    assert np.abs(gq[stop:stop + 61] - gq[stop]).max() < 1e-6
    err, tol = close(gq, q[:, 0])
    assert (err <= tol).all(), "max error %g m" % err.max()


def test_cart_follows_recurrence(cart_runs):
    """Every DOF of the two friction envs: y pushed below tau_f does not move, z
    holds 0.5 kg against gravity under 6 N and slides at (m g - tau_f) / m under
    2 N, the POS drive parks inside its dead band, the frictionless y of env 3
    accelerates freely."""
    _, (pos, vel, _), _ = cart_runs
    for e in (1, 3):
        q, u = cart_reference(e, CART_FRIC, FRAMES)
        err, tol = close(pos[:, 3 * e:3 * e + 3], q)
        print("env %d: max err %s m, max |q| %s" % (e, err.max(0), np.abs(q).max(0)))
        assert (err <= tol).all(), "env %d: max error %g m over the bound by %g" % (e, err.max(), (err - tol).max())
    # y of env 1 (3 N against 4 N) and z of env 1 (4.905 N against 6 N) never move
    assert np.abs(pos[:, 4]).max() < 1e-6 and np.abs(vel[:, 4]).max() <= 1e-6 * (H * Y_PUSH / CART_M[1])
    assert np.abs(pos[:, 5]).max() < 1e-6 and np.abs(vel[:, 5]).max() <= 1e-6 * (H * G)
    # z of env 3 slides at (m g - tau_f) / m
    acc = (CART_M[2] * G - 2.0) / CART_M[2]
    assert abs(vel[-1, 11] + acc * FRAMES / 60.0) < 1e-3 * acc * FRAMES / 60.0
    # the POS drive came to rest inside the dead band |q* - q| <= tau_f / kp, off the target
    rest = pos[-1, 9]
    assert abs(vel[-1, 9]) <= 1e-6 and 1e-4 < abs(TGT - rest) <= 6.0 / KP
    assert np.abs(pos[-61:, 9] - rest).max() < 1e-6


def test_cart_frictionless_envs_keep_their_bits(cart_runs):
    """Envs 0, 2 and 4 carry no friction: bit for bit the friction-free sim,
    whichever kernel stepped them."""
    _, (pos, vel, rb), (ppos, pvel, prb) = cart_runs
    nbe = rb.shape[0] // 5
    for e in (0, 2, 4):
        assert np.array_equal(pos[:, 3 * e:3 * e + 3], ppos[:, 3 * e:3 * e + 3])
        assert np.array_equal(vel[:, 3 * e:3 * e + 3], pvel[:, 3 * e:3 * e + 3])
        assert np.array_equal(rb[nbe * e:nbe * (e + 1)], prb[nbe * e:nbe * (e + 1)])
    assert not np.array_equal(pos[:, 3:6], ppos[:, 3:6])


# ------------------------------------------------------ 2. coupled DOFs, float64
HINGE_FRAMES = 60
# hinges -> (envs, tau_f per hinge, expected build); friction on alternate hinges of the 6-chain
HINGES = {
    2: (5, np.array([0.25, 0.12])),
    6: (5, np.array([0.6, 0.0, 0.3, 0.0, 0.08, 0.0])),
    18: (2, 0.2 * 0.9 ** np.arange(18)),
}
ARMATURE = 0.005


def hinge_init(n):
    k = np.arange(n)
    return 0.35 * np.cos(1.3 * k + 0.4), 1.5 * np.sin(0.9 * k + 1.0)


def hinge_scene(gym, tmp_path, n, tau_f, coupled):
    name = "hinge%d.urdf" % n
    (tmp_path / name).write_text(hinge_chain_urdf(n))
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.armature = 0.0
    asset = gym.load_asset(sim, str(tmp_path), name, opts)
    box = far_box(gym, sim) if coupled else None
    q0, u0 = hinge_init(n)
    for i in range(HINGES[n][0]):
        env = gym.create_env(sim, gymapi.Vec3(-1.0, -1.0, 0.0), gymapi.Vec3(1.0, 1.0, 2.0), 3)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 0.0, 6.0)
        h = gym.create_actor(env, asset, pose, "chain", i, 0 if coupled else 1)
        if coupled:
            add_far_box(gym, env, box, i)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_NONE
        for k in ("stiffness", "damping", "effort", "velocity"):
            props[k][:] = 0.0
        props["armature"][:] = ARMATURE
        props["friction"][:] = tau_f
        gym.set_actor_dof_properties(env, h, props)
        st = gym.get_actor_dof_states(env, h, gymapi.STATE_ALL)
        st["pos"][:], st["vel"][:] = q0, u0
        gym.set_actor_dof_states(env, h, st, gymapi.STATE_ALL)
    gym.prepare_sim(sim)
    return sim


_HINGE_REF = {}


def hinge_reference(A, n, tau_f):
    """Per-frame q [frames, n] of the float64 stepper, computed once per scene."""
    key = (n, bool(np.any(tau_f > 0)))
    if key not in _HINGE_REF:
        dyn = Dynamics(A, 0, (0.0, 0.0, -G))
        base = A["body_state0"][int(A["artic_i"][0][0]), 0:7].astype(np.float64)
        q0, u0 = hinge_init(n)
        # the engine starts from the float32 state
        qs, us, _ = FrictionStepper(dyn, H, 4, 1, tau_f).run(base, q0.astype(np.float32), u0.astype(np.float32),
                                                            2 * HINGE_FRAMES)
        _HINGE_REF[key] = (qs[1::2], us[1::2], dyn, base)
    return _HINGE_REF[key]


@pytest.mark.parametrize("coupled", [False, True], ids=["uncoupled", "coupled"])
@pytest.mark.parametrize("n", [2, 6, 18])
def test_hinge_chain_against_float64(gym, tmp_path, n, coupled):
    """The friction builds against the float64 stepper, within 4x the distance the
    friction-free kernels keep from it on the same scene (tau_f = 0: the plain
    launch uncoupled, the plain k_env_step coupled)."""
    ne, tau_f = HINGES[n]
    nfd = int(np.count_nonzero(tau_f))
    errs = {}
    for fric in (False, True):
        tf = tau_f if fric else np.zeros(n)
        sim = hinge_scene(gym, tmp_path, n, tf, coupled)
        st = stats(sim)
        want = (0, 0, 0) if not fric else ((ne * nfd, 0, ne) if coupled else (ne * nfd, ne, 0))
        assert st == want, (st, want)
        assert N.lib.mg_num_coupled_envs(sim.native) == (ne if coupled else 0)
        A = sim.model_arrays
        pos, vel, _ = run(gym, sim, HINGE_FRAMES)
        gym.destroy_sim(sim)
        q, u, dyn, base = hinge_reference(A, n, tf)
        assert np.isfinite(pos).all()
        errs[fric] = max(np.abs(pos[:, n * e:n * e + n] - q).max() for e in range(ne))
        if fric:
            # no friction hinge rests within 10 % of its stick threshold: where the chain has come to
            # rest, the static load on each friction hinge is off tau_f by more than that
            if np.abs(u[-1]).max() < 1e-3:
                load = np.abs(dyn.bias(base, q[-1], np.zeros(n)))
                on = tau_f > 0
                assert np.all(np.abs(load[on] / tau_f[on] - 1.0) > 0.1), load[on] / tau_f[on]
            assert np.abs(q - hinge_reference(A, n, np.zeros(n))[0]).max() > 0.05      # friction matters here
    print("%d hinges %s: max |q - float64| %.3g rad with friction, %.3g rad without (bound 4x)"
          % (n, "coupled" if coupled else "uncoupled", errs[True], errs[False]))
    assert errs[False] > 0.0
    assert errs[True] <= 4.0 * errs[False], errs


# ---------------------------------------------------------------- 3. third law
TWO_BOX = """<robot name="twobox">
<link name="a"><inertial><origin xyz="0.05 0.02 -0.03"/><mass value="1.2"/>
  <inertia ixx="0.02" iyy="0.03" izz="0.025" ixy="0.002" ixz="-0.001" iyz="0.0015"/></inertial></link>
<link name="b"><inertial><origin xyz="-0.04 0.06 0.1"/><mass value="0.7"/>
  <inertia ixx="0.012" iyy="0.008" izz="0.015" ixy="-0.001" ixz="0.002" iyz="0.001"/></inertial></link>
<joint name="h" type="continuous"><parent link="a"/><child link="b"/><origin xyz="0.1 0 0.05"/>
  <axis xyz="0.36 0.48 0.8"/></joint>
</robot>"""
SPIN = 6.0


def two_box_run(gym, tmp_path, tau_f):
    (tmp_path / "twobox.urdf").write_text(TWO_BOX)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params(gravity=(0.0, 0.0, 0.0)))
    opts = gymapi.AssetOptions()
    opts.fix_base_link = False
    opts.armature = 0.0
    opts.linear_damping = 0.0
    opts.angular_damping = 0.0
    opts.max_linear_velocity = 1000.0
    opts.max_angular_velocity = 1000.0
    asset = gym.load_asset(sim, str(tmp_path), "twobox.urdf", opts)
    for i in range(5):
        env = gym.create_env(sim, gymapi.Vec3(-1.0, -1.0, 0.0), gymapi.Vec3(1.0, 1.0, 2.0), 3)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 0.0, 1.0)
        h = gym.create_actor(env, asset, pose, "tb", i, 1)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_NONE
        for k in ("stiffness", "damping", "effort", "velocity", "armature"):
            props[k][:] = 0.0
        props["friction"][:] = tau_f
        gym.set_actor_dof_properties(env, h, props)
        st = gym.get_actor_dof_states(env, h, gymapi.STATE_ALL)
        st["vel"][:] = SPIN
        gym.set_actor_dof_states(env, h, st, gymapi.STATE_ALL)
    gym.prepare_sim(sim)
    st = stats(sim)
    assert st == ((5, 0, 5) if tau_f > 0 else (0, 0, 0)), st
    A = sim.model_arrays
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    mass = A["body_mass"][0:2].astype(np.float64)

    def momentum():
        """Total linear momentum and angular momentum about the COM of env 0 (float64)."""
        s = rb[0:2].cpu().numpy().astype(np.float64)
        P, L, cs = np.zeros(3), np.zeros(3), []
        from kinematics64 import qmat
        for k in range(2):
            m, com = mass[k, 11], mass[k, 8:11]
            R = qmat(s[k, 3:7] / np.linalg.norm(s[k, 3:7]))
            cs.append(s[k, 0:3] + R @ com)
            P += m * s[k, 7:10]
        C = (mass[0, 11] * cs[0] + mass[1, 11] * cs[1]) / (mass[0, 11] + mass[1, 11])
        for k in range(2):
            m = mass[k, 11]
            R = qmat(s[k, 3:7] / np.linalg.norm(s[k, 3:7])) @ qmat(mass[k, 4:8])
            Iw = R @ np.diag([1.0 / x for x in mass[k, 1:4]]) @ R.T
            L += Iw @ s[k, 10:13] + m * np.cross(cs[k] - C, s[k, 7:10])
        return P, L

    # the reference is the momentum after the first frame: the link velocities of
    # the rigid-body tensor follow the DOF state from the first step on
    P0 = L0 = None
    dP = dL = 0.0
    for _ in range(FRAMES + 1):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_rigid_body_state_tensor(sim)
        P, L = momentum()
        if P0 is None:
            P0, L0 = P, L
        dP, dL = max(dP, np.abs(P - P0).max()), max(dL, np.abs(L - L0).max())
    gym.refresh_dof_state_tensor(sim)
    rate = dof[:, 1].cpu().numpy().copy()
    gym.destroy_sim(sim)
    return dP, dL, rate, np.abs(P0).max(), np.abs(L0).max()


def test_third_law_floating_hinge(gym, tmp_path):
    """Two boxes joined by a hinge, floating, no gravity, no damping, a relative
    spin to start with: friction stops the hinge and moves no momentum."""
    dP0, dL0, rate0, Pn, Ln = two_box_run(gym, tmp_path, 0.0)
    dP1, dL1, rate1, _, _ = two_box_run(gym, tmp_path, 0.05)
    print("momentum drift over %d frames (|P0| %.3g, |L0| %.3g): friction dP %.3g dL %.3g; none dP %.3g dL %.3g"
          % (FRAMES, Pn, Ln, dP1, dL1, dP0, dL0))
    assert Ln > 0.01 and np.all(np.abs(rate0) > 1.0)
    assert np.all(np.abs(rate1) <= 1e-6 * SPIN)
    assert dP1 <= 4.0 * dP0 and dL1 <= 4.0 * dL0


# ------------------------------------------------------ 4. refusals and routing
def test_refused_with_attractor_sensor_or_reporting(gym, tmp_path):
    """Friction on a coupled group together with a feature whose friction build
    does not exist: refused at simulate, naming the actor."""
    for what in ("attractor", "sensor", "reporting"):
        (tmp_path / "cart3.urdf").write_text(CART_URDF)
        sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params())
        opts = gymapi.AssetOptions()
        opts.fix_base_link = True
        asset = gym.load_asset(sim, str(tmp_path), "cart3.urdf", opts)
        if what == "sensor":
            p = gymapi.ForceSensorProperties()
            assert gym.create_asset_force_sensor(asset, 3, gymapi.Transform(), p) == 0
        box = far_box(gym, sim)
        for i in range(2):
            env = gym.create_env(sim, gymapi.Vec3(-1.0, -1.0, 0.0), gymapi.Vec3(1.0, 1.0, 2.0), 2)
            pose = gymapi.Transform()
            pose.p = gymapi.Vec3(*CART_POSE)
            h = gym.create_actor(env, asset, pose, "cart", i, 0)
            add_far_box(gym, env, box, i)
            props = gym.get_actor_dof_properties(env, h)
            props["driveMode"][:] = gymapi.DOF_MODE_NONE
            props["friction"][:] = 1.0 if i == 1 else 0.0
            gym.set_actor_dof_properties(env, h, props)
            if what == "attractor" and i == 0:
                last = gym.find_actor_rigid_body_handle(env, h, "lz")
                assert gym.create_rigid_body_attractor(
                    env, attractor(last, 100.0, 10.0, gymapi.AXIS_TRANSLATION, CART_POSE)) == 0
        gym.prepare_sim(sim)
        if what == "reporting":
            gym.set_rigid_contact_reporting(sim, True)
        assert stats(sim) == (3, 0, 2)
        with pytest.raises(N.MigymError, match="actor 2: joint friction"):
            gym.simulate(sim)
        gym.destroy_sim(sim)


def one_cart(gym, tmp_path):
    sim, handles = cart_scene(gym, tmp_path, {}, False, num_envs=2)
    return sim, handles


def test_set_after_prepare_reroutes(gym, tmp_path):
    """0 -> tau_f after prepare_sim: the instance moves to the friction launch and
    its joint sticks; a negative value is refused and changes nothing."""
    sim, handles = one_cart(gym, tmp_path)
    assert stats(sim) == (0, 0, 0) and N.lib.mg_step_out_supported(sim.native) == 1
    pos, vel, _ = run(gym, sim, 5, effort=cart_effort(2))
    assert np.all(vel[-1, [0, 3]] == X_V0)
    env, h = handles[1]
    props = gym.get_actor_dof_properties(env, h)
    props["friction"][0] = 50.0
    gym.set_actor_dof_properties(env, h, props)
    assert stats(sim) == (1, 1, 0) and N.lib.mg_step_out_supported(sim.native) == 0
    pos, vel, _ = run(gym, sim, 20, effort=cart_effort(2))
    assert vel[-1, 0] == X_V0 and abs(vel[-1, 3]) <= 1e-6 and np.abs(pos[-1, 3] - pos[10, 3]) < 1e-6
    dp = np.zeros((6, N.MG_DOFPROP_N), dtype=np.float32)
    dp[2, 9] = -1.0
    assert N.lib.mg_set_dof_props(sim.native, dp.ctypes.data) == -1            # MG_ERR_ARG
    assert "friction" in N.last_error() and stats(sim) == (1, 1, 0)
    props["friction"][0] = 0.0
    gym.set_actor_dof_properties(env, h, props)
    assert stats(sim) == (0, 0, 0) and N.lib.mg_step_out_supported(sim.native) == 1
    gym.destroy_sim(sim)


def test_reroute_refused_after_capture(gym, tmp_path):
    """A set that changes the routing after a simulate was captured into a graph
    is refused (the replays keep the old launches); one that keeps it is not."""
    sim, handles = one_cart(gym, tmp_path)
    env, h = handles[1]
    props = gym.get_actor_dof_properties(env, h)
    props["friction"][0] = 50.0
    gym.set_actor_dof_properties(env, h, props)
    try:
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                gym.simulate(sim)
                gym.fetch_results(sim, True)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        props["friction"][0] = 20.0                      # the same routing: accepted, the replays read the new value
        gym.set_actor_dof_properties(env, h, props)
        assert stats(sim) == (1, 1, 0)
        props["friction"][0] = 0.0
        with pytest.raises(N.MigymError, match="captured into a graph"):
            gym.set_actor_dof_properties(env, h, props)
        assert stats(sim) == (1, 1, 0)
    finally:
        gym.destroy_sim(sim)
