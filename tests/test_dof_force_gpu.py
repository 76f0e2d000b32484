"""DOF force tensor on the GPU: the step kernels' per-DOF
drive forces against the drive law evaluated in float64 from the DOF-state
tensor, statics, saturation, the grip-force cross-check, no side effects on
the trajectory, graph capture and the CPU pipeline."""
import math

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
from test_isaacgym_amd import scenes
from kinematics64 import Articulation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 9.8
POS, VEL, EFFORT = 1, 2, 3


def _wrap(gym, sim):
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    frc = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
    return dof, frc


def _enable(gym, envs, actor=0):
    for env in envs:
        assert gym.enable_actor_dof_force_sensors(env, actor) is True


def _step(gym, sim):
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_dof_state_tensor(sim)
    gym.refresh_dof_force_tensor(sim)


def _identity(gym, sim, frames, targets, before_step=None, what=""):
    """With one substep: tau = clamp(kp (q* - q_prev - dt u_new) + kd (qd* - u_new), +-eff),
    q_prev read before the step, u_new after it, in float64; per DOF within
    16 * 2^-23 * (kp (|q*| + |q_prev| + dt |u_prev| + dt |u_new|) + kd (|qd*| + |u_prev| + |u_new|)),
    the rounding of the dozen fp32 operations of tau0 - imp (u+ - u) / h. A DOF
    outside it must read +-eff bit for bit (the effort-limit re-solve ran it at
    the limit). Returns (readings per frame, DOFs at +-eff per frame)."""
    assert sim.params.substeps == 1
    pr = sim.model_arrays["dof_props"].astype(np.float64)
    mode, eff = pr[:, 0].astype(int), pr[:, 3]
    kp = np.where(mode == POS, pr[:, 1], 0.0)
    kd = np.where((mode == POS) | (mode == VEL), pr[:, 2], 0.0)
    assert not np.any(mode == EFFORT)
    dt = float(sim.params.dt)
    dof, frc = _wrap(gym, sim)
    gym.refresh_dof_state_tensor(sim)
    eff32 = eff.astype(np.float32)
    out, nsat, worst = [], [], 0.0
    for k in range(frames):
        prev = dof.cpu().numpy().astype(np.float64)
        tp, tv = targets(k, prev)
        tp, tv = tp.astype(np.float32), tv.astype(np.float32)
        assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(torch.from_numpy(tp).to(DEV)))
        assert gym.set_dof_velocity_target_tensor(sim, gymtorch.unwrap_tensor(torch.from_numpy(tv).to(DEV)))
        if before_step is not None:
            before_step(k)
        _step(gym, sim)
        new = dof.cpu().numpy().astype(np.float64)
        got = frc.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        tp64, tv64 = tp.astype(np.float64), tv.astype(np.float64)
        rhs = kp * (tp64 - prev[:, 0] - dt * new[:, 1]) + kd * (tv64 - new[:, 1])
        rhs = np.where(eff > 0, np.clip(rhs, -eff, eff), rhs)
        tol = 16.0 * 2.0 ** -23 * (kp * (np.abs(tp64) + np.abs(prev[:, 0]) + dt * np.abs(prev[:, 1]) + dt * np.abs(new[:, 1]))
                                   + kd * (np.abs(tv64) + np.abs(prev[:, 1]) + np.abs(new[:, 1])))
        err = np.abs(got.astype(np.float64) - rhs)
        at_eff = (eff > 0) & ((got == eff32) | (got == -eff32))
        inside = err <= tol
        bad = ~inside & ~at_eff
        worst = max(worst, float((err / np.maximum(tol, 1e-30))[inside | bad].max(initial=0.0)))
        assert not bad.any(), "%s frame %d: DOFs %s read %s, drive law %s (tol %s)" % (
            what, k, np.nonzero(bad)[0][:8], got[bad][:8], rhs[bad][:8], tol[bad][:8])
        out.append(got.copy())
        nsat.append(int((at_eff & ~inside).sum()))
    print("%s: %d frames x %d DOFs, worst err / tol %.3f, readings at +-eff outside the drive law: %d, max |tau| %.4g"
          % (what, frames, len(eff), worst, sum(nsat), max(float(np.abs(o).max()) for o in out)))
    return out, nsat


def _wave(amp, rate):
    """Targets moving about the start pose: q0 + amp sin(rate k + phase_d)."""
    st = {}

    def targets(k, prev):
        if "q0" not in st:
            st["q0"] = prev[:, 0].copy()
            st["ph"] = np.random.RandomState(11).uniform(0, 2 * math.pi, size=len(prev))
        tp = st["q0"] + amp * np.sin(rate * (k + 1) + st["ph"])
        tv = amp * rate * 60.0 * 0.1 * np.cos(rate * (k + 1) + st["ph"])
        return tp, tv
    return targets


# ------------------------------------------------------------- GPU 1: identity
def _gimbal(gym, n, substeps=None, gravity=None, **kw):
    sim, envs = scenes.gimbal_scene(gym, n, **kw)
    if substeps is not None:
        sim.params.substeps = substeps
    if gravity is not None:
        sim.params.gravity = gymapi.Vec3(0.0, 0.0, gravity)
    return sim, envs


def test_identity_gimbal_quad(gym):
    """k_artic_chain_q (four lanes per chain): 4 gimbals, 30 frames of moving targets."""
    sim, envs = _gimbal(gym, 4, substeps=1)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    out, _ = _identity(gym, sim, 30, _wave(0.12, 0.35), what="gimbal quad")
    assert max(np.abs(o).max() for o in out) > 0.5
    gym.destroy_sim(sim)


@pytest.mark.parametrize("differ", ["dof_props", "link_mass"])
def test_identity_gimbal_quad_per_lane_forms(gym, differ):
    """The chain kernel's other forms: one env with its own DOF properties (the
    per-lane property loads) or its own link masses (no shared constants at all)."""
    sim, envs = _gimbal(gym, 5, substeps=1)
    if differ == "dof_props":
        props = gym.get_actor_dof_properties(envs[1], 0)
        props["stiffness"][:] = 30.0
        props["damping"][:] = 2.0
        gym.set_actor_dof_properties(envs[1], 0, props)
    else:
        bp = gym.get_actor_rigid_body_properties(envs[1], 0)
        for b in bp:
            b.mass = b.mass * 3.0
        gym.set_actor_rigid_body_properties(envs[1], 0, bp, True)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    out, _ = _identity(gym, sim, 10, _wave(0.12, 0.35), what="gimbal quad, own " + differ)
    # not a trivial zero: the readings stand four orders above the tolerance (~1e-5 N m)
    assert max(np.abs(o).max() for o in out) > 0.1
    gym.destroy_sim(sim)


def test_identity_gimbal_one_lane(gym):
    """k_artic_chain's one-lane form: just over MG_CHAIN_QUAD_MAX / 4 = 16384 gimbals, one step."""
    n = 16384 + 70
    sim, envs = _gimbal(gym, n, substeps=1)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_dof_force_dofs(sim.native) == 3 * n
    out, _ = _identity(gym, sim, 1, _wave(0.12, 0.35), what="gimbal one lane")
    assert np.count_nonzero(out[0]) > 2 * n
    gym.destroy_sim(sim)


def _franka_alone(gym, n, substeps=1):
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -G)
    sp.dt, sp.substeps = 1.0 / 60.0, substeps
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 4
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.armature = 0.01
    opts.flip_visual_attachments = True
    asset = gym.load_asset(sim, scenes.ASSET_ROOT, "franka/franka_proxy.urdf", opts)
    assert asset is not None
    props = gym.get_asset_dof_properties(asset)
    mids = 0.5 * (props["upper"] + props["lower"])
    props["driveMode"][:] = gymapi.DOF_MODE_POS
    props["stiffness"][:7], props["damping"][:7] = 400.0, 40.0
    props["stiffness"][7:], props["damping"][7:] = 800.0, 40.0
    envs = []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 2)
        h = gym.create_actor(env, asset, gymapi.Transform(), "franka", i, 1)
        gym.set_actor_dof_properties(env, h, props)
        st = gym.get_actor_dof_states(env, h, gymapi.STATE_NONE)
        st["pos"][:] = mids
        gym.set_actor_dof_states(env, h, st, gymapi.STATE_POS)
        envs.append(env)
    return sim, envs


def test_identity_franka_lanes(gym):
    """k_artic_lanes: the Franka alone (9 DOFs, gravity on), POS arm and fingers."""
    sim, envs = _franka_alone(gym, 4)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == 0
    out, _ = _identity(gym, sim, 30, _wave(0.02, 0.3), what="franka lanes")
    assert max(np.abs(o).max() for o in out) > 1.0
    gym.destroy_sim(sim)


def test_identity_cube_pick_contact(gym):
    """k_env_step with contacts: the cube-pick scene (POS arm and fingers), the
    cube held between the open fingers while they close on it."""
    n = 4
    sim, info = scenes.franka_scene(gym, n, controller="ik")
    sim.params.substeps = 1
    envs = info["envs"]
    _enable(gym, envs, actor=2)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == n
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    gym.refresh_actor_root_state_tensor(sim)
    gym.refresh_rigid_body_state_tensor(sim)
    hand = rb[info["hand_idxs"]].clone()
    # between the fingers: 0.0584 m (the finger joints) + 0.032 m along the hand's z
    q = hand[:, 3:7]
    z = torch.stack([2 * (q[:, 0] * q[:, 2] + q[:, 3] * q[:, 1]), 2 * (q[:, 1] * q[:, 2] - q[:, 3] * q[:, 0]),
                     1 - 2 * (q[:, 0] ** 2 + q[:, 1] ** 2)], dim=1)
    box_actor = torch.tensor([3 * e + 1 for e in range(n)], dtype=torch.int32, device=DEV)
    held = root.clone()
    held[box_actor.long(), 0:3] = hand[:, 0:3] + 0.0904 * z
    held[box_actor.long(), 3:7] = q
    held[box_actor.long(), 7:13] = 0.0
    touched = []

    def hold(k):
        assert gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(held),
                                                       gymtorch.unwrap_tensor(box_actor), n)
        if k > 0:
            gym.refresh_net_contact_force_tensor(sim)
            touched.append(float(ncf[info["box_idxs"]].abs().max()))

    def targets(k, prev):
        tp = prev[:, 0].copy().reshape(n, 9)
        if k == 0:
            targets.q0 = tp.copy()
        tp = targets.q0.copy()
        tp[:, 7:] = 0.0                      # close the fingers
        return tp.reshape(-1), np.zeros(n * 9)

    out, _ = _identity(gym, sim, 30, targets, before_step=hold, what="cube pick")
    print("cube pick: max |net contact force| on the cube per frame: %s" % np.round(touched, 2))
    assert max(touched) > 0.1, "the fingers never touched the cube"
    fingers = np.stack(out)[:, :].reshape(30, n, 9)[:, :, 7:]
    assert np.abs(fingers[-1]).min() > 0.5      # both fingers of every env squeeze
    gym.destroy_sim(sim)


def test_identity_ant_floating_base(gym):
    """k_env_step on a floating base: the MJCF ant dropped onto the ground, POS drives."""
    n = 4
    sim, info = scenes.ant_scene(gym, n, height=0.6)
    assert sim.params.substeps == 1
    for env, a in zip(info["envs"], info["actors"]):
        props = gym.get_actor_dof_properties(env, a)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:] = 20.0
        props["damping"][:] = 1.0
        gym.set_actor_dof_properties(env, a, props)
        assert gym.enable_actor_dof_force_sensors(env, a) is True
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == n
    out, _ = _identity(gym, sim, 40, _wave(0.2, 0.3), what="ant")
    assert max(np.abs(o).max() for o in out) > 0.5
    gym.destroy_sim(sim)


def test_identity_ball_joint_chain(gym, tmp_path):
    """Ball joints: test13's chain (three prismatic joints, then a spherical one
    whose three packed DOFs report like any other)."""
    from test_ball_joint import _scene, _urdf
    d = str(tmp_path)
    n = 4
    rng = np.random.RandomState(3)
    init = rng.uniform(-0.3, 0.3, size=(n, 6)).astype(np.float32)
    sim, _ = _scene(gym, d, n, _urdf(d, "b.urdf"), gpu=True, drive=(40.0, 4.0),
                    init=lambda i: (init[i], np.zeros(6)))
    sim.params.substeps = 1
    for env in sim.envs:
        assert gym.enable_actor_dof_force_sensors(env, 0) is True
    gym.prepare_sim(sim)
    out, _ = _identity(gym, sim, 30, _wave(0.05, 0.3), what="ball joint chain")
    ball = np.stack(out).reshape(30, n, 6)[:, :, 3:]
    assert np.abs(ball).max() > 0.5
    gym.destroy_sim(sim)


# ------------------------------------------------------------- GPU 2: statics
LIFT_URDF = """<robot name="lift">
<link name="base"><inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
<link name="load"><inertial><mass value="2"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial>
<collision><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
<joint name="lift" type="prismatic"><parent link="base"/><child link="load"/><origin xyz="0 0 0"/><axis xyz="0 0 1"/>
<limit lower="-1" upper="1" effort="100" velocity="10"/></joint></robot>"""


def test_static_vertical_prismatic(gym, tmp_path):
    """A 2 kg load held by a vertical POS drive, 2 substeps, settled for 240
    frames: tau = M g within M |du| / dt + 1e-4 M g."""
    (tmp_path / "lift.urdf").write_text(LIFT_URDF)
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -G)
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    asset = gym.load_asset(sim, str(tmp_path), "lift.urdf", opts)
    n, M = 4, 2.0
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 2)
        h = gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 1.0)), "lift", i, 1)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:], props["damping"][:] = 1000.0, 100.0
        gym.set_actor_dof_properties(env, h, props)
        assert gym.get_actor_rigid_body_properties(env, h)[1].mass == M
        assert gym.enable_actor_dof_force_sensors(env, h) is True
    gym.prepare_sim(sim)
    dof, frc = _wrap(gym, sim)
    tg = torch.full((n,), 0.2, dtype=torch.float32, device=DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(239):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_dof_state_tensor(sim)
    u0 = dof[:, 1].cpu().numpy().astype(np.float64)
    _step(gym, sim)
    u1 = dof[:, 1].cpu().numpy().astype(np.float64)
    tau = frc.cpu().numpy().astype(np.float64)
    bound = M * np.abs(u1 - u0) * 60.0 + 1e-4 * M * G
    print("lift: tau %s, M g %.6f, |tau - M g| %s, bound %s" % (tau, M * G, np.abs(tau - M * G), bound))
    assert np.all(np.abs(tau - M * G) <= bound)
    gym.destroy_sim(sim)


def test_static_gimbal_gravity_torque(gym):
    """The gimbal (1 kg links, COMs off the axes) held off-axis under gravity:
    each joint's tau is the float64 gravity torque about its axis
    (kinematics64), within sum_k M_jk |du_k| / dt + 1e-4 sum_l m_l g |Jv_l[:, j]|."""
    n = 4
    com = [(0.04, 0.03, 0.02), (-0.03, 0.02, 0.05), (0.02, -0.04, 0.03)]
    sim, envs = _gimbal(gym, n, gravity=-G)
    for env in envs:
        bp = gym.get_actor_rigid_body_properties(env, 0)
        for b, c in zip(bp[1:], com):
            b.mass = b.mass * 100.0
            b.com = gymapi.Vec3(*c)
        gym.set_actor_rigid_body_properties(env, 0, bp, True)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    dof, frc = _wrap(gym, sim)
    tg = torch.tensor([0.5, 0.4, -0.3] * n, dtype=torch.float32, device=DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(239):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_dof_state_tensor(sim)
    u0 = dof[:, 1].cpu().numpy().astype(np.float64).reshape(n, 3)
    _step(gym, sim)
    ds = dof.cpu().numpy().astype(np.float64).reshape(n, 3, 2)
    tau = frc.cpu().numpy().astype(np.float64).reshape(n, 3)
    A = sim.model_arrays
    art = Articulation(A)
    gv = np.array([0.0, 0.0, -G])
    for e in range(n):
        fb = int(A["actor_root_body"][e])
        q = ds[e, :, 0]
        ps, Rs, zs = art.fk(A["body_state0"][fb, 0:7], q)
        ref, scale = np.zeros(3), np.zeros(3)
        for l, b in art.bodies()[1:]:
            mrow = A["body_mass"][fb + b].astype(np.float64)
            Jv = art.point_jacobian(ps, zs, l, ps[l] + Rs[l] @ mrow[8:11])[0:3]
            ref -= mrow[11] * (gv @ Jv)
            scale += mrow[11] * G * np.linalg.norm(Jv, axis=0)
        Mq = art.mass_matrix(A["body_state0"][fb, 0:7], q, fb)
        bound = np.abs(Mq) @ np.abs(ds[e, :, 1] - u0[e]) * 60.0 + 1e-4 * scale
        print("gimbal env %d: tau %s, gravity torque %s, bound %s" % (e, tau[e], ref, bound))
        assert np.abs(ref).max() > 0.1
        assert np.all(np.abs(tau[e] - ref) <= bound)
    gym.destroy_sim(sim)


# ------------------------------------------------- GPU 3: saturation and modes
def test_saturation_reads_effort_limit(gym):
    """kp 2000 on 10 kg links against the 10 N m limit (the scene of
    test_gimbal_effort_limit_parity): a DOF whose position error asks for 20
    times the limit reads exactly +-eff."""
    n, steps = 4, 20
    sim, envs = _gimbal(gym, n, stiffness=2000.0, damping=0.5, link_mass_scale=1000.0)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    dof, frc = _wrap(gym, sim)
    tg = scenes.gimbal_targets(n, steps, DEV, seed=5)
    gym.refresh_dof_state_tensor(sim)
    seen = 0
    for k in range(steps):
        q_prev = dof[:, 0].cpu().numpy().astype(np.float64)
        assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg[k].contiguous()))
        _step(gym, sim)
        got = frc.cpu().numpy()
        err = tg[k].cpu().numpy().astype(np.float64) - q_prev
        sat = np.abs(err) > 0.1
        seen += int(sat.sum())
        want = np.where(err > 0, np.float32(10.0), np.float32(-10.0)).astype(np.float32)
        assert np.array_equal(got[sat], want[sat]), "frame %d: %s vs %s" % (k, got[sat], want[sat])
        assert np.all(np.abs(got) <= np.float32(10.0))
    assert seen > steps * n
    gym.destroy_sim(sim)


def test_effort_and_none_modes(gym):
    """EFFORT: the reading is the applied effort, clamped to +-eff; NONE: 0."""
    n = 4
    for mode in (gymapi.DOF_MODE_EFFORT, gymapi.DOF_MODE_NONE):
        sim, envs = _gimbal(gym, n, drive_mode=mode)
        _enable(gym, envs)
        gym.prepare_sim(sim)
        dof, frc = _wrap(gym, sim)
        rng = np.random.RandomState(2)
        for k in range(3):
            f = rng.uniform(-15.0, 15.0, size=3 * n).astype(np.float32)
            assert gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(torch.from_numpy(f).to(DEV)))
            _step(gym, sim)
            got = frc.cpu().numpy()
            want = np.clip(f, np.float32(-10.0), np.float32(10.0)) if mode == gymapi.DOF_MODE_EFFORT else np.zeros_like(f)
            assert np.array_equal(got, want), (mode, got, want)
        assert mode == gymapi.DOF_MODE_NONE or np.abs(got).max() == 10.0
        gym.destroy_sim(sim)


# ------------------------------------------------- GPU 4: grip force cross-check
PUSHER_URDF = """<robot name="pusher">
<link name="base"><inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
<link name="pad"><inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial>
<collision><geometry><box size="0.1 0.1 0.1"/></geometry></collision></link>
<joint name="push" type="prismatic"><parent link="base"/><child link="pad"/><origin xyz="0 0 0"/><axis xyz="1 0 0"/>
<limit lower="-1" upper="1" effort="1000" velocity="10"/></joint></robot>"""


def test_grip_force_matches_contact_force(gym, tmp_path):
    """A fixed-base one-DOF prismatic pusher drives a 0.5 kg box against a static
    wall (no gravity, no ground), target beyond the wall. At rest the drive
    force equals the force the box returns to the pad along the wall normal.

    The net contact force of the box itself is no measure of the grip: it sums
    the pad's push and the wall's reaction, which cancel at rest. The pad's own
    entry holds the box's reaction alone, so tau = -F_pad . n, within
    m_box |dv_box| / dt + m_pad |du| / dt + 1e-3 |tau|."""
    (tmp_path / "pusher.urdf").write_text(PUSHER_URDF)
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, 0.0)
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 8
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    pusher = gym.load_asset(sim, str(tmp_path), "pusher.urdf", opts)
    wall = gym.create_box(sim, 0.1, 0.4, 0.4, opts)
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    n, m_box, m_pad = 4, 0.5, 1.0
    pads, boxes = [], []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 2)
        h = gym.create_actor(env, pusher, gymapi.Transform(gymapi.Vec3(0, 0, 1.0)), "pusher", i, 0)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:], props["damping"][:] = 200.0, 40.0
        gym.set_actor_dof_properties(env, h, props)
        b = gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.12, 0, 1.0)), "box", i, 0)
        bp = gym.get_actor_rigid_body_properties(env, b)
        bp[0].mass = m_box
        gym.set_actor_rigid_body_properties(env, b, bp, True)
        gym.create_actor(env, wall, gymapi.Transform(gymapi.Vec3(0.24, 0, 1.0)), "wall", i, 0)
        assert gym.enable_actor_dof_force_sensors(env, h) is True
        pads.append(gym.find_actor_rigid_body_index(env, h, "pad", gymapi.DOMAIN_SIM))
        boxes.append(gym.get_actor_rigid_body_index(env, b, 0, gymapi.DOMAIN_SIM))
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == n
    dof, frc = _wrap(gym, sim)
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    tg = torch.full((n,), 0.3, dtype=torch.float32, device=DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(179):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_dof_state_tensor(sim)
    gym.refresh_rigid_body_state_tensor(sim)
    u0 = dof[:, 1].cpu().numpy().astype(np.float64)
    v0 = rb[boxes, 7].cpu().numpy().astype(np.float64)
    _step(gym, sim)
    gym.refresh_rigid_body_state_tensor(sim)
    gym.refresh_net_contact_force_tensor(sim)
    u1 = dof[:, 1].cpu().numpy().astype(np.float64)
    v1 = rb[boxes, 7].cpu().numpy().astype(np.float64)
    q = dof[:, 0].cpu().numpy()
    tau = frc.cpu().numpy().astype(np.float64)
    f_pad = ncf[pads, 0].cpu().numpy().astype(np.float64)
    f_box = ncf[boxes, 0].cpu().numpy().astype(np.float64)
    bound = m_box * np.abs(v1 - v0) * 60.0 + m_pad * np.abs(u1 - u0) * 60.0 + 1e-3 * np.abs(tau)
    print("pusher: q %s, tau %s, -F_pad.x %s, F_box.x %s, bound %s" % (q, tau, -f_pad, f_box, bound))
    assert np.all(q > 0.01) and np.all(q < 0.06)          # the pad rests against the box, the box against the wall
    assert np.all(tau > 10.0)
    assert np.all(np.abs(tau - (-f_pad)) <= bound)
    gym.destroy_sim(sim)


# ------------------------------------------------------ GPU 5: no side effects
def _scene_for(gym, name, n):
    if name == "gimbal":
        sim, envs = _gimbal(gym, n)
        return sim, envs, 0, 3
    if name == "franka":
        sim, envs = _franka_alone(gym, n, substeps=2)
        return sim, envs, 0, 9
    sim, info = scenes.franka_scene(gym, n, controller="ik")
    return sim, info["envs"], 2, 9


@pytest.mark.parametrize("name", ["gimbal", "franka", "cube_pick"])
def test_reporting_leaves_the_trajectory_alone(gym, name):
    """Two sims of one scene, reporting on the actors of envs 0 and 2 in one of
    them: root, rigid-body and DOF states bit-identical after 60 frames; the
    other envs' rows of the tensor exactly 0."""
    n = 4
    runs = []
    for report in (False, True):
        sim, envs, actor, nd = _scene_for(gym, name, n)
        if report:
            for e in (0, 2):
                assert gym.enable_actor_dof_force_sensors(envs[e], actor) is True
        gym.prepare_sim(sim)
        assert N.lib.mg_num_dof_force_dofs(sim.native) == (2 * nd if report else 0)
        dof, frc = _wrap(gym, sim)
        root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
        rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        gym.refresh_dof_state_tensor(sim)
        q0 = dof[:, 0].clone()
        ph = torch.linspace(0.0, 5.0, q0.numel(), device=DEV)
        seen = torch.zeros_like(q0)
        for k in range(60):
            tg = (q0 + 0.1 * torch.sin(0.3 * k + ph)).contiguous()
            assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            gym.refresh_dof_force_tensor(sim)
            seen = torch.maximum(seen, frc.abs())
        gym.refresh_dof_state_tensor(sim)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        runs.append((root.clone(), rb.clone(), dof.clone(), seen.view(n, nd).cpu().numpy()))
        gym.destroy_sim(sim)
    (ra, ba, da, fa), (rb_, bb, db, fb) = runs
    assert torch.equal(ra, rb_) and torch.equal(ba, bb) and torch.equal(da, db)
    assert np.all(fa == 0.0)
    assert np.all(fb[[1, 3]] == 0.0)
    assert np.all(fb[[0, 2]].max(axis=1) > 0.0)


# ------------------------------------------------------------ GPU 6: lifecycle
def test_graph_capture_and_refusal(gym):
    """simulate + fetch + refresh_dof_force_tensor captured into a graph: three
    replays update the tensor as three eager steps do. Enabling after the
    captured simulate is refused (MG_ERR_STATE) and the sim stays usable."""
    n = 4
    tg = torch.tensor([0.3, -0.2, 0.1] * n, dtype=torch.float32, device=DEV)
    eager = []
    sim, envs = _gimbal(gym, n)
    _enable(gym, envs)
    gym.prepare_sim(sim)
    _, frc = _wrap(gym, sim)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(3):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_dof_force_tensor(sim)
        eager.append(frc.clone())
    gym.destroy_sim(sim)
    assert not torch.equal(eager[0], eager[2])

    sim, envs = _gimbal(gym, n)
    for e in (0, 1, 2):
        assert gym.enable_actor_dof_force_sensors(envs[e], 0) is True
    gym.prepare_sim(sim)
    assert gym.enable_actor_dof_force_sensors(envs[3], 0) is True      # after prepare_sim, before the first simulate
    _, frc = _wrap(gym, sim)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            gym.refresh_dof_force_tensor(sim)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(frc, eager[k]), "replay %d" % k
    # the flags choose the launches: refused after the capture, nothing changes
    on = np.zeros(n, dtype=np.int32)
    assert N.lib.mg_enable_dof_forces(sim.native, on.ctypes.data, n) == -3      # MG_ERR_STATE
    assert "captured into a graph" in N.last_error()
    assert N.lib.mg_num_dof_force_dofs(sim.native) == 3 * n
    assert gym.enable_actor_dof_force_sensors(envs[0], 0) is False
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(frc).all() and float(frc.abs().max()) > 0.0
    gym.simulate(sim)                                                   # eager again
    gym.fetch_results(sim, True)
    gym.refresh_dof_force_tensor(sim)
    assert torch.isfinite(frc).all()
    gym.destroy_sim(sim)


def test_cpu_pipeline_matches_gpu_pipeline(gym):
    """use_gpu_pipeline = False: a host tensor with the GPU pipeline's values."""
    n = 4
    tgs = scenes.gimbal_targets(n, 5, "cpu", seed=3) * 0.2
    got = {}
    for gpu in (True, False):
        sim, envs = _gimbal(gym, n, use_gpu_pipeline=gpu)
        _enable(gym, envs)
        gym.prepare_sim(sim)
        frc = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
        assert frc.device.type == ("cuda" if gpu else "cpu")
        rows = []
        for k in range(5):
            t = tgs[k].contiguous().to(DEV if gpu else "cpu")
            assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(t))
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            assert gym.refresh_dof_force_tensor(sim) is True
            rows.append(frc.cpu().numpy().copy())
        per_actor = np.concatenate([gym.get_actor_dof_forces(env, 0) for env in envs])
        assert np.array_equal(per_actor, rows[-1])
        got[gpu] = np.stack(rows)
        gym.destroy_sim(sim)
    assert np.abs(got[True]).max() > 0.1
    assert np.array_equal(got[True], got[False])
