"""Rigid-body attractors on the GPU: the implicit pose spring
in the articulated-body kernels (k_artic_lanes, k_env_step) and in the
free-body kernels, against the closed scalar recurrence a decoupled attractor
obeys, held here in float64:

    v <- (M v + h (K (x_t - x) + M g)) / (M + h D + h^2 K);   x <- x + h v

All scenes: dt 1/60, 2 substeps (h = 1/120). Tolerance on the displacement from
the start: 2e-5 m + 1e-4 |displacement| (the project's float64-check precedent,
rtol 1e-4 / atol 1e-5, the absolute term doubled for global coordinates of up
to 8 m)."""
import math

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
from test_isaacgym_amd import scenes

pytestmark = pytest.mark.gpu

H = 1.0 / 120.0
GAINS = [(200.0, 4.0), (5e5, 5e3)]          # soft and underdamped; the script's stiff pair
G_Z = -9.81
OFFSET = np.array([0.3, -0.2, 0.25])

CART_URDF = """<?xml version="1.0"?>
<robot name="cart3">
  <link name="base"/>
  <link name="lx"><inertial><origin xyz="0 0 0"/><mass value="3.0"/>
    <inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial></link>
  <link name="ly"><inertial><origin xyz="0 0 0"/><mass value="2.0"/>
    <inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial></link>
  <link name="lz"><inertial><origin xyz="0 0 0"/><mass value="0.5"/>
    <inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial></link>
  <joint name="jx" type="prismatic"><parent link="base"/><child link="lx"/><origin xyz="0 0 0"/>
    <axis xyz="1 0 0"/><limit lower="-100" upper="100" effort="1000" velocity="100"/></joint>
  <joint name="jy" type="prismatic"><parent link="lx"/><child link="ly"/><origin xyz="0 0 0"/>
    <axis xyz="0 1 0"/><limit lower="-100" upper="100" effort="1000" velocity="100"/></joint>
  <joint name="jz" type="prismatic"><parent link="ly"/><child link="lz"/><origin xyz="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-100" upper="100" effort="1000" velocity="100"/></joint>
</robot>
"""
CART_M = np.array([5.5, 2.5, 0.5])          # effective mass on x, y, z


def recurrence(M, K, D, g, xt, frames, x0=0.0, v0=0.0):
    """Positions after each frame (2 substeps), float64; arrays broadcast."""
    M, K, D, g, xt = (np.asarray(a, dtype=np.float64) for a in (M, K, D, g, xt))
    x = np.zeros(np.broadcast(M, K, D, g, xt).shape) + x0
    v = np.zeros_like(x) + v0
    out = []
    for _ in range(frames):
        for _ in range(2):
            v = (M * v + H * (K * (xt - x) + M * g)) / (M + H * D + H * H * K)
            x = x + H * v
        out.append(x.copy())
    return np.array(out)


def close(got, ref):
    """The issue's bound, on displacements from the start."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return err, 2e-5 + 1e-4 * np.abs(ref)


def sim_params(gravity=(0.0, 0.0, G_Z)):
    sp = gymapi.SimParams()
    sp.dt = 1.0 / 60.0
    sp.substeps = 2
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(*gravity)
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 4
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    return sp


def attractor(rigid_handle, K, D, axes, target_p, target_r=None):
    p = gymapi.AttractorProperties()
    p.stiffness, p.damping, p.axes, p.rigid_handle = K, D, axes, rigid_handle
    p.target = gymapi.Transform(gymapi.Vec3(*[float(c) for c in target_p]), target_r)
    return p


# ----------------------------------------------------------------- Cartesian chain
CART_POSE = (0.0, 0.0, 1.0)


def cart_scene(gym, tmp_path, attrs, y_vel=0.0, num_envs=5, coupled=False):
    """num_envs fixed bases with three prismatic joints along x, y, z, no ground.
    attrs: env -> (K, D, axes, target offset from the last link's start, target
    orientation or None); envs not listed carry no attractor. coupled: a fixed
    box 5 m away in the chain's collision group makes each env a coupled one
    (the chain has no collision shape, so nothing ever touches)."""
    (tmp_path / "cart3.urdf").write_text(CART_URDF)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.armature = 0.0
    opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE
    asset = gym.load_asset(sim, str(tmp_path), "cart3.urdf", opts)
    assert asset is not None
    lo, hi = gymapi.Vec3(-1.0, -1.0, 0.0), gymapi.Vec3(1.0, 1.0, 2.0)
    box = None
    if coupled:
        bopts = gymapi.AssetOptions()
        bopts.fix_base_link = True
        box = gym.create_box(sim, 0.1, 0.1, 0.1, bopts)
    for i in range(num_envs):
        env = gym.create_env(sim, lo, hi, 3)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(*CART_POSE)
        h = gym.create_actor(env, asset, pose, "cart", i, 0 if coupled else 1)
        if coupled:
            bpose = gymapi.Transform()
            bpose.p = gymapi.Vec3(0.0, 0.0, -5.0)
            gym.create_actor(env, box, bpose, "box", i, 0)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_NONE
        for k in ("stiffness", "damping", "armature", "friction"):
            props[k][:] = 0.0
        props["velocity"][:] = 100.0
        props["lower"][:], props["upper"][:] = -100.0, 100.0
        gym.set_actor_dof_properties(env, h, props)
        if y_vel:
            st = gym.get_actor_dof_states(env, h, gymapi.STATE_ALL)
            st["vel"][1] = y_vel
            gym.set_actor_dof_states(env, h, st, gymapi.STATE_ALL)
        if i in attrs:
            K, D, axes, off, rot = attrs[i]
            last = gym.find_actor_rigid_body_handle(env, h, "lz")
            assert gym.create_rigid_body_attractor(
                env, attractor(last, K, D, axes, np.array(CART_POSE) + off, rot)) == 0
    gym.prepare_sim(sim)
    return sim


def run_frames(gym, sim, frames):
    """(dof positions per frame [frames, nd], last DOF state, last rigid-body state)."""
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    pos = []
    for _ in range(frames):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_dof_state_tensor(sim)
        pos.append(dof[:, 0].cpu().numpy().copy())
    gym.refresh_rigid_body_state_tensor(sim)
    return np.array(pos), dof.cpu().numpy().copy(), rb.cpu().numpy().copy()


@pytest.fixture(scope="module")
def cart_plain(tmp_path_factory):
    """The 5-env chain scene with no attractor at all, 120 frames (shared)."""
    gym = gymapi.acquire_gym()
    sim = cart_scene(gym, tmp_path_factory.mktemp("cart_plain"), {})
    assert N.lib.mg_num_attractors(sim.native) == 0
    out = run_frames(gym, sim, 120)
    gym.destroy_sim(sim)
    return out


def env_offset(e):
    return OFFSET + np.array([0.02, -0.01, 0.03]) * e        # a different target per env


@pytest.mark.parametrize("K,D", GAINS)
def test_cartesian_chain_follows_recurrence(gym, tmp_path, cart_plain, K, D):
    """Test 1: the attractor in the ABA (k_artic_lanes; the chain would step in
    k_artic_chain without it). Envs 1 and 4 carry none and stay bit-identical to
    the attractor-free sim."""
    owners = (0, 2, 3)
    sim = cart_scene(gym, tmp_path, {e: (K, D, gymapi.AXIS_TRANSLATION, env_offset(e), None) for e in owners})
    pos, dof, rb = run_frames(gym, sim, 120)
    assert N.lib.mg_num_attractors(sim.native) == 3
    assert N.lib.mg_step_out_supported(sim.native) == 0
    gym.destroy_sim(sim)
    assert np.isfinite(pos).all() and np.isfinite(rb).all()
    for e in owners:
        ref = recurrence(CART_M, K, D, [0.0, 0.0, G_Z], env_offset(e), 120)
        err, tol = close(pos[:, 3 * e:3 * e + 3], ref)
        print("env %d K %g: max err %.3g m (max |x| %.3g)" % (e, K, err.max(), np.abs(ref).max()))
        assert (err <= tol).all(), "env %d: max error %g m over the bound by %g" % (e, err.max(), (err - tol).max())
    if K == 200.0:      # the soft pair overshoots the 0.3 m step on the light axis: a real transient
        assert recurrence(0.5, K, D, 0.0, 0.3, 120).max() > 0.38
    ppos, pdof, prb = cart_plain
    for e in (1, 4):
        assert np.array_equal(pos[:, 3 * e:3 * e + 3], ppos[:, 3 * e:3 * e + 3])
        assert np.array_equal(dof[3 * e:3 * e + 3], pdof[3 * e:3 * e + 3])
        assert np.array_equal(rb[4 * e:4 * e + 4], prb[4 * e:4 * e + 4])


def test_small_coupled_env(gym, tmp_path):
    """A coupled env of at most 4 links: the narrow phase runs in its 4-link
    build, the step in the 16-link attractor build (mg_launch_env_step)."""
    K, D = GAINS[0]
    sim = cart_scene(gym, tmp_path, {e: (K, D, gymapi.AXIS_TRANSLATION, env_offset(e), None) for e in (0, 2)},
                     num_envs=3, coupled=True)
    assert N.lib.mg_num_coupled_envs(sim.native) == 3
    pos, _, rb = run_frames(gym, sim, 120)
    gym.destroy_sim(sim)
    assert np.isfinite(pos).all() and np.isfinite(rb).all()
    for e, k in ((0, K), (1, 0.0), (2, K)):          # env 1: no attractor, free fall
        ref = recurrence(CART_M, k, D if k else 0.0, [0.0, 0.0, G_Z], env_offset(e), 120)
        err, tol = close(pos[:, 3 * e:3 * e + 3], ref)
        print("coupled env %d: max err %.3g m" % (e, err.max()))
        assert (err <= tol).all(), "env %d: max error %g m" % (e, err.max())


def test_axis_mask_and_target_frame(gym, tmp_path):
    """Test 2: axes select rows in the target frame. AXIS_X | AXIS_Z leaves y
    free (it coasts at its start velocity); with the target turned 90 degrees
    about z, AXIS_X pulls along world y."""
    K, D = GAINS[0]
    vy = 0.5
    rz = gymapi.Quat(0.0, 0.0, math.sin(math.pi / 4), math.cos(math.pi / 4))
    sim = cart_scene(gym, tmp_path, {0: (K, D, gymapi.AXIS_X | gymapi.AXIS_Z, OFFSET, None),
                                     1: (K, D, gymapi.AXIS_X, OFFSET, rz)}, y_vel=vy, num_envs=2)
    pos, _, _ = run_frames(gym, sim, 120)
    gym.destroy_sim(sim)
    g = [0.0, 0.0, G_Z]
    ref0 = recurrence(CART_M, [K, 0.0, K], [D, 0.0, D], g, OFFSET, 120, v0=[0.0, vy, 0.0])
    ref1 = recurrence(CART_M, [0.0, K, 0.0], [0.0, D, 0.0], g, OFFSET, 120, v0=[0.0, vy, 0.0])
    for e, ref in ((0, ref0), (1, ref1)):
        err, tol = close(pos[:, 3 * e:3 * e + 3], ref)
        print("env %d: max err per axis %s" % (e, err.max(0)))
        assert (err <= tol).all(), "env %d: max error %g m" % (e, err.max())
    assert abs(ref0[-1, 1] - 2.0 * vy) < 1e-9 and abs(ref1[-1, 0]) == 0.0


# ----------------------------------------------------------------- free bodies
def box_scene(gym, num_envs, attrs, gravity=(0.0, 0.0, G_Z), mass=0.5, per_row=9, spacing=0.5):
    """One free box per env, no ground, no damping. attrs: env -> AttractorProperties
    factory taking the body handle and the body's env-frame start position."""
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params(gravity))
    opts = gymapi.AssetOptions()
    opts.linear_damping = 0.0
    opts.angular_damping = 0.0
    opts.max_linear_velocity = 1000.0
    opts.max_angular_velocity = 1000.0
    asset = gym.create_box(sim, 0.1, 0.1, 0.1, opts)
    lo, hi = gymapi.Vec3(-0.5 * spacing, -0.5 * spacing, 0.0), gymapi.Vec3(0.5 * spacing, 0.5 * spacing, spacing)
    start = np.array([0.0, 0.0, 1.0])
    inertia = None
    for i in range(num_envs):
        env = gym.create_env(sim, lo, hi, per_row)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(*start)
        h = gym.create_actor(env, asset, pose, "box", i, 0)
        bp = gym.get_actor_rigid_body_properties(env, h)
        bp[0].mass = mass
        gym.set_actor_rigid_body_properties(env, h, bp, True)
        inertia = gym.get_actor_rigid_body_properties(env, h)[0].inertia.x.x
        if i in attrs:
            assert gym.create_rigid_body_attractor(env, attrs[i](gym.get_actor_rigid_body_handle(env, h, 0), start)) == 0
    gym.prepare_sim(sim)
    return sim, inertia


def run_rb(gym, sim, frames):
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    gym.refresh_rigid_body_state_tensor(sim)
    out = [rb.cpu().numpy().copy()]
    for _ in range(frames):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_rigid_body_state_tensor(sim)
        out.append(rb.cpu().numpy().copy())
    return np.array(out)          # [frames + 1, nb, 13], row 0 the start


@pytest.fixture(scope="module")
def boxes_plain():
    gym = gymapi.acquire_gym()
    sim, _ = box_scene(gym, 65, {})
    out = run_rb(gym, sim, 120)
    gym.destroy_sim(sim)
    return out


@pytest.mark.parametrize("K,D", GAINS)
def test_free_bodies_follow_recurrence(gym, boxes_plain, K, D):
    """Test 3: 65 free boxes (one full wavefront and one lane), attractors on
    envs 0, 63 and 64 at the COM; the other 62 stay bit-identical to the
    attractor-free sim."""
    owners = (0, 63, 64)
    mk = lambda h, start: attractor(h, K, D, gymapi.AXIS_TRANSLATION, start + OFFSET)   # noqa: E731
    sim, _ = box_scene(gym, 65, {e: mk for e in owners})
    st = run_rb(gym, sim, 120)
    gym.destroy_sim(sim)
    assert np.isfinite(st).all()
    ref = recurrence(0.5, K, D, [0.0, 0.0, G_Z], OFFSET, 120)
    for e in owners:
        disp = st[1:, e, 0:3].astype(np.float64) - st[0, e, 0:3].astype(np.float64)
        err, tol = close(disp, ref)
        print("env %d K %g: max err %.3g m" % (e, K, err.max()))
        assert (err <= tol).all(), "env %d: max error %g m" % (e, err.max())
    others = [e for e in range(65) if e not in owners]
    assert np.array_equal(st[:, others], boxes_plain[:, others])


def _rotvec_in(q_t, q_a):
    """R_t^T rotvec(q_t * q_a^-1), float64 (xyzw)."""
    def mul(a, b):
        return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                         a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                         a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                         a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    qt, qa = np.float64(q_t), np.float64(q_a)
    conj = lambda q: np.array([-q[0], -q[1], -q[2], q[3]])     # noqa: E731
    d = mul(qt, conj(qa))
    if d[3] < 0:
        d = -d
    n = np.linalg.norm(d[:3])
    phi = d[:3] * (2.0 * math.atan2(n, d[3]) / n) if n > 0 else np.zeros(3)
    # into the target frame: q_t^-1 phi q_t
    p = mul(mul(conj(qt), np.array([*phi, 0.0])), qt)
    return p[:3]


def test_rotation_rows():
    """Test 4: rotation rows on a free cube, gravity off. AXIS_ROTATION at
    critical damping turns the cube onto a target 0.5 rad about a principal
    axis without moving its COM; AXIS_TWIST alone leaves a tilt about the
    target's y untouched."""
    gym = gymapi.acquire_gym()
    K = 50.0
    qz = gymapi.Quat(0.0, 0.0, math.sin(0.25), math.cos(0.25))
    qy = gymapi.Quat(0.0, math.sin(0.2), 0.0, math.cos(0.2))
    sim, inertia = box_scene(gym, 1, {}, gravity=(0.0, 0.0, 0.0))
    gym.destroy_sim(sim)
    D = 2.0 * math.sqrt(K * inertia)
    sim, _ = box_scene(gym, 2, {0: lambda h, s: attractor(h, K, D, gymapi.AXIS_ROTATION, s, qz),
                                1: lambda h, s: attractor(h, K, D, gymapi.AXIS_TWIST, s, qy)},
                       gravity=(0.0, 0.0, 0.0))
    st = run_rb(gym, sim, 240)
    gym.destroy_sim(sim)
    assert np.isfinite(st).all()
    err = np.linalg.norm(_rotvec_in([qz.x, qz.y, qz.z, qz.w], st[-1, 0, 3:7]))
    moved = np.abs(st[:, 0, 0:3].astype(np.float64) - st[0, 0, 0:3].astype(np.float64)).max()
    print("rotation: final error %.3g rad, COM moved %.3g m, D %.4g" % (err, moved, D))
    assert err < 1e-3
    assert moved < 1e-6
    # a real turn, not a start on the target
    assert np.linalg.norm(_rotvec_in([qz.x, qz.y, qz.z, qz.w], st[0, 0, 3:7])) == pytest.approx(0.5, abs=1e-6)
    e0 = _rotvec_in([qy.x, qy.y, qy.z, qy.w], st[0, 1, 3:7])
    e1 = _rotvec_in([qy.x, qy.y, qy.z, qy.w], st[-1, 1, 3:7])
    print("twist only: error about the target's y %.7g -> %.7g" % (e0[1], e1[1]))
    assert e0[1] == pytest.approx(0.4, abs=1e-6)
    assert abs(e1[1] - e0[1]) < 1e-6


# ----------------------------------------------------------------- Franka
def script_franka_scene(gym, num_envs=5):
    """examples/franka_attractor.py:39-183 as data: y-up, a fixed-base Franka
    turned onto the y axis, every DOF at kp = kd = 1000, position drives on the
    first two joints and (1e10 / 1) on the fingers, the mid-range start pose."""
    sp = gymapi.SimParams()
    sp.dt = 1.0 / 60.0
    sp.substeps = 2
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 4
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.flip_visual_attachments = True
    opts.armature = 0.01
    opts.default_dof_drive_mode = gymapi.DOF_MODE_NONE      # joints 3-7: no drive (the bound's two-drive load)
    asset = gym.load_asset(sim, scenes.ASSET_ROOT, "franka/franka_proxy.urdf", opts)
    assert asset is not None
    props = gym.get_asset_dof_properties(asset)
    mids = 0.5 * (props["upper"] + props["lower"])
    props["stiffness"].fill(1000.0)
    props["damping"].fill(1000.0)
    props["driveMode"][0:2] = gymapi.DOF_MODE_POS
    props["driveMode"][7:] = gymapi.DOF_MODE_POS
    props["stiffness"][7:] = 1e10
    props["damping"][7:] = 1.0
    lo, hi = gymapi.Vec3(-1.0, 0.0, -1.0), gymapi.Vec3(1.0, 1.0, 1.0)
    pose = gymapi.Transform()
    pose.r = gymapi.Quat(-0.707107, 0.0, 0.0, 0.707107)
    envs, hands = [], []
    for i in range(num_envs):
        env = gym.create_env(sim, lo, hi, 2)
        h = gym.create_actor(env, asset, pose, "franka", i, 2)
        gym.set_actor_dof_properties(env, h, props)
        st = gym.get_actor_dof_states(env, h, gymapi.STATE_NONE)
        st["pos"][:] = mids
        gym.set_actor_dof_states(env, h, st, gymapi.STATE_POS)
        envs.append(env)
        hands.append(gym.find_actor_rigid_body_handle(env, h, "panda_hand"))
    return sim, envs, hands


def hand_errors(rb, hand_rows, targets):
    """(distance m, angle rad, speed m/s) of each hand against its global target."""
    d, a, v = [], [], []
    for row, (tp, tq) in zip(hand_rows, targets):
        d.append(np.linalg.norm(rb[row, 0:3].astype(np.float64) - tp))
        a.append(np.linalg.norm(_rotvec_in(tq, rb[row, 3:7])))
        v.append(np.linalg.norm(rb[row, 7:10].astype(np.float64)))
    return np.array(d), np.array(a), np.array(v)


def reach(gym, sim, envs, hands, hand_rows, off=(0.05, -0.05, 0.05), frames=120):
    """Attractors (5e5 / 5e3, all axes) on the hands, targets the start hand
    poses plus `off`; steps `frames`. Returns (state, global targets, env-frame
    targets)."""
    tgt_env, tgt_glob = [], []
    for env, hand in zip(envs, hands):
        t = gym.get_rigid_transform(env, hand)                    # global frame
        o = env.origin
        tl = gymapi.Transform(gymapi.Vec3(t.p.x - o[0] + off[0], t.p.y - o[1] + off[1], t.p.z - o[2] + off[2]), t.r)
        assert gym.create_rigid_body_attractor(env, attractor(hand, 5e5, 5e3, gymapi.AXIS_ALL,
                                                              (tl.p.x, tl.p.y, tl.p.z), tl.r)) == 0
        tgt_env.append(tl)
        tgt_glob.append((np.array([t.p.x + off[0], t.p.y + off[1], t.p.z + off[2]]), [t.r.x, t.r.y, t.r.z, t.r.w]))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    for _ in range(frames):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
    gym.refresh_rigid_body_state_tensor(sim)
    return rb, tgt_glob, tgt_env


def test_franka_uncoupled_reaches_and_tracks():
    """Test 5: the script's scene (k_artic_lanes; the kp = 1000 drives make the
    effort-limit re-solve run). Bounds, derived: the opposing load is the two
    kp = 1000 joint drives at up to 1 rad over a ~0.5 m lever, ~2 kN, i.e. 4 mm
    at K = 5e5, plus the arm's weight at 0.4 mm, rounded up 2x: 10 mm, 0.02 rad;
    then the target moves along the script's circle (:164-166, its radii and
    rates, laid through the reached target so that it moves continuously) at
    0.3 - 0.4 m/s, the lag bounded by D / K = 10 ms, 3 - 4 mm, plus the static
    offset: 30 mm."""
    gym = gymapi.acquire_gym()
    sim, envs, hands = script_franka_scene(gym)
    gym.prepare_sim(sim)
    nbody = envs[0].num_bodies
    rows = [i * nbody + h for i, h in enumerate(hands)]
    rb, tgt, tgt_env = reach(gym, sim, envs, hands, rows)
    st = rb.cpu().numpy()
    dofs = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    gym.refresh_dof_state_tensor(sim)
    assert np.isfinite(st).all() and np.isfinite(dofs.cpu().numpy()).all()
    d, a, v = hand_errors(st, rows, tgt)
    print("franka reach: distance %s m, angle %s rad, speed %s m/s" % (d, a, v))
    assert (d < 0.010).all() and (a < 0.02).all() and (v < 0.05).all()

    n = len(envs)

    def circle(t, i):       # franka_attractor.py:164-166
        ph = math.pi * float(i) / n
        return np.array([0.2 * math.sin(1.5 * t - ph), 0.7 + 0.1 * math.cos(2.5 * t - ph), 0.2 * math.cos(1.5 * t - ph)])

    # env i enters the circle at the time t0 its x is largest (1.5 t0 - ph = pi / 2),
    # so that the path heads towards the base and stays within the arm's reach
    t0 = [(0.5 * math.pi + math.pi * float(i) / n) / 1.5 for i in range(n)]
    worst = 0.0
    for f in range(1, 61):
        t = f / 60.0
        cur = []
        for i, env in enumerate(envs):
            step = circle(t0[i] + t, i) - circle(t0[i], i)
            pose = gym.get_attractor_properties(env, 0).target
            base = tgt_env[i].p
            pose.p = gymapi.Vec3(base.x + step[0], base.y + step[1], base.z + step[2])
            gym.set_attractor_target(env, 0, pose)
            cur.append((tgt[i][0] + step, tgt[i][1]))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_rigid_body_state_tensor(sim)
        st = rb.cpu().numpy()
        assert np.isfinite(st).all()
        d, _, _ = hand_errors(st, rows, cur)
        worst = max(worst, d.max())
    gym.destroy_sim(sim)
    print("franka track: worst distance to the moving target %.4g m" % worst)
    assert worst < 0.030


def test_franka_uncoupled_script_circle():
    """The script's own circle (:164-166: centre (0, 0.7, 0) in the env's frame,
    the hand orientation of the arm as created, all DOFs 0, which the script's
    attractor keeps), entered as the script does, by a jump: about 0.5 - 0.7 m
    from the reached target. The joints' speed limits (2.175 rad/s over a ~0.5
    m lever, ~1 m/s at the hand) bound the catch-up at 0.7 s, rounded up to 60
    frames; over the next 60 the hand must stay within the 30 mm of test 5.
    (Further round the circle each arm crosses a stretch where it falls up to
    36 mm / 0.1 rad behind and recovers; not asserted.)"""
    gym = gymapi.acquire_gym()
    sim, envs, hands = script_franka_scene(gym)
    a = envs[0].actors[0]
    keep = a.dof_state.copy()
    a.dof_state[:] = 0.0
    _, qs = sim.actor_world_body_poses(a)
    a.dof_state[:] = keep
    q0 = gymapi.Quat(*[float(c) for c in qs[hands[0]]])
    gym.prepare_sim(sim)
    n, nbody = len(envs), envs[0].num_bodies
    rows = [i * nbody + h for i, h in enumerate(hands)]
    rb, _, _ = reach(gym, sim, envs, hands, rows)
    worst = 0.0
    for f in range(1, 121):
        t = 1.5 + f / 60.0                      # the script starts moving the targets at t = 1.5 s
        cur = []
        for i, env in enumerate(envs):
            ph = math.pi * float(i) / n
            c = np.array([0.2 * math.sin(1.5 * t - ph), 0.7 + 0.1 * math.cos(2.5 * t - ph),
                          0.2 * math.cos(1.5 * t - ph)])
            gym.set_attractor_target(env, 0, gymapi.Transform(gymapi.Vec3(*c), q0))
            cur.append((c + env.origin, [q0.x, q0.y, q0.z, q0.w]))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_rigid_body_state_tensor(sim)
        st = rb.cpu().numpy()
        assert np.isfinite(st).all()
        if f > 60:
            d, _, _ = hand_errors(st, rows, cur)
            worst = max(worst, d.max())
    gym.destroy_sim(sim)
    print("franka script circle: worst distance after the catch-up %.4g m" % worst)
    assert worst < 0.030


def test_franka_coupled_reaches_cube_untouched():
    """Test 6: the cube-pick scene (k_env_step): the hand reaches a target above
    the table, the cube, never touched, stays bit-identical to a run without
    attractors. The target lies 8 cm towards the base and 8 cm below the start
    hand pose (0.45, 0, 0.85), 0.37 m above the table top: with the hand's
    orientation held, a target further out than the start is beyond the arm's
    reach (the attractor then settles at the nearest pose, 49 mm short)."""
    gym = gymapi.acquire_gym()
    sim0, info0 = scenes.franka_scene(gym, 5)
    gym.prepare_sim(sim0)
    rb0 = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim0))
    for _ in range(120):
        gym.simulate(sim0)
        gym.fetch_results(sim0, True)
    gym.refresh_rigid_body_state_tensor(sim0)
    plain = rb0.cpu().numpy().copy()
    gym.destroy_sim(sim0)

    sim, info = scenes.franka_scene(gym, 5)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == 5
    envs = info["envs"]
    hands = [gym.find_actor_rigid_body_handle(e, 2, "panda_hand") for e in envs]
    rb, tgt, _ = reach(gym, sim, envs, hands, info["hand_idxs"], off=(-0.08, -0.05, -0.08))
    st = rb.cpu().numpy()
    gym.destroy_sim(sim)
    assert np.isfinite(st).all()
    d, a, v = hand_errors(st, info["hand_idxs"], tgt)
    print("coupled franka reach: distance %s m, angle %s rad, speed %s m/s" % (d, a, v))
    assert (d < 0.010).all() and (a < 0.02).all() and (v < 0.05).all()
    # the hand is above the table top and far from the cube
    box = st[info["box_idxs"], 0:3]
    hand = st[info["hand_idxs"], 0:3]
    assert (np.linalg.norm(hand - box, axis=1) > 0.15).all()
    assert np.array_equal(st[info["box_idxs"]], plain[info["box_idxs"]])


# ----------------------------------------------------------------- refusals
def _refused_then_usable(gym, sim, env, body_handle):
    p = attractor(body_handle, 200.0, 4.0, gymapi.AXIS_TRANSLATION, (0.0, 0.5, 0.0))
    assert gym.create_rigid_body_attractor(env, p) == 0
    with pytest.raises(N.MigymError, match="attractor"):
        gym.simulate(sim)
    N.check(N.lib.mg_set_attractors(sim.native, None, 0), "mg_set_attractors")
    assert N.lib.mg_num_attractors(sim.native) == 0
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    gym.refresh_rigid_body_state_tensor(sim)
    assert torch.isfinite(rb).all()


def test_refused_on_pile_body(gym):
    """Test 7a: a pile env's body cannot carry an attractor: simulate says so."""
    sim, envs = scenes.ball_pile_scene(gym, 1)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_pile_envs(sim.native) == 1
    _refused_then_usable(gym, sim, envs[0], 3)
    gym.destroy_sim(sim)


def test_refused_on_coupled_free_body(gym):
    """Test 7b: nor can a free body of a coupled env (the cube of the pick scene)."""
    sim, info = scenes.franka_scene(gym, 2)
    gym.prepare_sim(sim)
    env = info["envs"][0]
    _refused_then_usable(gym, sim, env, gym.get_actor_rigid_body_handle(env, 1, 0))
    gym.destroy_sim(sim)


def test_capi_validation(gym):
    """mg_set_attractors: body range, one attractor per body, gains."""
    sim, _ = box_scene(gym, 2, {})
    tab = (N.MgAttractor * 2)()
    for r in tab:
        r.axes, r.stiffness, r.damping = 7, 1.0, 1.0
        r.offset_q[3] = r.target_q[3] = 1.0
    tab[0].body, tab[1].body = 0, 5
    assert N.lib.mg_set_attractors(sim.native, tab, 2) == -1                  # MG_ERR_ARG: body out of range
    tab[1].body = 0
    assert N.lib.mg_set_attractors(sim.native, tab, 2) == -4                  # MG_ERR_UNSUPPORTED: second on a body
    assert "attractor" in N.last_error()
    tab[1].body, tab[1].stiffness = 1, -1.0
    assert N.lib.mg_set_attractors(sim.native, tab, 2) == -1
    tab[1].stiffness = float("nan")
    assert N.lib.mg_set_attractors(sim.native, tab, 2) == -1
    assert N.lib.mg_num_attractors(sim.native) == 0                           # a refused table changes nothing
    tab[1].stiffness = 1.0
    assert N.lib.mg_set_attractors(sim.native, tab, 2) == 0
    assert N.lib.mg_num_attractors(sim.native) == 2
    pose = np.zeros((2, 7), dtype=np.float32)
    pose[:, 6] = 1.0
    assert N.lib.mg_set_attractor_targets(sim.native, pose.ctypes.data, 1, 2) == -1   # past the table
    assert N.lib.mg_set_attractor_targets(sim.native, pose.ctypes.data, 0, 2) == 0
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.destroy_sim(sim)
