"""GPU parity of the one-round +Z free-body step whose solver loops run two
sweeps per trip and whose rows' effective masses come from the paired
reciprocal on every lane (mg_rigid.hip tgs_zp and the packed row constants,
MG_RIGID1_SWEEP_PAIRS / MG_RIGID1_RECIP_PAIRS). The method of
tests/test_rigid_packed_geometry_gpu.py: the oracle, its contact cache kept from
step to step, is stepped beside the GPU sim; the rigid-body state, the root
state and the net contact force are compared with np.array_equal every frame,
and mg_last_rigid_form says which build ran.

  - iteration counts: the servo scene at 1 env (62 dead lanes) and 33 envs,
    record + box-only, with (position, velocity) iterations (1,0) (1,1) (2,1)
    (3,1) (4,1) (5,2) (6,1) (7,0): only the opening sweep, both parities of the
    pair loop's remainder, no / one / two velocity sweeps. 8 frames of
    teleports, the vehicles set down and 8 frames of rest, then 6 frames slid
    tangentially (anchors held, dropped and regrown);
  - one wave with every contact state: 8 envs at TGS 6/1, 12 frames, the
    vehicles far above the ground, just above it, on a corner, on an edge and
    flat (0 slots, 0 slots but not far, 1, 2 and 4: the selects that took the
    exec brackets' place); the oracle's cache holds 0, 1 and 2 anchors;
  - masses: the edge and flat placements with every vehicle's mass set to
    1e-3, 1 and 1e4 kg through the rigid-body properties;
  - controls that the change must not touch: the vehicle-and-ball record build
    (general shapes), the y-up general-basis build, one wide launch.
"""
import math

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N, scenes
import oracle
import rigid_box_scenes as RS
import rigid_pair_scenes as PS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 67
NO_DOF = np.zeros((0, 2), np.float32)
REC = N.MG_RIGID_FORM_REC
REC_BOX = N.MG_RIGID_FORM_REC | N.MG_RIGID_FORM_BOX
WIDE = N.MG_RIGID_FORM_WIDE
HALF = np.array([3.75, 1.5, 1.25])     # assets/servo/ground_vehicle.urdf: box 7.5 x 3 x 2.5
ITERS = [(1, 0), (1, 1), (2, 1), (3, 1), (4, 1), (5, 2), (6, 1), (7, 0)]
TELEPORTS, REST, SLIDE = 8, 8, 6
SET_DOWN = 1.255                       # the vehicles' origin when set down: 5 mm above the ground

_REF = {}


def _servo(gym, n, npos=6, nvel=1, mass=None):
    """scenes.servo_scene (UAV then vehicle per env) with the solver's
    iteration counts and, optionally, every vehicle's mass set."""
    sp = scenes.servo_sim_params(True)
    sp.physx.num_position_iterations = npos
    sp.physx.num_velocity_iterations = nvel
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    plane.distance = 0
    plane.static_friction = 1
    plane.dynamic_friction = 1
    plane.restitution = 0
    gym.add_ground(sim, plane)
    opts = gymapi.AssetOptions()
    opts.armature = 0.01
    uav = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/uav.urdf", opts)
    veh = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/ground_vehicle.urdf", opts)
    assert uav is not None and veh is not None
    lower, upper = gymapi.Vec3(-20.0, -20.0, -20.0), gymapi.Vec3(20.0, 20.0, 20.0)
    for e in range(n):
        env = gym.create_env(sim, lower, upper, int(math.sqrt(n)))
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(-10.0, 0.0, 102.0)
        gym.create_actor(env, uav, pose, "uav%d" % e, e, -1)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 0.0, 2.0)
        h = gym.create_actor(env, veh, pose, "veh%d" % e, e, -1)
        if mass is not None:
            props = gym.get_actor_rigid_body_properties(env, h)
            props[0].mass = mass
            assert gym.set_actor_rigid_body_properties(env, h, props, recomputeInertia=True)
    return sim


def _build(gym, kind, n, npos, nvel, mass):
    """(sim, up axis, vehicle actor rows, [(actor rows, rest height)])."""
    if kind == "yup_ball":
        sim, veh, ball = PS.build_yup_ball(gym, n)
        return sim, 1, veh, [(veh, SET_DOWN), (ball, 0.25)]
    if kind == "ball":
        sim, veh, ball = RS.build(gym, "ball", n)
        return sim, 2, veh, [(veh, SET_DOWN), (ball, 0.25)]
    veh = 2 * np.arange(n, dtype=np.int64) + 1
    return _servo(gym, n, npos, nvel, mass), 2, veh, [(veh, SET_DOWN)]


def _qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz],
                    axis=-1).astype(np.float32)


def _set_down(up, low, yaw_quats):
    sets = []
    for i, (rows, height) in enumerate(low):
        sets.append((rows, up, up + 1, np.full((len(rows), 1), height, np.float32)))
        if i == 0:
            q = yaw_quats if up == 2 else _qmul(np.asarray(PS.UPRIGHT, np.float32)[None, :], yaw_quats)
            sets.append((rows, 3, 7, q))
        sets.append((rows, 7, 13, np.zeros((len(rows), 6), np.float32)))
    return sets


def _quat_to(src, dst):
    """The shortest rotation (x, y, z, w) that turns direction src onto dst."""
    a, b = src / np.linalg.norm(src), dst / np.linalg.norm(dst)
    q = np.concatenate([np.cross(a, b), [1.0 + a @ b]])
    return q / np.linalg.norm(q)


def _placements(which):
    """(z of the origin, quaternion) of a vehicle by contact state."""
    down = np.array([0.0, 0.0, -1.0])
    edge = np.array([0.0, HALF[1], -HALF[2]])
    out = {
        "far": (50.0, np.array([0.0, 0.0, 0.0, 1.0])),
        "near": (HALF[2] + 0.05, np.array([0.0, 0.0, 0.0, 1.0])),                  # above contact_offset (0.01)
        "corner": (np.linalg.norm(HALF) + 0.004, _quat_to(HALF * [1, 1, -1], down)),
        "edge": (np.linalg.norm(edge) + 0.004, _quat_to(edge, down)),
        "flat": (HALF[2] + 0.004, np.array([0.0, 0.0, 0.0, 1.0])),
    }
    return out[which]


def _script(kind, n, plan, veh, low, up):
    """Per frame, the root-state writes made before the step: a list of
    (actor rows, first column, end column, values)."""
    every = np.arange(2 * n, dtype=np.int64)
    if plan == "teleports":
        acts = scenes.servo_actions(n, 6, "cpu", seed=SEED).numpy()
        return [[(every, 3, 10, acts[k])] for k in range(6)]
    if plan in ("teleports_rest", "teleports_rest_slide"):
        acts = scenes.servo_actions(n, TELEPORTS + 1, "cpu", seed=SEED).numpy()
        frames = [[(every, 3, 10, acts[k])] for k in range(TELEPORTS)]
        frames.append(_set_down(up, low, acts[TELEPORTS - 1][1::2, 0:4]))
        frames += [[] for _ in range(REST - 1)]
        if plan == "teleports_rest_slide":
            # horizontal velocities of 2 to 6 m/s in the actions' random directions
            v = acts[TELEPORTS][1::2, 4:6]
            v = v / np.linalg.norm(v, axis=1, keepdims=True) * (2.0 + 4.0 * np.abs(acts[TELEPORTS][1::2, 6:7]) / 50.0)
            frames.append([(veh, 7, 9, v.astype(np.float32))])
            frames += [[] for _ in range(SLIDE - 1)]
        return frames
    # the vehicles placed by contact state (plan: the states, repeated over the envs), at rest
    states = [plan[e % len(plan)] for e in range(n)]
    z = np.array([[_placements(s)[0]] for s in states], np.float32)
    q = np.array([_placements(s)[1] for s in states], np.float32)
    first = [(veh, 2, 3, z), (veh, 3, 7, q), (veh, 7, 13, np.zeros((n, 6), np.float32))]
    return [first] + [[] for _ in range(11)]


def _reference(gym, key):
    """The oracle's trajectory: per frame the body states, the net contact
    forces and the anchor counts of its contact cache. Once per case, read-only."""
    if key not in _REF:
        kind, n, plan, npos, nvel, mass = key
        sim, up, veh, low = _build(gym, kind, n, npos, nvel, mass)
        gym.prepare_sim(sim)
        p, m = sim.mg_params(), sim.mg_model()
        assert (p.num_position_iterations, p.num_velocity_iterations) == (npos, nvel) or kind != "servo"
        cc = oracle.contact_cache(m)
        st = sim.model_arrays["body_state0"].copy()
        roots = sim.model_arrays["actor_root_body"]
        frames = []
        for sets in _script(kind, n, plan, veh, low, up):
            for rows, c0, c1, val in sets:
                st[roots[rows], c0:c1] = val
            cf = oracle.step(p, m, st, NO_DOF, contact_cache=cc)
            s, c, a = st.copy(), np.array(cf, copy=True), cc.body[:, 0].copy()
            for arr in (s, c, a):
                arr.setflags(write=False)
            frames.append((s, c, a))
        gym.destroy_sim(sim)
        _REF[key] = frames
    return _REF[key]


def _run(gym, kind, n, plan, want_form, npos=6, nvel=1, mass=None):
    frames = _reference(gym, (kind, n, plan, npos, nvel, mass))
    sim, up, veh, low = _build(gym, kind, n, npos, nvel, mass)
    gym.prepare_sim(sim)
    gym.set_step_fusion(sim, gymapi.STEP_FUSION_ALL)
    roots = sim.model_arrays["actor_root_body"]
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    gym.refresh_actor_root_state_tensor(sim)
    for k, (sets, (st, cf, _)) in enumerate(zip(_script(kind, n, plan, veh, low, up), frames)):
        for rows, c0, c1, val in sets:
            root[torch.as_tensor(rows, device=DEV), c0:c1] = torch.from_numpy(np.ascontiguousarray(val)).to(DEV)
        if sets:
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(root))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        assert N.lib.mg_last_rigid_form(sim.native) == want_form
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        got = rb.cpu().numpy()
        assert np.array_equal(got, st), "frame %d: rigid-body state, max |diff| %g" % (k, np.abs(got - st).max())
        got = root.cpu().numpy()
        assert np.array_equal(got, st[roots]), "frame %d: root state, max |diff| %g" % (k, np.abs(got - st[roots]).max())
        assert np.array_equal(ncf.cpu().numpy(), cf), "frame %d: contact force" % k
    gym.destroy_sim(sim)
    return frames, roots[veh]


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("npos,nvel", ITERS)
def test_iteration_counts_bitexact(gym, n, npos, nvel):
    frames, veh = _run(gym, "servo", n, "teleports_rest_slide", REC_BOX, npos, nvel)
    rest = frames[TELEPORTS:TELEPORTS + REST]
    assert all(np.any(cf[veh] != 0.0) for _, cf, _ in rest[2:])          # set down: the vehicles touch the ground
    assert any(np.any(a[veh] > 0.0) for _, _, a in rest)                 # and hold anchors before they are slid
    moved = np.linalg.norm(frames[-1][0][veh, 0:2] - rest[-1][0][veh, 0:2], axis=1)
    assert np.all(moved > 0.05), moved                                   # slid past the correlation distance


def test_every_contact_state_in_one_wave_bitexact(gym):
    plan = ("far", "near", "corner", "edge", "flat", "corner", "edge", "flat")
    frames, veh = _run(gym, "servo", 8, plan, REC_BOX)
    held = np.stack([a[veh] for _, _, a in frames])                      # [frame, env] anchor counts
    print(held)
    for want in (0.0, 1.0, 2.0):                                         # held anchors of count 0, 1 and 2
        assert np.any(held == want), (want, held)
    assert np.all(held[:, 0] == 0.0)                                     # the far vehicle never touches
    assert np.all(frames[0][1][veh[1]] == 0.0)                           # nor, at first, the near one
    force = np.stack([cf[veh] for _, cf, _ in frames])
    assert all(np.any(force[:, e] != 0.0) for e in range(2, 8))          # corner, edge and flat all do


@pytest.mark.parametrize("mass", [1e-3, 1.0, 1e4])
def test_masses_bitexact(gym, mass):
    frames, veh = _run(gym, "servo", 8, ("edge", "flat"), REC_BOX, mass=mass)
    assert all(np.any(cf[veh] != 0.0) for _, cf, _ in frames[3:])
    assert any(np.any(a[veh] == 2.0) for _, _, a in frames)


def test_control_general_shapes_bitexact(gym):
    frames, _ = _run(gym, "ball", 33, "teleports_rest", REC)
    assert any(np.any(cf != 0.0) for _, cf, _ in frames[TELEPORTS:])


def test_control_yup_general_basis_bitexact(gym):
    frames, _ = _run(gym, "yup_ball", 33, "teleports_rest", REC)
    assert any(np.any(cf != 0.0) for _, cf, _ in frames[TELEPORTS:])


def test_control_wide_bitexact(gym):
    """More waves than one resident round (4 SIMDs x 2 waves per CU): the wide form."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _run(gym, "servo", cus * 4 * 2 * 64 // 2 + 64, "teleports", WIDE)
