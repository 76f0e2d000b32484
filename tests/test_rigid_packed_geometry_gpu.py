"""GPU parity of the one-round free-body step with its geometry on packed f32
pairs (mg_rigid.hip ground_patch_update_pk and the pair helpers of mg_pair.h,
DESIGN.md §3.2): each half of a packed operation is the scalar form's correctly
rounded operation, so every build still equals the oracle bit for bit. The
method of tests/test_rigid_box_only_gpu.py: the oracle (oracle/migym_oracle.c,
its contact cache kept from step to step) is stepped beside the GPU sim and the
rigid-body state, the root state and the net contact force are compared with
np.array_equal every frame; mg_last_rigid_form says which build ran.

  - box-only: the servo scene at 1 env (62 dead lanes), 33 and 96 envs, 20
    frames of teleports, then the vehicles set down and 20 frames of rest:
    record + box-only;
  - general shapes: a vehicle and a ball per env, 33 envs: the record build;
  - general ground basis: a vehicle and a ball per env on a y-up ground
    (tests/rigid_pair_scenes.py), 33 envs: the record build over the general
    basis (the packed patch update with the scalar rows);
  - a vehicle beside a box whose inertial frame is displaced and turned
    (non-zero com, non-identity iq): tests/golden/offcentre_box.urdf, a plain
    box, so record + box-only, and tests/golden/offcentre_posed_box.urdf, the
    same with its shape posed against the link frame: the record build;
  - held anchors, then slip: the servo scene's vehicles set down, 30 frames at
    rest (every vehicle then holds two anchors), then a tangential velocity
    that slides them for 10 frames (anchors dropped and regrown): record + box;
  - wide control: the servo scene above one resident round, 6 frames of
    teleports: the wide form, whose code is the scalar one.

The attractor and reporting builds keep the scalar geometry (their tests are
tests/test_attractor_gpu.py and tests/test_contact_list_gpu.py).
"""
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
SEED = 59
TELEPORTS, REST = 20, 20
NO_DOF = np.zeros((0, 2), np.float32)
REC = N.MG_RIGID_FORM_REC
REC_BOX = N.MG_RIGID_FORM_REC | N.MG_RIGID_FORM_BOX

_REF = {}


def _qmul(a, b):
    """Hamilton product of (x, y, z, w) rows."""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz],
                    axis=-1).astype(np.float32)


def _build(gym, kind, n):
    """(sim, up axis, [(actor rows, rest height)]): the bodies that are set down."""
    if kind == "yup_ball":
        sim, veh, ball = PS.build_yup_ball(gym, n)
        return sim, 1, [(veh, 1.4), (ball, 0.25)]
    if kind in ("offcentre", "offcentre_posed"):
        sim, veh, _ = RS.build(gym, "other", n, other=PS.OFFCENTRE if kind == "offcentre" else PS.OFFCENTRE_POSED)
        return sim, 2, [(veh, 1.4), (veh + 1, 1.05)]
    sim, veh, ball = RS.build(gym, kind, n)
    return sim, 2, [(veh, 1.4)] + ([(ball, 0.25)] if len(ball) else [])


def _set_down(up, low, yaw_quats):
    """Root-state writes that put the bodies of `low` just above their rest
    heights, at rest; the first group (the vehicles) upright at the yaws given
    (yaw_quats: rotations about z)."""
    sets = []
    for i, (rows, height) in enumerate(low):
        sets.append((rows, up, up + 1, np.full((len(rows), 1), height, np.float32)))
        if i == 0:
            q = yaw_quats if up == 2 else _qmul(np.asarray(PS.UPRIGHT, np.float32)[None, :], yaw_quats)
            sets.append((rows, 3, 7, q))
        sets.append((rows, 7, 13, np.zeros((len(rows), 6), np.float32)))
    return sets


def _script(kind, n, plan, low, up):
    """Per frame, the root-state writes made before the step: a list of
    (actor rows, first column, end column, values)."""
    every = np.arange(2 * n, dtype=np.int64)
    if plan == "teleports_rest":
        acts = scenes.servo_actions(n, TELEPORTS, "cpu", seed=SEED).numpy()
        frames = [[(every, 3, 10, acts[k])] for k in range(TELEPORTS)]
        frames.append(_set_down(up, low, acts[-1][1::2, 0:4]))
        return frames + [[] for _ in range(REST - 1)]
    if plan == "teleports":
        acts = scenes.servo_actions(n, 6, "cpu", seed=SEED).numpy()
        return [[(every, 3, 10, acts[k])] for k in range(6)]
    assert plan == "rest_slip"
    acts = scenes.servo_actions(n, 2, "cpu", seed=SEED).numpy()
    frames = [_set_down(up, low, acts[0][1::2, 0:4])] + [[] for _ in range(29)]
    # horizontal velocities of 2 to 6 m/s in the actions' random directions
    v = acts[1][1::2, 4:6]
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (2.0 + 4.0 * np.abs(acts[1][1::2, 6:7]) / 50.0)
    frames.append([(low[0][0], 7, 9, v.astype(np.float32))])
    return frames + [[] for _ in range(9)]


def _reference(gym, kind, n, plan):
    """The oracle's trajectory: per frame the body states and the net contact
    forces, and the anchor counts of the contact cache after each frame.
    Computed once per case, read-only."""
    key = (kind, n, plan)
    if key not in _REF:
        sim, up, low = _build(gym, kind, n)
        gym.prepare_sim(sim)
        p, m = sim.mg_params(), sim.mg_model()
        cc = oracle.contact_cache(m)
        st = sim.model_arrays["body_state0"].copy()
        roots = sim.model_arrays["actor_root_body"]
        frames = []
        for sets in _script(kind, n, plan, low, up):
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


def _run(gym, kind, n, plan, want_form):
    frames = _reference(gym, kind, n, plan)
    sim, up, low = _build(gym, kind, n)
    gym.prepare_sim(sim)
    gym.set_step_fusion(sim, gymapi.STEP_FUSION_ALL)
    roots = sim.model_arrays["actor_root_body"]
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    gym.refresh_actor_root_state_tensor(sim)
    assert N.lib.mg_last_rigid_form(sim.native) == -1
    for k, (sets, (st, cf, _)) in enumerate(zip(_script(kind, n, plan, low, up), frames)):
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
    return frames, roots, low


def _touched(frames):
    """Some body carried a contact force in some frame: the case did run the patch update."""
    return any(np.any(cf != 0.0) for _, cf, _ in frames)


@pytest.mark.parametrize("n", [1, 33, 96])
def test_servo_box_only_bitexact(gym, n):
    frames, _, _ = _run(gym, "servo", n, "teleports_rest", REC_BOX)
    assert _touched(frames[TELEPORTS:])


def test_vehicle_and_ball_general_shapes_bitexact(gym):
    frames, _, _ = _run(gym, "ball", 33, "teleports_rest", REC)
    assert _touched(frames[TELEPORTS:])


def test_yup_ground_general_basis_bitexact(gym):
    frames, roots, low = _run(gym, "yup_ball", 33, "teleports_rest", REC)
    # at rest on the +y ground: every vehicle's patch holds two anchors
    assert np.all(frames[-1][2][roots[low[0][0]]] == 2.0)


@pytest.mark.parametrize("kind,form", [("offcentre", REC_BOX), ("offcentre_posed", REC)])
def test_offcentre_inertial_frame_bitexact(gym, kind, form):
    """The off-centre box as a plain box (the box-only build: the flag looks at
    the shapes alone) and with its shape posed against the link frame (the
    general record build, the shape's own matrix beside the shared qmat(q))."""
    sim, _, low = _build(gym, kind, 2)
    gym.prepare_sim(sim)
    A = sim.model_arrays
    b = A["actor_root_body"][low[1][0][0]]
    mass = A["body_mass"][b]
    gym.destroy_sim(sim)
    assert np.any(mass[4:7] != 0.0) and mass[7] != 1.0, "the asset's principal frame is the identity"
    assert np.any(mass[8:11] != 0.0), "the asset's centre of mass is the body origin"
    frames, roots, low = _run(gym, kind, 33, "teleports_rest", form)
    box = roots[low[1][0]]
    assert all(np.any(cf[box] != 0.0) for _, cf, _ in frames[TELEPORTS:])   # the off-centre boxes stay in contact
    assert np.any(frames[-1][2][box] == 2.0)


def test_held_anchors_then_slip_bitexact(gym):
    frames, roots, low = _run(gym, "servo", 33, "rest_slip", REC_BOX)
    veh = roots[low[0][0]]
    assert np.all(frames[29][2][veh] == 2.0)               # every vehicle rests on two anchors
    moved = np.linalg.norm(frames[-1][0][veh, 0:2] - frames[29][0][veh, 0:2], axis=1)
    assert np.all(moved > 0.05), moved                     # past the correlation distance: anchors regrown
    assert np.all(frames[30][2][veh] == 0.0)               # sliding: the patch lets go at each substep's end
    assert np.any(frames[-1][2][veh] == 2.0)               # and holds again where a vehicle has come to rest


def test_wide_control_bitexact(gym):
    """More waves than one resident round (4 SIMDs x 2 waves per CU): the wide
    form, which keeps the scalar geometry."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 4 * 2 * 64 // 2 + 64
    _run(gym, "servo", n, "teleports", N.MG_RIGID_FORM_WIDE)
