"""The rigid contact list on the GPU: the reporting builds of
the free-body, coupled and pile step kernels (mg_rigid.hip, mg_env.hip,
mg_pile.hip, template flag CREP) and the compaction (mg_contact.hip).

The list is checked without an oracle: with substeps = 1 the listed impulses of
a body must sum to that body's row of the net contact force tensor,

    sum over entries with body0 == b of (lambda n + fimp)
  - sum over entries with body1 == b of (lambda n + fimp),   divided by dt.

The tolerance is derived, not measured: 1e-5 * sum |terms| / dt + 1e-6 N
(float32 re-association of at most 48 + 48 terms: 96 * 2^-24 = 6e-6).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
from test_isaacgym_amd import scenes
import pile_scenes as PS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = 1.0 / 60.0
G = 9.8
NBOX = 65            # more than one wavefront
HIGH, HELD, SLID = 7, 11, 12


def _sim(gym, substeps=1):
    sp = gymapi.SimParams()
    sp.dt = DT
    sp.substeps = substeps
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -G)
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 4
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, plane)
    return sim


def _boxes(gym, n=NBOX, reporting=None, max_contacts=0):
    """n unit boxes, one per env, nothing to touch but the ground (uncoupled
    envs: the free-body kernel). Env HIGH starts 5 m up."""
    sim = _sim(gym)
    box = gym.create_box(sim, 1.0, 1.0, 1.0, gymapi.AssetOptions())
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-2, -2, 0), gymapi.Vec3(2, 2, 4), 8)
        z = 5.5 if i == HIGH else 0.5
        gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0, 0, z)), "box", i, 0)
    if reporting is not None:
        gym.set_rigid_contact_reporting(sim, reporting, max_contacts)
    gym.prepare_sim(sim)
    return sim


def _mass_mu(sim):
    A = sim.model_arrays
    m = 1.0 / float(A["body_mass"][0][0])
    sh = A["shapes"][int(A["tmpl_body_i"][A["body_tmpl"][0]][0])]
    return m, 0.5 * (float(sh[11]) + float(sim.mg_params().ground_dynamic_friction))


def _push_tensors(sim, m, mu):
    """Env HELD pushed along x below mu m g, env SLID above it."""
    f = np.zeros((sim.num_bodies, 3), np.float32)
    f[HELD, 0] = 0.5 * mu * m * G
    f[SLID, 0] = 1.5 * mu * m * G
    ft = torch.from_numpy(f).to(DEV)
    return ft, torch.zeros_like(ft)


def _step(gym, sim, push=None):
    if push is not None:
        assert gym.apply_rigid_body_force_tensors(sim, gymtorch.unwrap_tensor(push[0]),
                                                  gymtorch.unwrap_tensor(push[1]), gymapi.ENV_SPACE)
    gym.simulate(sim)
    gym.fetch_results(sim, True)


def _ncf(gym, sim):
    t = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    gym.refresh_net_contact_force_tensor(sim)
    return t.cpu().numpy().astype(np.float64)


def _assert_balance(rec, ncf, what, skip=None):
    """The listed impulses of every body against the net contact force tensor.
    skip: bodies left out (static bodies: no kernel steps them, their row of the
    tensor is never written)."""
    nb = ncf.shape[0]
    imp = rec["lambda"].astype(np.float64)[:, None] * rec["n"].astype(np.float64) + rec["fimp"].astype(np.float64)
    tot = np.zeros((nb, 3))
    mag = np.zeros((nb, 3))
    for name, sign in (("body0", 1.0), ("body1", -1.0)):
        b = rec[name]
        on = b >= 0
        np.add.at(tot, b[on], sign * imp[on])
        np.add.at(mag, b[on], np.abs(imp[on]))
    err = np.abs(tot / DT - ncf)
    tol = 1e-5 * mag / DT + 1e-6
    if skip is not None:
        err[skip] = 0.0
    worst = float((err - tol).max())
    print("%s: balance max |err| %.3e N, max err / tol %.3f" % (what, err.max(), float((err / tol).max())))
    assert worst <= 0.0, "%s: balance off by %g N beyond the tolerance" % (what, worst)


def test_free_bodies_balance_and_resting_box(gym):
    sim = _boxes(gym, reporting=True)
    m, mu = _mass_mu(sim)
    push = _push_tensors(sim, m, mu)
    assert gym.get_rigid_contact_reporting(sim) is True
    assert N.lib.mg_contact_reporting(sim.native) == 1
    assert N.lib.mg_step_out_supported(sim.native) == 0
    try:
        for k in range(30):
            _step(gym, sim, push)
            rec, total = sim.rigid_contact_records()
            assert total == len(rec)
            _assert_balance(rec, _ncf(gym, sim), "frame %d" % k)
            # owner order: free bodies by index; the falling box lists nothing
            assert np.all(np.diff(rec["body0"]) >= 0) and np.all(np.diff(rec["env"]) >= 0)
            assert not np.any(rec["body0"] == HIGH)
            assert np.array_equal(rec["env"], rec["body0"])          # one body per env
            assert np.all(rec["body1"] == -1)
            # an owner's anchors follow its points
            for b in (0, HELD, SLID, NBOX - 1):
                kinds = rec["kind"][rec["body0"] == b]
                assert np.all(np.diff(kinds) >= 0), (b, kinds)
        ncf = _ncf(gym, sim)
        # a resting box: 4 points on the ground, normal up, carrying its weight
        for b in (0, 33, NBOX - 1):
            r = rec[(rec["body0"] == b) & (rec["kind"] == 0)]
            assert len(r) == 4
            assert np.all(np.abs(r["n"] - np.array([0.0, 0.0, 1.0], np.float32)) <= 1e-6)
            assert np.all(r["body1"] == -1)
            assert abs(r["lambda"].astype(np.float64).sum() / DT - m * G) <= 1e-3 * m * G
            assert np.all(np.abs(np.abs(r["p"][:, 0:2] - [(b % 8) * 4.0, (b // 8) * 4.0]) - 0.5) < 1e-3)
            assert np.all(np.abs(r["mu"] - mu) < 1e-6)
            a = rec[(rec["body0"] == b) & (rec["kind"] == 1)]
            assert 1 <= len(a) <= 2 and np.all(a["lambda"] == 0.0)
        # held below mu m g: the anchors carry the push; above: they saturate at mu m g
        held = rec[(rec["body0"] == HELD) & (rec["kind"] == 1)]
        fh = held["fimp"].astype(np.float64).sum(axis=0) / DT
        assert abs(fh[0] + 0.5 * mu * m * G) <= 0.1 * 0.5 * mu * m * G, fh
        slid = rec[rec["body0"] == SLID]
        fs = np.linalg.norm(slid["fimp"].astype(np.float64).sum(axis=0)) / DT
        print("sliding box: |sum fimp| / dt = %.2f N, mu m g = %.2f N" % (fs, mu * m * G))
        assert abs(fs - mu * m * G) <= 0.1 * mu * m * G
        assert abs(ncf[SLID, 0] + mu * m * G) <= 0.1 * mu * m * G
    finally:
        gym.destroy_sim(sim)


def test_gymapi_view_of_the_list(gym):
    """get_env_rigid_contacts / get_rigid_contacts: Isaac Gym's record over the
    same entries (env-local bodies, body-frame points, friction on (t1, t2))."""
    sim = _boxes(gym, n=9, reporting=True)
    m, mu = _mass_mu(sim)
    try:
        for _ in range(5):
            _step(gym, sim)
        rec, _ = sim.rigid_contact_records()
        allc = gym.get_rigid_contacts(sim)
        assert allc.dtype == gymapi.RigidContact.dtype and len(allc) == len(rec)
        assert np.array_equal(allc["env0"], rec["env"]) and np.array_equal(allc["env1"], rec["env"])
        assert np.all(allc["body0"] == 0) and np.all(allc["body1"] == -1)
        assert np.array_equal(allc["lambda"], rec["lambda"]) and np.array_equal(allc["friction"], rec["mu"])
        assert np.array_equal(allc["minDist"], rec["separation"])
        assert np.array_equal(allc["normal"]["z"], rec["n"][:, 2])
        # n = +z: t1 = n x x^ = +y, t2 = n x t1 = -x
        assert np.allclose(allc["lambdaFriction"]["x"], rec["fimp"][:, 1], atol=1e-7)
        assert np.allclose(allc["lambdaFriction"]["y"], -rec["fimp"][:, 0], atol=1e-7)
        env = gym.get_env(sim, 3)
        ec = gym.get_env_rigid_contacts(env)
        assert len(ec) == int((rec["env"] == 3).sum()) and np.all(ec["env0"] == 3)
        pts = ec[ec["lambda"] > 0.0]
        assert len(pts) == 4
        # the box's bottom corners in its own frame; the ground's point in the env's
        for c in "xy":
            assert np.all(np.abs(np.abs(pts["localPos0"][c]) - 0.5) < 1e-3)
            assert np.all(np.abs(np.abs(pts["localPos1"][c]) - 0.5) < 1e-3)
        assert np.all(np.abs(pts["localPos0"]["z"] + 0.5) < 1e-3)
        assert np.all(np.abs(pts["localPos1"]["z"]) < 2e-3)
        anchors = ec[(ec["lambda"] == 0.0)]
        assert len(anchors) >= 1
        f = gym.get_env_rigid_contact_forces(env)
        assert f.dtype == gymapi.Vec3.dtype and f.shape == (1,)
        assert abs(float(f["z"][0]) - m * G) <= 1e-3 * m * G
        fa = gym.get_rigid_contact_forces(sim)
        assert fa.shape == (9,) and float(fa["z"][HIGH]) == 0.0
    finally:
        gym.destroy_sim(sim)


def test_first_query_turns_reporting_on(gym, capfd):
    sim = _boxes(gym, n=3)
    try:
        _step(gym, sim)
        assert gym.get_rigid_contact_reporting(sim) is False
        first = gym.get_rigid_contacts(sim)
        assert len(first) == 0 and "next simulate" in capfd.readouterr().err
        assert gym.get_rigid_contact_reporting(sim) is True
        assert len(gym.get_rigid_contacts(sim)) == 0          # still no reporting simulate
        _step(gym, sim)
        assert len(gym.get_rigid_contacts(sim)) >= 3 * 4
        assert capfd.readouterr().err == ""
        gym.set_rigid_contact_reporting(sim, False)
        assert N.lib.mg_contact_reporting(sim.native) == 0
        assert N.lib.mg_step_out_supported(sim.native) == 1
    finally:
        gym.destroy_sim(sim)


def test_capacity_drops_and_never_overruns(gym):
    full = _boxes(gym, reporting=True)
    capped = _boxes(gym, reporting=True, max_contacts=10)
    try:
        for _ in range(3):
            _step(gym, full)
            _step(gym, capped)
        want, total = full.rigid_contact_records()
        assert total == len(want) and total > 10
        got, ctotal = capped.rigid_contact_records()
        assert len(got) == 10 and ctotal == total
        assert got.tobytes() == want[:10].tobytes()
        # a destination of 10 records followed by a canary, on the host and on the device
        size = N.RIGID_CONTACT_DTYPE.itemsize
        tot = ctypes.c_int32(0)
        host = np.full((10 + 4) * size, 0xAB, dtype=np.uint8)
        n = N.lib.mg_refresh_rigid_contacts(full.native, host.ctypes.data, 10, 1, ctypes.byref(tot), full.stream())
        assert n == 10 and tot.value == total
        assert host[:10 * size].tobytes() == want[:10].tobytes() and np.all(host[10 * size:] == 0xAB)
        dev = torch.full(((10 + 4) * size,), 0xAB, dtype=torch.uint8, device=DEV)
        n = N.lib.mg_refresh_rigid_contacts(capped.native, dev.data_ptr(), 14, 0, ctypes.byref(tot), capped.stream())
        torch.cuda.synchronize()
        assert n == 10 and tot.value == total                 # the sim stored 10, whatever the destination holds
        back = dev.cpu().numpy()
        assert back[:10 * size].tobytes() == want[:10].tobytes() and np.all(back[10 * size:] == 0xAB)
        n = N.lib.mg_refresh_rigid_contacts(capped.native, dev.data_ptr(), 3, 0, None, capped.stream())
        assert n == 3
    finally:
        gym.destroy_sim(full)
        gym.destroy_sim(capped)


def test_off_means_off(gym):
    """Stepping with reporting on changes neither the state nor the net contact
    force, bit for bit."""
    out = {}
    for on in (False, True):
        sim = _boxes(gym, reporting=on if on else None)
        m, mu = _mass_mu(sim)
        push = _push_tensors(sim, m, mu)
        rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        for _ in range(30):
            _step(gym, sim, push)
        gym.refresh_rigid_body_state_tensor(sim)
        out[on] = (rb.cpu().numpy().copy(), _ncf(gym, sim))
        if not on:
            rec, total = sim.rigid_contact_records()
            assert len(rec) == 0 and total == 0
        gym.destroy_sim(sim)
    assert np.array_equal(out[False][0], out[True][0])
    assert np.array_equal(out[False][1], out[True][1])
    assert abs(out[True][0][SLID, 0] - out[True][0][HELD, 0] - 4.0) > 0.05       # the pushed box did slide


_DUMBBELL = """<?xml version="1.0"?>
<robot name="dumbbell">
  <link name="bar">
    <inertial><origin xyz="0 0 0"/><mass value="4.0"/>
      <inertia ixx="0.1" iyy="0.4" izz="0.4" ixy="0" ixz="0" iyz="0"/></inertial>
    <collision><origin xyz="-0.3 0 0"/><geometry><box size="0.2 0.2 0.2"/></geometry></collision>
    <collision><origin xyz="0.3 0 0"/><geometry><box size="0.2 0.2 0.2"/></geometry></collision>
  </link>
</robot>
"""


def test_multi_shape_bodies_beside_single_shape_ones(gym, tmp_path):
    """A two-box body (k_rigid_step's shift-register slots: per-point friction,
    the points carry fimp) in every other env, unit boxes in the rest: both
    launches stage into one record table, in storage-slot order."""
    (tmp_path / "dumbbell.urdf").write_text(_DUMBBELL)
    sim = _sim(gym)
    bell = gym.load_asset(sim, str(tmp_path), "dumbbell.urdf", gymapi.AssetOptions())
    assert len(bell.bodies[0].shapes) == 2
    box = gym.create_box(sim, 1.0, 1.0, 1.0, gymapi.AssetOptions())
    n = 70
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-2, -2, 0), gymapi.Vec3(2, 2, 4), 8)
        if i % 2:
            gym.create_actor(env, bell, gymapi.Transform(gymapi.Vec3(0, 0, 0.1)), "bell", i, 0)
        else:
            gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0, 0, 0.5)), "box", i, 0)
    gym.set_rigid_contact_reporting(sim, True)
    gym.prepare_sim(sim)
    f = np.zeros((n, 3), np.float32)
    f[1::2, 1] = 5.0                    # a sideways push on the dumbbells: friction at their points
    push = (torch.from_numpy(f).to(DEV), torch.zeros((n, 3), device=DEV))
    try:
        for k in range(30):
            _step(gym, sim, push)
            rec, total = sim.rigid_contact_records()
            assert total == len(rec)
            _assert_balance(rec, _ncf(gym, sim), "frame %d" % k)
        r = rec[rec["body0"] == 1]
        assert len(r) == 8 and np.all(r["kind"] == 0) and np.all(r["env"] == 1)
        assert np.abs(r["fimp"][:, 1]).max() > 0.0
        assert abs(r["lambda"].astype(np.float64).sum() / DT - 4.0 * G) <= 1e-3 * 4.0 * G
        # single-shape bodies first (their storage slots come first), then the others
        even = rec["body0"] % 2 == 0
        assert np.all(even[:int(even.sum())]) and np.all(np.diff(rec["body0"][even]) >= 0)
        assert np.all(np.diff(rec["body0"][~even]) >= 0)
    finally:
        gym.destroy_sim(sim)


def test_wide_launch_reports(gym):
    """More single-shape bodies than one resident round (4 SIMDs x 2 waves per
    CU; 2048 wavefronts on 256 CUs): k_rigid_step1's wide reporting build, and
    a compaction over more blocks than one pass of its base sum. The smallest
    size that gets there on this device (2.9 s on an MI355X)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * (cus * 4 * 2 + 2)
    sim = _sim(gym)
    box = gym.create_box(sim, 1.0, 1.0, 1.0, gymapi.AssetOptions())
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-2, -2, 0), gymapi.Vec3(2, 2, 4), 512)
        gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0, 0, 5.5 if i % 1000 == 7 else 0.5)), "box", i, 0)
    gym.set_rigid_contact_reporting(sim, True)
    gym.prepare_sim(sim)
    try:
        for k in range(2):
            _step(gym, sim)
        rec, total = sim.rigid_contact_records()
        assert total == len(rec)
        _assert_balance(rec, _ncf(gym, sim), "%d boxes" % n)
        assert np.array_equal(rec["env"], rec["body0"]) and np.all(np.diff(rec["env"]) >= 0)
        counts = np.bincount(rec["env"], minlength=n)
        high = np.arange(n) % 1000 == 7
        assert np.all(counts[high] == 0) and np.all(counts[~high] >= 5) and np.all(counts <= 6)
        assert np.all(np.bincount(rec["env"][rec["kind"] == 0], minlength=n)[~high] == 4)
    finally:
        gym.destroy_sim(sim)


def test_graph_rule(gym):
    """Set before the capture the list follows the replays; the switch is
    refused after a captured simulate (MG_ERR_STATE)."""
    eager = []
    sim = _boxes(gym, n=NBOX, reporting=True)
    for _ in range(5):
        _step(gym, sim)
        eager.append(sim.rigid_contact_records()[0])
    gym.destroy_sim(sim)
    sim = _boxes(gym, n=NBOX, reporting=True)
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
        for k in range(5):
            g.replay()
            torch.cuda.synchronize()
            rec, total = sim.rigid_contact_records()
            assert total == len(eager[k]) and rec.tobytes() == eager[k].tobytes(), "replay %d" % k
        assert N.lib.mg_set_contact_reporting(sim.native, 0, 0) == -3          # MG_ERR_STATE
        assert "captured into a graph" in N.last_error()
        with pytest.raises(N.MigymError):
            gym.set_rigid_contact_reporting(sim, False)
        assert gym.get_rigid_contact_reporting(sim) is True
        assert N.lib.mg_contact_reporting(sim.native) == 1
        _step(gym, sim)                                                        # eager again
        gym.set_rigid_contact_reporting(sim, False)
        assert N.lib.mg_contact_reporting(sim.native) == 0
    finally:
        gym.destroy_sim(sim)


STACK = (0.3, 0.2, 0.1)


def _add_stack(gym, sim, group):
    """test_pile.test_box_stack_stands' three boxes, one on the other: a pile env."""
    env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 4)
    z = 0.0
    for k, s in enumerate(STACK):
        box = gym.create_box(sim, s, s, s, gymapi.AssetOptions())
        gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.01 * k, -0.005 * k, z + s / 2)), "b%d" % k, group, 0)
        z += s
    return env


def _stacks(gym, n=2, substeps=1, dt=DT):
    sp = PS.sim_params(True, substeps=substeps, npos=8, contact_offset=0.002)
    sp.dt = dt
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, plane)
    for i in range(n):
        _add_stack(gym, sim, i)
    gym.set_rigid_contact_reporting(sim, True)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_pile_envs(sim.native) == n
    return sim


def test_pile_stack(gym):
    """Three stacked boxes per env (k_pile_step): every body's balance, the
    middle box on both sides of a pair, the ground carrying the whole stack."""
    sim = _stacks(gym)
    mass = 1000.0 * np.array(STACK) ** 3
    try:
        for k in range(60):
            _step(gym, sim)
            rec, total = sim.rigid_contact_records()
            assert total == len(rec)
            _assert_balance(rec, _ncf(gym, sim), "frame %d" % k)
        assert np.all(rec["kind"] == 0) and np.all(np.diff(rec["env"]) >= 0)
        assert int((rec["env"] == 0).sum()) == int((rec["env"] == 1).sum()) > 0
        for e in (0, 1):
            r = rec[rec["env"] == e]
            b = 3 * e
            pairs = set(zip(r["body0"].tolist(), r["body1"].tolist()))
            assert pairs == {(b, -1), (b, b + 1), (b + 1, b + 2)}, pairs
            # pair order, a pair's points together
            key = r["body0"].astype(np.int64) * 8 + (r["body1"] + 1)
            assert np.all(np.diff(np.where(r["body1"] < 0, -1, key)) >= 0)
            ground = r[r["body1"] == -1]
            assert np.all(np.abs(ground["n"] - np.array([0, 0, 1], np.float32)) <= 1e-6)
            carried = ground["lambda"].astype(np.float64).sum() / DT
            print("env %d: the ground carries %.3f N of %.3f N" % (e, carried, mass.sum() * G))
            assert abs(carried - mass.sum() * G) <= 0.02 * mass.sum() * G
            top = r[r["body0"] == b + 1]
            assert abs(top["lambda"].astype(np.float64).sum() / DT - mass[2] * G) <= 0.02 * mass[2] * G
        allc = gym.get_env_rigid_contacts(gym.get_env(sim, 1))
        assert set(zip(allc["body0"].tolist(), allc["body1"].tolist())) == {(0, -1), (0, 1), (1, 2)}
    finally:
        gym.destroy_sim(sim)


def test_two_substeps_list_is_the_last_substeps(gym):
    """substeps = 2: the list is the last substep's. A sim of half the dt and
    one substep, from the same start, ends its frame 2 k where the other ends
    its frame k's last substep: the same points, normals and bodies."""
    two = _stacks(gym, substeps=2, dt=DT)
    one = _stacks(gym, substeps=1, dt=DT / 2)
    try:
        for k in range(3):
            _step(gym, two)
            _step(gym, one)
            _step(gym, one)
            a, _ = two.rigid_contact_records()
            b, _ = one.rigid_contact_records()
            assert len(a) == len(b) > 0
            for f in ("env", "body0", "body1", "kind", "p", "n"):
                assert np.array_equal(a[f], b[f]), (k, f)
    finally:
        gym.destroy_sim(two)
        gym.destroy_sim(one)


def test_mixed_sim_owner_order(gym):
    """Free bodies and pile envs in one sim: the free bodies' entries first, then
    the pile envs', with the entry counts of the families run alone."""
    def build(kinds):
        sp = PS.sim_params(True, substeps=1, npos=8, contact_offset=0.002)
        sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
        plane = gymapi.PlaneParams()
        plane.normal = gymapi.Vec3(0, 0, 1)
        gym.add_ground(sim, plane)
        box = gym.create_box(sim, 0.2, 0.2, 0.2, gymapi.AssetOptions())
        for i, kind in enumerate(kinds):
            if kind == "stack":
                _add_stack(gym, sim, i)
            else:
                env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 4)
                gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0, 0, 0.1)), "box", i, 0)
        gym.set_rigid_contact_reporting(sim, True)
        gym.prepare_sim(sim)
        return sim

    def run(kinds):
        sim = build(kinds)
        try:
            for _ in range(5):
                _step(gym, sim)
            rec, _ = sim.rigid_contact_records()
            _assert_balance(rec, _ncf(gym, sim), "+".join(kinds))
            return rec
        finally:
            gym.destroy_sim(sim)

    kinds = ["stack", "box", "box", "stack", "box"]
    mixed = run(kinds)
    boxes = run(["box"])
    stacks = run(["stack"])
    # owner order: the free bodies (envs 1, 2, 4), then the pile envs (0, 3)
    envs = mixed["env"].tolist()
    order = [e for i, e in enumerate(envs) if i == 0 or envs[i - 1] != e]
    assert order == [1, 2, 4, 0, 3], order
    for e, kind in enumerate(kinds):
        alone = boxes if kind == "box" else stacks
        got = mixed[mixed["env"] == e]
        assert len(got) == len(alone) > 0, (e, kind)
        assert np.array_equal(got["kind"], alone["kind"])
        first = min(got["body0"])
        assert np.array_equal(got["body0"] - first, alone["body0"])
        assert np.array_equal(np.where(got["body1"] < 0, -1, got["body1"] - first), alone["body1"])


NB_COUPLED = 7      # bodies per env of _coupled: gimbal 0..3, static box 4, free boxes 5, 6


def _add_coupled(gym, sim, assets, group):
    """A 4-link fixed-base arm (the gimbal, out of reach above), a free box on a
    static box and a free box on the ground, one collision group: a 16-lane
    coupled env."""
    gimbal, table, box = assets
    env = gym.create_env(sim, gymapi.Vec3(-2, -2, 0), gymapi.Vec3(2, 2, 4), 4)
    gym.create_actor(env, gimbal, gymapi.Transform(gymapi.Vec3(0, 0, 2.0)), "gimbal", group, 0)
    gym.create_actor(env, table, gymapi.Transform(gymapi.Vec3(0, 0, 0.2)), "table", group, 0)
    gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.05, 0.02, 0.5)), "on_table", group, 0)
    gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.9, 0, 0.1)), "on_ground", group, 0)
    return env


def _coupled_assets(gym, sim):
    fixed = gymapi.AssetOptions()
    fixed.fix_base_link = True
    gimbal = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/gimbal.urdf", fixed)
    assert len(gimbal.bodies) == 4
    return gimbal, gym.create_box(sim, 0.4, 0.4, 0.4, fixed), gym.create_box(sim, 0.2, 0.2, 0.2, gymapi.AssetOptions())


def _coupled(gym, n=5, reporting=True):
    sim = _sim(gym)
    assets = _coupled_assets(gym, sim)
    for i in range(n):
        _add_coupled(gym, sim, assets, i)
    if reporting is not None:
        gym.set_rigid_contact_reporting(sim, reporting)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == n and sim.num_bodies == NB_COUPLED * n
    return sim


def _ctab(sim, k):
    """Coupled env k's contact table of the last substep (mg_debug_copy_env_ctab):
    participants, point, normal, separation of each contact."""
    cap = N.lib.mg_env_ctab_floats()
    buf = (ctypes.c_float * cap)()
    n = N.lib.mg_debug_copy_env_ctab(sim.native, k, buf, cap)
    assert n > 0
    maxct = (n - 8) // 24
    a = np.frombuffer(buf, np.float32)[:n]
    ib = a.view(np.int32)
    nc = min(int(ib[0]), maxct)
    rows = a[8:8 + 10 * nc].reshape(nc, 10)
    return rows.view(np.int32)[:, 0:2].copy(), rows[:, 2:5].copy(), rows[:, 5:8].copy(), rows[:, 8].copy()


def test_coupled_env_16_lanes(gym):
    """5 coupled envs of a 4-link arm, a free box on a static box and one on the
    ground (k_env_step<.., 16>): the balance, both pairs with the right body1,
    and the points field by field, bit for bit, the contact table's."""
    sim = _coupled(gym)
    static = np.arange(sim.num_bodies) % NB_COUPLED == 4
    rbt = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    try:
        for k in range(30):
            gym.refresh_rigid_body_state_tensor(sim)
            before = rbt.cpu().numpy().astype(np.float64)
            _step(gym, sim)
            rec, total = sim.rigid_contact_records()
            assert total == len(rec)
            _assert_balance(rec, _ncf(gym, sim), "frame %d" % k, skip=static)
        gym.refresh_rigid_body_state_tensor(sim)
        after = rbt.cpu().numpy().astype(np.float64)
        assert np.all(np.diff(rec["env"]) >= 0)
        for e in range(5):
            r = rec[rec["env"] == e]
            g0 = NB_COUPLED * e
            pts, anc = r[r["kind"] == 0], r[r["kind"] == 1]
            assert np.all(np.diff(r["kind"]) >= 0)                       # the anchors after the points
            pairs = set(zip(pts["body0"].tolist(), pts["body1"].tolist()))
            assert pairs == {(g0 + 5, g0 + 4), (g0 + 6, -1)}, pairs
            assert set(zip(anc["body0"].tolist(), anc["body1"].tolist())) == pairs
            assert np.all(anc["lambda"] == 0.0) and np.all(pts["fimp"] == 0.0)
            ab, p, n, sep = _ctab(sim, e)
            assert len(pts) == len(ab) > 0
            body = {-1: -1, 64: g0 + 5, 65: g0 + 6, 80: g0 + 4}
            body.update({l: g0 + l for l in range(4)})
            assert pts["body0"].tolist() == [body[a] for a in ab[:, 0].tolist()]
            assert pts["body1"].tolist() == [body[b] for b in ab[:, 1].tolist()]
            assert pts["p"].tobytes() == p.tobytes() and pts["n"].tobytes() == n.tobytes()
            assert pts["separation"].tobytes() == sep.tobytes()
            # the listed impulses on a box are its change of momentum over the
            # frame less gravity's (no linear damping, one substep): Newton, to
            # the float32 roundings of the velocity updates (about a hundred,
            # as in the balance: 1e-5 of the terms' magnitudes)
            for b in (g0 + 5, g0 + 6):
                m = 1.0 / float(sim.model_arrays["body_mass"][b][0])
                rb_ = r[r["body0"] == b]
                assert not np.any(r["body1"] == b)
                terms = rb_["lambda"].astype(np.float64)[:, None] * rb_["n"] + rb_["fimp"]
                want = m * (after[b, 7:10] - before[b, 7:10]) + np.array([0.0, 0.0, m * G * DT])
                mag = (np.abs(terms).sum(axis=0) + m * np.abs(after[b, 7:10]) + m * np.abs(before[b, 7:10]) +
                       m * G * DT)
                err = np.abs(terms.sum(axis=0) - want)
                print("env %d body %d: momentum max err / tol %.3f" % (e, b, float((err / (1e-5 * mag + 1e-9)).max())))
                assert np.all(err <= 1e-5 * mag + 1e-9), (err, mag)
        ec = gym.get_env_rigid_contacts(gym.get_env(sim, 2))
        assert set(zip(ec["body0"].tolist(), ec["body1"].tolist())) == {(5, 4), (6, -1)}
    finally:
        gym.destroy_sim(sim)


def test_coupled_env_64_lanes_ant(gym):
    """nv_ant.xml dropped on the ground, 3 envs: once a foot is down every
    listed body0 is a link of its env's ant, in contact with the ground."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_assets")
    sim, info = scenes.ant_scene(gym, 3, asset_root=root, asset_file="mjcf/nv_ant.xml", height=0.6)
    gym.set_rigid_contact_reporting(sim, True)
    gym.prepare_sim(sim)
    nb = info["num_bodies"]
    assert N.lib.mg_num_coupled_envs(sim.native) == 3
    dt = float(sim.params.dt)
    assert abs(dt - DT) < 1e-9
    down = 0
    try:
        for k in range(60):
            _step(gym, sim)
            rec, total = sim.rigid_contact_records()
            assert total == len(rec)
            _assert_balance(rec, _ncf(gym, sim), "frame %d" % k)
            if len(rec):
                down += 1
                assert np.all(rec["body1"] == -1) and np.all(np.diff(rec["env"]) >= 0)
                assert np.all(rec["body0"] // nb == rec["env"])
                assert np.all(np.abs(rec["n"] - np.array([0, 0, 1], np.float32)) <= 1e-6)
        assert down >= 10 and set(rec["env"].tolist()) == {0, 1, 2}
        assert float(rec["lambda"].sum()) > 0.0
    finally:
        gym.destroy_sim(sim)


def test_off_means_off_coupled(gym):
    """The coupled scene stepped 30 frames with reporting never enabled and with
    it enabled: state, DOF state and net contact force bit-identical."""
    out = {}
    for on in (False, True):
        sim = _coupled(gym, reporting=True if on else None)
        rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
        for _ in range(30):
            _step(gym, sim)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_dof_state_tensor(sim)
        out[on] = (rb.cpu().numpy().copy(), dof.cpu().numpy().copy(), _ncf(gym, sim))
        gym.destroy_sim(sim)
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(a, b)
    assert np.abs(out[True][2]).max() > 1.0


def test_mixed_sim_all_three_families(gym):
    """Free bodies, coupled envs and a pile env in one sim: the owner order is
    free, coupled, pile, each by env index, with the entry counts, kinds and
    bodies of the families run alone."""
    def run(kinds):
        sim = _sim(gym)
        assets = _coupled_assets(gym, sim)
        for i, kind in enumerate(kinds):
            if kind == "stack":
                _add_stack(gym, sim, i)
            elif kind == "coupled":
                _add_coupled(gym, sim, assets, i)
            else:
                env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 4)
                gym.create_actor(env, assets[2], gymapi.Transform(gymapi.Vec3(0, 0, 0.1)), "box", i, 0)
        gym.set_rigid_contact_reporting(sim, True)
        gym.prepare_sim(sim)
        try:
            for _ in range(5):
                _step(gym, sim)
            rec, _ = sim.rigid_contact_records()
            kind_of = sim.model_arrays["body_kind"]
            _assert_balance(rec, _ncf(gym, sim), "+".join(kinds), skip=kind_of == N.MG_BODY_STATIC)
            first = [e.actors[0].global_body for e in sim.envs]
            return rec, first
        finally:
            gym.destroy_sim(sim)

    kinds = ["stack", "coupled", "box", "coupled", "box", "stack"]
    mixed, first = run(kinds)
    alone = {k: run([k])[0] for k in ("box", "coupled", "stack")}
    envs = mixed["env"].tolist()
    order = [e for i, e in enumerate(envs) if i == 0 or envs[i - 1] != e]
    assert order == [2, 4, 1, 3, 0, 5], order
    for e, kind in enumerate(kinds):
        got, want = mixed[mixed["env"] == e], alone[kind]
        assert len(got) == len(want) > 0, (e, kind)
        assert np.array_equal(got["kind"], want["kind"])
        assert np.array_equal(got["body0"] - first[e], want["body0"])
        assert np.array_equal(np.where(got["body1"] < 0, -1, got["body1"] - first[e]), want["body1"])
