"""Rigid-body attractors, host side: handles, properties, the packed table
handed to mg_set_attractors (no device needed), and examples/franka_attractor.py
unmodified up to its first gym.simulate."""
import ctypes
import math
import os

import numpy as np
import pytest

from isaacgym import gymapi
from test_isaacgym_amd import _native as N

from conftest import has_gpu
from test_reference_scripts import REFERENCE, _exec_script


def _scene(gym, num_envs=3, two_bodies=False):
    sp = gymapi.SimParams()
    sp.dt = 1.0 / 60.0
    sp.substeps = 2
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -9.81)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    asset = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    lo, hi = gymapi.Vec3(-0.75, -0.75, 0.0), gymapi.Vec3(0.75, 0.75, 1.5)
    envs, actors = [], []
    for i in range(num_envs):
        env = gym.create_env(sim, lo, hi, 2)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.1, 0.2, 1.0)
        hs = [gym.create_actor(env, asset, pose, "box", i, 0)]
        if two_bodies:
            pose.p = gymapi.Vec3(0.5, 0.2, 1.0)
            hs.append(gym.create_actor(env, asset, pose, "box2", i, 0))
        envs.append(env)
        actors.append(hs)
    return sim, envs, actors


def _props(rigid_handle, target=(0.0, 0.0, 0.0)):
    p = gymapi.AttractorProperties()
    p.stiffness = 200.0
    p.damping = 4.0
    p.axes = gymapi.AXIS_TRANSLATION
    p.rigid_handle = rigid_handle
    p.target.p = gymapi.Vec3(*target)
    return p


def test_axis_flag_values():
    assert (gymapi.AXIS_X, gymapi.AXIS_Y, gymapi.AXIS_Z) == (1, 2, 4)
    assert (gymapi.AXIS_TWIST, gymapi.AXIS_SWING_1, gymapi.AXIS_SWING_2) == (8, 16, 32)
    assert gymapi.AXIS_TRANSLATION == gymapi.AXIS_X | gymapi.AXIS_Y | gymapi.AXIS_Z == 7
    assert gymapi.AXIS_ROTATION == gymapi.AXIS_TWIST | gymapi.AXIS_SWING_1 | gymapi.AXIS_SWING_2 == 56
    assert gymapi.AXIS_ALL == 63 and gymapi.AXIS_NONE == 0


def test_handles_and_property_round_trip():
    gym = gymapi.acquire_gym()
    sim, envs, actors = _scene(gym, 2, two_bodies=True)
    try:
        env = envs[1]
        b0 = gym.get_actor_rigid_body_handle(env, actors[1][0], 0)
        b1 = gym.get_actor_rigid_body_handle(env, actors[1][1], 0)
        assert gym.create_rigid_body_attractor(env, _props(b0, (0.1, 0.2, 0.3))) == 0
        assert gym.create_rigid_body_attractor(env, _props(b1, (0.4, 0.5, 0.6))) == 1
        assert gym.create_rigid_body_attractor(envs[0], _props(0)) == 0      # numbering is per env
        got = gym.get_attractor_properties(env, 1)
        assert (got.stiffness, got.damping, got.axes, got.rigid_handle) == (200.0, 4.0, 7, b1)
        assert (got.target.p.x, got.target.p.y, got.target.p.z) == (0.4, 0.5, 0.6)
        # a copy: changing it changes nothing until it is handed back
        got.target.p.x = 9.0
        got.stiffness = 1.0
        again = gym.get_attractor_properties(env, 1)
        assert again.target.p.x == 0.4 and again.stiffness == 200.0
        assert gym.set_attractor_properties(env, 1, got)
        got.stiffness = 2.0                                                    # the sim kept its own copy
        again = gym.get_attractor_properties(env, 1)
        assert again.target.p.x == 9.0 and again.stiffness == 1.0
        t = gymapi.Transform(gymapi.Vec3(1.0, 2.0, 3.0), gymapi.Quat(0.0, 0.0, math.sin(0.25), math.cos(0.25)))
        assert gym.set_attractor_target(env, 0, t)
        t.p.x = -1.0
        got = gym.get_attractor_properties(env, 0)
        assert (got.target.p.x, got.target.p.y, got.target.p.z) == (1.0, 2.0, 3.0)
        assert got.target.r.z == pytest.approx(math.sin(0.25))
    finally:
        gym.destroy_sim(sim)


def test_invalid_handle_and_second_attractor_refused():
    gym = gymapi.acquire_gym()
    sim, envs, actors = _scene(gym, 1)
    try:
        env = envs[0]
        assert gym.create_rigid_body_attractor(env, _props(gymapi.INVALID_HANDLE)) == gymapi.INVALID_HANDLE
        assert gym.create_rigid_body_attractor(env, _props(7)) == gymapi.INVALID_HANDLE
        assert gym.create_rigid_body_attractor(env, _props(0)) == 0
        assert gym.create_rigid_body_attractor(env, _props(0)) == gymapi.INVALID_HANDLE   # one per body
        assert len(env.attractors) == 1
    finally:
        gym.destroy_sim(sim)


def test_target_accepts_pose_record():
    """franka_attractor.py:122-124: a ['pose'] record is assigned, then written
    through .target.p."""
    gym = gymapi.acquire_gym()
    sim, envs, actors = _scene(gym, 1)
    try:
        st = gym.get_actor_rigid_body_states(envs[0], actors[0][0], gymapi.STATE_POS)
        p = gymapi.AttractorProperties()
        p.target = st["pose"][:][0]
        assert isinstance(p.target, gymapi.Transform)
        assert (p.target.p.x, p.target.p.y, p.target.p.z) == pytest.approx((0.1, 0.2, 1.0))
        p.target.p.y -= 0.1
        p.target.p.z = 0.1
        assert (p.target.p.y, p.target.p.z) == pytest.approx((0.1, 0.1))
        assert float(st["pose"]["p"]["y"][0]) == pytest.approx(0.2)     # the record was copied
    finally:
        gym.destroy_sim(sim)


def test_packed_table_global_bodies_and_targets():
    gym = gymapi.acquire_gym()
    sim, envs, actors = _scene(gym, 3, two_bodies=True)
    try:
        for i, env in enumerate(envs):
            h = gym.get_actor_rigid_body_handle(env, actors[i][1], 0)        # the env's second body
            p = _props(h, (0.1 * i, 0.2, 0.3))
            p.offset.p = gymapi.Vec3(0.01, 0.02, 0.03)
            p.target.r = gymapi.Quat(0.0, 0.0, math.sin(0.5), math.cos(0.5))
            assert gym.create_rigid_body_attractor(env, p) == 0
        tab, n = sim.attractor_table()
        assert n == 3
        origins = np.array([e.origin for e in envs])
        assert np.abs(origins[1:]).max() > 1.0                                # non-zero env origins
        for i in range(3):
            r = tab[i]
            assert r.body == 2 * i + 1
            assert r.axes == 7 and r.stiffness == 200.0 and r.damping == 4.0
            assert list(r.offset_p) == pytest.approx([0.01, 0.02, 0.03])
            assert list(r.offset_q) == [0.0, 0.0, 0.0, 1.0]
            assert list(r.target_p) == pytest.approx(list(origins[i] + np.array([0.1 * i, 0.2, 0.3])))
            assert list(r.target_q) == pytest.approx([0.0, 0.0, math.sin(0.5), math.cos(0.5)])
        assert ctypes.sizeof(N.MgAttractor) == 72        # include/migym.h mg_attractor: 2 int32 + 16 float
    finally:
        gym.destroy_sim(sim)


@pytest.mark.skipif(has_gpu(), reason="CPU-container variant")
@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree absent")
def test_franka_attractor_script_setup(monkeypatch):
    """examples/franka_attractor.py unmodified up to its first gym.simulate.

    Pins a known deviation: attractor targets are in the env's
    frame (the script's update_franka, :155-168, sends every env the same
    circle), but this build's get_actor_rigid_body_states returns global
    coordinates, and the script feeds the one into the other (:118-124). So the
    script's *initial* target of an env off the origin is the hand pose plus the
    env origin a second time, until update_franka replaces it at t = 1.5 s."""
    path = os.path.join(REFERENCE, "examples", "franka_attractor.py")
    ns, err = _exec_script(path, os.path.join(REFERENCE, "examples"), monkeypatch)
    assert isinstance(err, N.MigymError)                    # raised by gym.simulate: no device here
    gym, envs = ns["gym"], ns["envs"]
    assert len(ns["attractor_handles"]) == 36 and all(h == 0 for h in ns["attractor_handles"])
    for env, fh in zip(envs, ns["franka_handles"]):
        hand = gym.find_actor_rigid_body_handle(env, fh, "panda_hand")
        # the hand pose the script read (:119): the actor as created, all DOFs at
        # 0 (the mid-range pose is set after the attractors, :178-183)
        a = env.actors[fh]
        keep = a.dof_state.copy()
        a.dof_state[:] = 0.0
        ps, qs = env.sim.actor_world_body_poses(a)
        a.dof_state[:] = keep
        hp, hq = np.float32(ps[hand - a.body_offset]), np.float32(qs[hand - a.body_offset])
        p = gym.get_attractor_properties(env, 0)
        assert (p.stiffness, p.damping, p.axes, p.rigid_handle) == (5e5, 5e3, 63, hand)
        assert p.target.p.x == pytest.approx(float(hp[0]), abs=1e-6)
        assert p.target.p.y == pytest.approx(float(hp[1]) - 0.1, abs=1e-6)
        assert p.target.p.z == pytest.approx(0.1, abs=1e-7)
        assert [p.target.r.x, p.target.r.y, p.target.r.z, p.target.r.w] == pytest.approx(list(hq), abs=1e-6)
    # what the sim is handed: the env-frame target plus the env origin. For env 0
    # (at the origin) that is the hand pose with y - 0.1, z = 0.1; for an env off
    # the origin it is NOT: x carries the origin twice (the deviation above)
    tab, n = ns["sim"].attractor_table()
    assert n == 36
    hand_glob = []
    for env, fh in zip(envs, ns["franka_handles"]):
        a = env.actors[fh]
        keep = a.dof_state.copy()
        a.dof_state[:] = 0.0
        ps, _ = env.sim.actor_world_body_poses(a)
        a.dof_state[:] = keep
        hand_glob.append(np.array(ps[gym.find_actor_rigid_body_handle(env, fh, "panda_hand") - a.body_offset]))
    assert list(envs[0].origin) == [0.0, 0.0, 0.0]
    assert list(tab[0].target_p) == pytest.approx([hand_glob[0][0], hand_glob[0][1] - 0.1, 0.1], abs=1e-6)
    assert [tab[i].body for i in range(36)] == [11 * i + 8 for i in range(36)]
    for i in (1, 7, 35):
        o = envs[i].origin
        assert np.abs(o).max() >= 2.0
        want = [hand_glob[i][0] + o[0], hand_glob[i][1] - 0.1 + o[1], 0.1 + o[2]]
        assert list(tab[i].target_p) == pytest.approx(want, abs=1e-5)
        intended = np.array([hand_glob[i][0], hand_glob[i][1] - 0.1, o[2] + 0.1])
        assert np.linalg.norm(np.array(tab[i].target_p) - intended) == pytest.approx(abs(o[0]), abs=1e-5)


def test_target_updates_leave_in_one_call(monkeypatch):
    """update_franka's per-env set_attractor_target loop (franka_attractor.py:
    155-168) ends in one mg_set_attractor_targets call at the next simulate; a
    created or replaced attractor sends the whole table once."""
    gym = gymapi.acquire_gym()
    sim, envs, actors = _scene(gym, 3)
    calls = []

    def set_table(native, tab, n):
        calls.append(("table", n, [tab[k].body for k in range(n)]))
        return 0

    def set_targets(native, ptr, first, n):
        pose = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n, 7)).copy()
        calls.append(("targets", first, n, pose))
        return 0

    monkeypatch.setattr(N.lib, "mg_set_attractors", set_table)
    monkeypatch.setattr(N.lib, "mg_set_attractor_targets", set_targets)
    try:
        for env in envs:
            assert gym.create_rigid_body_attractor(env, _props(0, (0.1, 0.2, 0.3))) == 0
        sim.native = 1                          # stands in for a device sim: only the patched entries are called
        sim.push_attractors()
        assert calls == [("table", 3, [0, 1, 2])]
        sim.push_attractors()                   # nothing changed: nothing sent
        assert len(calls) == 1
        for i, env in enumerate(envs):
            p = gym.get_attractor_properties(env, 0)
            pose = p.target
            pose.p.x = 0.5 + i
            gym.set_attractor_target(env, 0, pose)
        sim.push_attractors()
        assert len(calls) == 2
        kind, first, n, pose = calls[1]
        assert (kind, first, n) == ("targets", 0, 3)
        want = np.array([e.origin + np.array([0.5 + i, 0.2, 0.3]) for i, e in enumerate(envs)])
        assert pose[:, 0:3] == pytest.approx(want) and (pose[:, 3:7] == [0.0, 0.0, 0.0, 1.0]).all()
        gym.set_attractor_target(envs[2], 0, gymapi.Transform(gymapi.Vec3(1.0, 1.0, 1.0)))
        sim.push_attractors()
        assert calls[2][:3] == ("targets", 2, 1)
    finally:
        sim.native = None
        gym.destroy_sim(sim)
