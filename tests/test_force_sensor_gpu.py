"""Force sensors on the GPU: the readings against the float64
restatement of their definition (force_sensor64), statics, the contact moment
against the DOF force tensor, the parts and frames, frames that begin with a
state set, no side effects on the trajectory, graph capture and the CPU
pipeline."""
import math

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
from test_isaacgym_amd import scenes
from kinematics64 import Articulation, qmat, qmul
import force_sensor64 as F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 9.8
U = 2.0 ** -23


# ------------------------------------------------------------------ helpers
def _rand_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return rng.uniform(-0.1, 0.1, size=3), q


def _transform(p, q):
    return gymapi.Transform(gymapi.Vec3(*[float(x) for x in p]), gymapi.Quat(*[float(x) for x in q]))


def _props(fd=True, cs=True, world=False):
    p = gymapi.ForceSensorProperties()
    p.enable_forward_dynamics_forces, p.enable_constraint_solver_forces, p.use_world_frame = fd, cs, world
    return p


def _sensor_every_body(gym, asset, seed=5, bodies=None):
    """A sensor on every body (or on `bodies`) at a random local pose, every
    other one in the world frame. Returns [(body, p, q, world)]."""
    rng = np.random.RandomState(seed)
    out = []
    for k, b in enumerate(range(len(asset.bodies)) if bodies is None else bodies):
        p, q = _rand_pose(rng)
        world = k % 2 == 1
        assert gym.create_asset_force_sensor(asset, b, _transform(p, q), _props(world=world)) == k
        out.append((b, p, q, world))
    return out


class Probe:
    """The tensors of a sim and the float64 facts of one actor kind (the actor
    `actor` of every env, all from one asset)."""

    def __init__(self, gym, sim, envs, actor, sensors):
        self.gym, self.sim, self.envs, self.actor, self.sensors = gym, sim, envs, actor, sensors
        gym.prepare_sim(sim)
        self.fs = gymtorch.wrap_tensor(gym.acquire_force_sensor_tensor(sim))
        self.rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        self.ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
        self.nb_sim = self.rb.shape[0]
        a0 = sim.envs[0].actors[actor]
        self.art = Articulation(sim.model_arrays, int([r[2] for r in sim.model_arrays["artic_i"]
                                                       if r[0] == a0.global_body][0]))
        self.nb = a0.num_bodies
        self.g0 = [env.actors[actor].global_body for env in sim.envs]
        self.props = [F64.body_props(gym.get_actor_rigid_body_properties(env, actor)) for env in envs]
        self.rows = [[gym.get_actor_force_sensor(env, actor, k).global_index for k in range(len(sensors))]
                     for env in envs]
        self.sub = [F64.subtree(self.art, b) for b, _, _, _ in sensors]
        g = sim.params.gravity
        self.gravity = None if a0.asset.options.disable_gravity else np.array([g.x, g.y, g.z])
        self.dt = float(sim.params.dt)
        gym.refresh_rigid_body_state_tensor(sim)

    def state(self):
        return self.rb.cpu().numpy().astype(np.float64)

    def step(self, ext_f=None, ext_t=None):
        """One frame; returns (rb before, rb after, net contact force, readings)."""
        gym, sim = self.gym, self.sim
        rb0 = self.state()
        if ext_f is not None:
            f = torch.from_numpy(ext_f.astype(np.float32)).to(DEV)
            t = torch.from_numpy(ext_t.astype(np.float32)).to(DEV)
            assert gym.apply_rigid_body_force_tensors(sim, gymtorch.unwrap_tensor(f), gymtorch.unwrap_tensor(t),
                                                      gymapi.ENV_SPACE)
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        assert gym.refresh_force_sensor_tensor(sim) is True
        got = self.fs.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        return rb0, self.state(), self.ncf.cpu().numpy().astype(np.float64), got.astype(np.float64)

    def reference(self, e, k, rb0, rb1, ext_f=None, ext_t=None, cf=None, **flags):
        """force_sensor64's reading of sensor k of env e, its tolerances K 2^-23 S
        (K = F64.rounding_count of the subtree's size)."""
        b, p, q, world = self.sensors[k]
        g0, nb = self.g0[e], self.nb
        cut = lambda x: None if x is None else x[g0:g0 + nb]
        Fr, Tr, SF, ST = F64.reading(self.sub[k], self.props[e], rb0[g0:g0 + nb], rb1[g0:g0 + nb], self.dt,
                                     self.gravity, p, q, b, cut(ext_f), cut(ext_t), cut(cf),
                                     world=flags.pop("world", world), **flags)
        K = F64.rounding_count(len(self.sub[k]))
        return Fr, Tr, K * U * SF, K * U * ST


def _compare(pr, frames, before_step=None, wrench=None, contacts=False, forces_only=False, what="", skip=1):
    """The identity over `frames` frames (after `skip` unchecked ones: the first
    frame reads 0). Returns the worst error / tolerance and the largest reading."""
    worst_f = worst_t = big = 0.0
    for k in range(skip + frames):
        if before_step is not None:
            before_step(k)
        ef, et = wrench(k) if wrench is not None else (None, None)
        rb0, rb1, ncf, got = pr.step(ef, et)
        if k < skip:
            continue
        for e in range(len(pr.envs)):
            for s in range(len(pr.sensors)):
                Fr, Tr, tf, tt = pr.reference(e, s, rb0, rb1, ef, et, ncf if contacts else None)
                row = got[pr.rows[e][s]]
                ef_, et_ = np.abs(row[0:3] - Fr).max(), np.abs(row[3:6] - Tr).max()
                worst_f = max(worst_f, ef_ / tf)
                big = max(big, np.abs(row).max())
                assert ef_ <= tf, "%s frame %d env %d sensor %d: force %s, float64 %s, tol %g" % (
                    what, k, e, s, row[0:3], Fr, tf)
                if not forces_only:
                    worst_t = max(worst_t, et_ / tt)
                    assert et_ <= tt, "%s frame %d env %d sensor %d: torque %s, float64 %s, tol %g" % (
                        what, k, e, s, row[3:6], Tr, tt)
    print("%s: %d frames, worst force err / tol %.3f, worst torque err / tol %.3f, max |reading| %.4g"
          % (what, frames, worst_f, worst_t, big))
    return max(worst_f, worst_t), big


def _wave_targets(gym, sim, amp, rate):
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    gym.refresh_dof_state_tensor(sim)
    q0 = dof[:, 0].clone()
    ph = torch.linspace(0.0, 5.0, q0.numel(), device=DEV)

    def before(k):
        tg = (q0 + amp * torch.sin(rate * (k + 1) + ph)).contiguous()
        assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    return before


GIMBAL_COM = [(0.04, 0.03, 0.02), (-0.03, 0.02, 0.05), (0.02, -0.04, 0.03)]


def _gimbal(gym, n, substeps=2, gravity=-G, **kw):
    """The S2 gimbal with 1 kg links whose COMs lie off the axes, gravity on."""
    sim, envs = scenes.gimbal_scene(gym, n, link_mass_scale=100.0, **kw)
    sim.params.substeps = substeps
    sim.params.gravity = gymapi.Vec3(0.0, 0.0, gravity)
    for env in envs:
        bp = gym.get_actor_rigid_body_properties(env, 0)
        for b, c in zip(bp[1:], GIMBAL_COM):
            b.com = gymapi.Vec3(*c)
        gym.set_actor_rigid_body_properties(env, 0, bp, False)
    return sim, envs


# ---------------------------------------------------- 1: identity, no contacts
@pytest.mark.parametrize("substeps", [1, 2])
def test_identity_gimbal_chain(gym, substeps):
    """k_artic_chain: 8 gimbals under gravity, moving targets, a sensor on every link."""
    from test_step_out_chain_gpu import _artic_groups
    sim, envs = _gimbal(gym, 8, substeps=substeps)
    sens = _sensor_every_body(gym, sim.assets[0])
    pr = Probe(gym, sim, envs, 0, sens)
    grp = [g for g in _artic_groups(sim) if g["step_count"] > 0]
    assert len(grp) == 1 and (grp[0]["nl"], grp[0]["step_count"], grp[0]["chain"]) == (4, 8, 1), grp
    assert N.lib.mg_num_force_sensors(sim.native) == 32
    _, big = _compare(pr, 20, before_step=_wave_targets(gym, sim, 0.3, 0.35), what="gimbal chain, %d substeps" % substeps)
    assert big > 1.0
    gym.destroy_sim(sim)


@pytest.mark.parametrize("substeps", [1, 2])
def test_identity_franka_lanes(gym, substeps):
    """k_artic_lanes: 4 Frankas alone, wrenches applied on link 4 and the hand."""
    from test_dof_force_gpu import _franka_alone
    sim, envs = _franka_alone(gym, 4, substeps=substeps)
    asset = sim.assets[0]
    sens = _sensor_every_body(gym, asset)
    names = [b.name for b in asset.bodies]
    l4, hand = names.index("panda_link4"), names.index("panda_hand")
    pr = Probe(gym, sim, envs, 0, sens)
    assert N.lib.mg_num_coupled_envs(sim.native) == 0
    rng = np.random.RandomState(9)

    def wrench(k):
        f, t = np.zeros((pr.nb_sim, 3)), np.zeros((pr.nb_sim, 3))
        for g0 in pr.g0:
            f[g0 + l4], t[g0 + l4] = rng.uniform(-8, 8, 3), rng.uniform(-1, 1, 3)
            f[g0 + hand], t[g0 + hand] = rng.uniform(-5, 5, 3), rng.uniform(-0.5, 0.5, 3)
        return f.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)

    _, big = _compare(pr, 20, before_step=_wave_targets(gym, sim, 0.05, 0.3), wrench=wrench,
                      what="franka lanes, %d substeps" % substeps)
    assert big > 10.0
    gym.destroy_sim(sim)


@pytest.mark.parametrize("substeps", [1, 2])
def test_identity_ball_joint_chain(gym, tmp_path, substeps):
    """test13's chain: three prismatic links, then a ball joint whose two
    virtual links pass the subtree through."""
    from test_ball_joint import _scene, _urdf
    d, n = str(tmp_path), 4
    init = np.random.RandomState(3).uniform(-0.3, 0.3, size=(n, 6)).astype(np.float32)
    sim, asset = _scene(gym, d, n, _urdf(d, "b.urdf"), gpu=True, drive=(40.0, 4.0),
                        init=lambda i: (init[i], np.zeros(6)))
    sim.params.substeps = substeps
    sens = _sensor_every_body(gym, asset)
    pr = Probe(gym, sim, sim.envs, 0, sens)
    assert pr.art.L > len(asset.bodies)                      # virtual links exist
    _, big = _compare(pr, 20, before_step=_wave_targets(gym, sim, 0.05, 0.3),
                      what="ball joint chain, %d substeps" % substeps)
    assert big > 10.0
    gym.destroy_sim(sim)


# --------------------------------------- 2: identity with contacts, forces only
ANT_FEET = ("front_left_foot", "front_right_foot", "left_back_foot", "right_back_foot")


def _ant(gym, n, height=0.6, props=None, asset_options=None):
    sim, info = scenes.ant_scene(gym, n, height=height, asset_options=asset_options)
    asset = info["asset"]
    names = [b.name for b in asset.bodies]
    bodies = [names.index(f) for f in ANT_FEET] + [names.index("torso")]
    sens = []
    rng = np.random.RandomState(2)
    for k, b in enumerate(bodies):
        p, q = _rand_pose(rng)
        world = k % 2 == 1
        gym.create_asset_force_sensor(asset, b, _transform(p, q), props or _props(world=world))
        sens.append((b, p, q, (props.use_world_frame if props else world)))
    for env, a in zip(info["envs"], info["actors"]):
        dp = gym.get_actor_dof_properties(env, a)
        dp["driveMode"][:] = gymapi.DOF_MODE_POS
        dp["stiffness"][:], dp["damping"][:] = 20.0, 1.0
        gym.set_actor_dof_properties(env, a, dp)
    return sim, info, sens


def test_identity_ant_landing_forces(gym):
    """k_env_step on a floating base: 4 ants dropped onto the ground, sensors on
    the four feet and the torso, 30 frames through the landing; force rows
    (the contact moment is no public tensor: tests 4 and 5 cover the torque)."""
    sim, info, sens = _ant(gym, 4)
    pr = Probe(gym, sim, info["envs"], 0, sens)
    assert N.lib.mg_num_coupled_envs(sim.native) == 4
    touched = []

    def before(k):
        touched.append(float(pr.ncf.abs().max()))

    _, big = _compare(pr, 30, before_step=before, contacts=True, forces_only=True, what="ant landing")
    assert max(touched) > 1.0, "the ants never landed"
    assert big > 1.0
    gym.destroy_sim(sim)


# ------------------------------------------------------------------ 3: statics
def _unsteadiness(pr, e, bodies, frames_rb, o_s=None):
    """sum_k m_k max |v+ - v-| / dt over the compared frames (and, about o_s,
    the angular form sum_k (|c_k - o_s| m_k |dv| + I_max |dw|) / dt): the size
    of the net wrench the pose's residual motion can hide."""
    g0 = pr.g0[e]
    lin = ang = 0.0
    for k in bodies:
        m, com, I = pr.props[e][k]
        dv = max(np.linalg.norm(b[g0 + k, 7:10] - a[g0 + k, 7:10]) for a, b in frames_rb)
        dw = max(np.linalg.norm(b[g0 + k, 10:13] - a[g0 + k, 10:13]) for a, b in frames_rb)
        lin += m * dv / pr.dt
        if o_s is not None:
            rb1 = frames_rb[-1][1]
            c = rb1[g0 + k, 0:3] + qmat(rb1[g0 + k, 3:7]) @ com
            ang += (np.linalg.norm(c - o_s) * m * dv + np.linalg.eigvalsh(I).max() * dw) / pr.dt
    return lin, ang


def test_static_franka_weight_and_moment(gym):
    """A fixed-base Franka held by its drives until it rests: every link's
    world-frame sensor reads its subtree's weight -M g and gravity moment about
    the sensor origin (float64 from the state tensor); the base's is the whole
    arm's. Tolerance: the identity's K 2^-23 S plus the measured unsteadiness."""
    from test_dof_force_gpu import _franka_alone
    sim, envs = _franka_alone(gym, 2, substeps=2)
    asset = sim.assets[0]
    off = np.array([0.1, 0.05, -0.08])
    sens = []
    for b in range(len(asset.bodies)):
        gym.create_asset_force_sensor(asset, b, _transform(off, (0, 0, 0, 1)), _props(world=True))
        sens.append((b, off, np.array([0.0, 0.0, 0.0, 1.0]), True))
    pr = Probe(gym, sim, envs, 0, sens)
    for _ in range(360):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_rigid_body_state_tensor(sim)
    frames = []
    for _ in range(5):
        rb0, rb1, _, got = pr.step()
        frames.append((rb0, rb1, got))
    pairs = [(a, b) for a, b, _ in frames]
    g = pr.gravity
    worst = 0.0
    for e in range(2):
        g0 = pr.g0[e]
        for s, (b, p, q, _) in enumerate(sens):
            for rb0, rb1, got in frames:
                o_s = rb1[g0 + b, 0:3] + qmat(rb1[g0 + b, 3:7]) @ p
                Fw, Tw = np.zeros(3), np.zeros(3)
                for k in pr.sub[s]:
                    m, com, _ = pr.props[e][k]
                    c = rb1[g0 + k, 0:3] + qmat(rb1[g0 + k, 3:7]) @ com
                    Fw += -m * g
                    Tw += np.cross(c - o_s, -m * g)
                _, _, tf, tt = pr.reference(e, s, rb0, rb1)
                lin, ang = _unsteadiness(pr, e, pr.sub[s], pairs, o_s)
                row = got[pr.rows[e][s]]
                ef, et = np.linalg.norm(row[0:3] - Fw), np.linalg.norm(row[3:6] - Tw)
                worst = max(worst, ef / (tf + lin), et / (tt + ang))
                assert ef <= tf + lin, ("force", e, s, row[0:3], Fw, tf, lin)
                assert et <= tt + ang, ("torque", e, s, row[3:6], Tw, tt, ang)
                assert np.linalg.norm(Fw) >= 100 * (tf + lin), ("force too small for its tolerance", s, Fw, tf, lin)
                assert np.linalg.norm(Tw) >= 100 * (tt + ang), ("torque too small for its tolerance", s, Tw, tt, ang)
        assert pr.sub[0] == list(range(pr.nb))                # the base sensor carries the whole arm
    print("franka statics: worst err / (tol + unsteadiness) %.3f" % worst)
    gym.destroy_sim(sim)


def test_static_prismatic_load(gym, tmp_path):
    """A 2 kg load on a vertical POS drive reads m g along +z (what the base exerts on it)."""
    from test_dof_force_gpu import LIFT_URDF
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
    gym.create_asset_force_sensor(asset, 1, gymapi.Transform(), _props(world=True))
    sens = [(1, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), True)]
    n, M = 4, 2.0
    envs = []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 2)
        h = gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 1.0)), "lift", i, 1)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:], props["damping"][:] = 1000.0, 100.0
        gym.set_actor_dof_properties(env, h, props)
        envs.append(env)
    pr = Probe(gym, sim, envs, 0, sens)
    tg = torch.full((n,), 0.2, dtype=torch.float32, device=DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(240):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_rigid_body_state_tensor(sim)
    frames = [pr.step()[:2] + (pr.fs.cpu().numpy().astype(np.float64),) for _ in range(5)]
    pairs = [(a, b) for a, b, _ in frames]
    for e in range(n):
        lin, _ = _unsteadiness(pr, e, [1], pairs)
        for rb0, rb1, got in frames:
            _, _, tf, _ = pr.reference(e, 0, rb0, rb1)
            row = got[pr.rows[e][0]]
            err = np.linalg.norm(row[0:3] - np.array([0.0, 0.0, M * G]))
            assert err <= tf + lin, (e, row, tf, lin)
            assert M * G >= 100 * (tf + lin)
    gym.destroy_sim(sim)


# ------------------------------- 4: the contact moment against the DOF force
ARM_URDF = """<robot name="arm">
<link name="base"><inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
<link name="arm"><inertial><origin xyz="0.3 0 0"/><mass value="1"/><inertia ixx="0.001" iyy="0.03" izz="0.03" ixy="0" ixz="0" iyz="0"/></inertial>
<collision><origin xyz="0.3 0 0"/><geometry><box size="0.6 0.05 0.05"/></geometry></collision></link>
<joint name="hinge" type="revolute"><parent link="base"/><child link="arm"/><origin xyz="0 0 0"/><axis xyz="0 1 0"/>
<limit lower="-1" upper="1" effort="1000" velocity="10"/></joint></robot>"""
ARM_M, ARM_COM, ARM_TIP = 1.0, 0.3, 0.55


def _arm_scene(gym, tmp_path, n, sensors):
    """Coupled envs: a one-hinge arm (axis +y: a positive angle lowers the tip),
    POS drive towards 0.06 rad, its tip resting on a static box whose top lies
    5 mm under the horizontal arm's underside. sensors: ForceSensorProperties
    and local poses on the arm body. Returns (sim, envs, arm body rows)."""
    (tmp_path / "arm.urdf").write_text(ARM_URDF)
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -G)
    sp.dt, sp.substeps = 1.0 / 60.0, 2
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 8
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    arm = gym.load_asset(sim, str(tmp_path), "arm.urdf", opts)
    block = gym.create_box(sim, 0.1, 0.1, 0.1, opts)
    for pose, props in sensors:
        gym.create_asset_force_sensor(arm, 1, pose, props)
    envs, rows = [], []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 2)
        h = gym.create_actor(env, arm, gymapi.Transform(gymapi.Vec3(0, 0, 0.5)), "arm", i, 0)
        dp = gym.get_actor_dof_properties(env, h)
        dp["driveMode"][:] = gymapi.DOF_MODE_POS
        dp["stiffness"][:], dp["damping"][:] = 100.0, 10.0
        gym.set_actor_dof_properties(env, h, dp)
        gym.create_actor(env, block, gymapi.Transform(gymapi.Vec3(ARM_TIP, 0, 0.5 - 0.025 - 0.005 - 0.05)), "block", i, 0)
        assert gym.enable_actor_dof_force_sensors(env, h) is True
        rows.append(gym.find_actor_rigid_body_index(env, h, "arm", gymapi.DOMAIN_SIM))
        envs.append(env)
    return sim, envs, rows


def _settle_arm(gym, sim, n, frames=240):
    tg = torch.full((n,), 0.06, dtype=torch.float32, device=DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    for _ in range(frames):
        gym.simulate(sim)
    gym.fetch_results(sim, True)


def test_contact_moment_matches_dof_force(gym, tmp_path):
    """The arm resting its tip on the box: the hinge-axis component of the arm
    sensor's torque (sensor at the joint origin) is the drive torque the DOF
    force tensor reports — the parent's code — so the contact moment
    k_env_step keeps is the contacts' true moment. Tolerance: the arm's
    angular unsteadiness (|c - o| m |dv| + I |dw|) / dt over the 20 frames plus
    4 x the frame-to-frame spread of the DOF force readings."""
    n = 4
    sim, envs, arm_rows = _arm_scene(gym, tmp_path, n, [(gymapi.Transform(), _props(world=True))])
    sens = [(1, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), True)]
    pr = Probe(gym, sim, envs, 0, sens)
    assert N.lib.mg_num_coupled_envs(sim.native) == n
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    frc = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
    _settle_arm(gym, sim, n)
    gym.refresh_rigid_body_state_tensor(sim)
    recs = []
    for _ in range(20):
        rb0, rb1, ncf, got = pr.step()
        gym.refresh_dof_force_tensor(sim)
        gym.refresh_dof_state_tensor(sim)
        recs.append((rb0, rb1, ncf, got, frc.cpu().numpy().astype(np.float64), dof.cpu().numpy().astype(np.float64)))
    pairs = [(r[0], r[1]) for r in recs]
    for e in range(n):
        q = np.array([r[5][e, 0] for r in recs])
        assert np.all(q > 0.002) and np.all(q < 0.05), q         # resting on the box, far from the limits
        tau = np.array([r[4][e] for r in recs])
        spread = tau.max() - tau.min()
        o = recs[-1][1][pr.g0[e] + 1, 0:3]
        _, ang = _unsteadiness(pr, e, [1], pairs, o)
        lin, _ = _unsteadiness(pr, e, [1], pairs)
        tol = ang + 4.0 * spread
        for rb0, rb1, ncf, got, f, _ in recs:
            row = got[pr.rows[e][0]]
            fz = ncf[arm_rows[e], 2]
            share = 0.5 * fz                                      # the contact's moment about the hinge, at least (the box begins at x = 0.5)
            assert abs(row[4] - f[e]) <= tol, (e, row[4], f[e], tol, ang, spread)
            assert share >= 20 * tol, (e, share, tol)
            # the vertical force: the joint carries the weight the box does not
            _, _, tf, _ = pr.reference(e, 0, rb0, rb1, cf=ncf)
            assert abs(row[2] - (ARM_M * G - fz)) <= tf + lin, (e, row[2], ARM_M * G - fz, tf, lin)
        print("arm env %d: tau_y sensor %.6f, DOF force %.6f, tol %.3g (unsteadiness %.3g, spread %.3g), contact share %.4g"
              % (e, recs[-1][3][pr.rows[e][0]][4], recs[-1][4][e], tol, ang, spread, 0.5 * recs[-1][2][arm_rows[e], 2]))
    gym.destroy_sim(sim)


# -------------------------------------------------------- 5: parts and frames
def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_parts_and_frames_arm(gym, tmp_path):
    """On the arm scene: forward-dynamics part + constraint part = both within
    4 ulp of the larger part (the kernel adds the two parts once, after turning
    each into the sensor frame); both off reads exactly 0; the world-frame
    reading is the local one rotated (float64; 2 x 19 roundings of the two
    fp32 rotations apart)."""
    n = 4
    rng = np.random.RandomState(4)
    p, q = _rand_pose(rng)
    pose = _transform(p, q)
    kinds = [_props(), _props(cs=False), _props(fd=False), _props(fd=False, cs=False), _props(world=True),
             _props(cs=False, world=True), _props(fd=False, world=True)]
    sim, envs, _ = _arm_scene(gym, tmp_path, n, [(pose, k) for k in kinds])
    sens = [(1, p, q, k.use_world_frame) for k in kinds]
    pr = Probe(gym, sim, envs, 0, sens)
    _settle_arm(gym, sim, n, frames=30)                           # still moving: both parts are large
    gym.refresh_rigid_body_state_tensor(sim)
    for _ in range(5):
        rb0, rb1, ncf, _ = pr.step()
        got32 = pr.fs.cpu().numpy()
        for e in range(n):
            both, fd, cs, off, world, wfd, wcs = (got32[pr.rows[e][k]] for k in range(7))
            assert np.all(off == 0.0)
            assert np.abs(cs).max() > 0.1 and np.abs(fd).max() > 0.1
            for whole, a, b in ((both, fd, cs), (world, wfd, wcs)):
                larger = np.maximum(np.abs(a), np.abs(b))
                assert np.all(np.abs(whole.astype(np.float64) - (a.astype(np.float64) + b)) <= 4 * _ulp(larger))
            R = qmat(qmul(rb1[pr.g0[e] + 1, 3:7], q))
            for lo in (0, 3):
                w = R @ both[lo:lo + 3].astype(np.float64)
                assert np.abs(w - world[lo:lo + 3]).max() <= 2 * 19 * U * np.linalg.norm(w)
    gym.destroy_sim(sim)


def test_ant_torso_reads_zero_at_rest(gym):
    """A floating base's root sensor: nothing holds the ant but the ground, whose
    wrench the reading takes out, so at rest it reads force and torque below the
    unsteadiness of the pose (plus the identity's rounding bound): measured
    |F| 2.8e-5 N (bound 8.2e-4), |T| 1.3e-5 N m (bound 6.6e-4) on the 8.9 N ant.

    The asset's angular damping is off here. The step's resting state keeps a
    root angular velocity of 6.5e-3 rad/s that the pose does not follow (the
    velocity sweep's remainder), and AssetOptions' default damping of 0.5 / s
    scales it down every substep: a drag against the world that no force row
    records. It acts through v+, so it shows in the reading (measured with the
    default: 4.4e-4 to 8.0e-4 N and 1.5e-3 N m, constant from frame to frame,
    above the bound)."""
    opts = gymapi.AssetOptions()
    opts.angular_damping = 0.0
    sim, info, sens = _ant(gym, 1, height=0.45, props=_props(world=True), asset_options=opts)
    pr = Probe(gym, sim, info["envs"], 0, sens)
    # held at the middle of every joint's range, clear of the limit rows and
    # the limit clamp (an ant left to sag rests its ankles on their limits)
    dp = gym.get_actor_dof_properties(info["envs"][0], info["actors"][0])
    mid = torch.from_numpy((0.5 * (dp["lower"] + dp["upper"])).astype(np.float32)).to(DEV)
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(mid))
    for _ in range(300):
        gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_rigid_body_state_tensor(sim)
    frames = [pr.step() for _ in range(5)]
    pairs = [(f[0], f[1]) for f in frames]
    torso = len(sens) - 1
    assert pr.sub[torso] == list(range(pr.nb))
    for rb0, rb1, ncf, got in frames:
        o_s = rb1[pr.g0[0], 0:3] + qmat(rb1[pr.g0[0], 3:7]) @ sens[torso][1]
        lin, ang = _unsteadiness(pr, 0, pr.sub[torso], pairs, o_s)
        # the contact moment is no public tensor: its size is bounded by lever x force
        _, _, tf, tt = pr.reference(0, torso, rb0, rb1, cf=ncf)
        row = got[pr.rows[0][torso]]
        weight = sum(m for m, _, _ in pr.props[0]) * 9.81
        print("ant torso at rest: F %s |F| %.3g (bound %.3g), T %s |T| %.3g (bound %.3g), weight %.4g, root |w| %.3g"
              % (row[0:3], np.linalg.norm(row[0:3]), tf + lin, row[3:6], np.linalg.norm(row[3:6]), tt + ang, weight,
                 np.linalg.norm(rb1[pr.g0[0], 10:13])))
        assert np.abs(ncf[pr.g0[0]:pr.g0[0] + pr.nb, 2]).sum() > 0.5 * weight      # it stands on the ground
        dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
        gym.refresh_dof_state_tensor(sim)
        q = dof[:, 0].cpu().numpy()
        margin = 0.05 * (dp["upper"] - dp["lower"])
        assert np.all(q > dp["lower"] + margin) and np.all(q < dp["upper"] - margin), q     # no limit row, no clamp
        assert np.linalg.norm(row[0:3]) <= tf + lin
        assert np.linalg.norm(row[3:6]) <= tt + ang
    gym.destroy_sim(sim)


# ----------------------------------------------------------------- 6: set frames
def test_set_frames_read_zero(gym):
    """4 gimbals and a twin sim. The sim's first frame reads 0. After
    set_dof_state_tensor_indexed on env 1, env 1's sensors read exactly 0 for
    one frame while the other envs equal the twin bit for bit; the frame after,
    env 1 passes the identity again. A set of identical values zeroes nothing."""
    n = 4
    sims = []
    for _ in range(2):
        sim, envs = _gimbal(gym, n)
        sens = _sensor_every_body(gym, sim.assets[0])
        sims.append((sim, Probe(gym, sim, envs, 0, sens), _wave_targets(gym, sim, 0.3, 0.35)))
    (sa, pa, wa), (sb, pb, wb) = sims
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sa))
    idx = torch.tensor([1], dtype=torch.int32, device=DEV)
    ns = len(pa.sensors)
    for k in range(8):
        wa(k)
        wb(k)
        if k == 3:       # env 1 of sim a: a new DOF state
            gym.refresh_dof_state_tensor(sa)
            new = dof.clone()
            new[3:6, 0] += 0.2
            new[3:6, 1] = 0.0
            assert gym.set_dof_state_tensor_indexed(sa, gymtorch.unwrap_tensor(new), gymtorch.unwrap_tensor(idx), 1)
        if k == 6:       # the same values again: not a change
            gym.refresh_dof_state_tensor(sa)
            assert gym.set_dof_state_tensor_indexed(sa, gymtorch.unwrap_tensor(dof.clone()),
                                                    gymtorch.unwrap_tensor(idx), 1)
        rb0, rb1, _, ga = pa.step()
        _, _, _, gb = pb.step()
        ga, gb = ga.reshape(n, ns, 6), gb.reshape(n, ns, 6)
        if k == 0:
            assert np.all(ga == 0.0) and np.all(gb == 0.0)
        elif k == 3:
            assert np.all(ga[1] == 0.0)
            assert np.array_equal(ga[[0, 2, 3]], gb[[0, 2, 3]]) and np.abs(gb[1]).max() > 0.1
        else:
            assert np.abs(ga[1]).max() > 0.1, k
            if k < 3:
                assert np.array_equal(ga, gb)
            else:
                assert np.array_equal(ga[[0, 2, 3]], gb[[0, 2, 3]])
                for s in range(ns):     # env 1 again obeys the identity (also after the no-op set)
                    Fr, Tr, tf, tt = pa.reference(1, s, rb0, rb1)
                    assert np.abs(ga[1, s, 0:3] - Fr).max() <= tf and np.abs(ga[1, s, 3:6] - Tr).max() <= tt, (k, s)
    gym.destroy_sim(sa)
    gym.destroy_sim(sb)


# ------------------------------------------------------ 7: trajectory untouched
def _traj_scene(gym, name, n, sensors):
    from test_dof_force_gpu import _franka_alone
    if name == "gimbal":
        sim, envs = _gimbal(gym, n)
        asset = sim.assets[0]
    elif name == "franka":
        sim, envs = _franka_alone(gym, n, substeps=2)
        asset = sim.assets[0]
    elif name == "cube_pick":
        sim, info = scenes.franka_scene(gym, n, controller="ik")
        envs, asset = info["envs"], sim.envs[0].actors[2].asset
    else:
        sim, info = scenes.ant_scene(gym, n, height=0.6)
        envs, asset = info["envs"], info["asset"]
        for env, a in zip(envs, info["actors"]):
            dp = gym.get_actor_dof_properties(env, a)
            dp["driveMode"][:] = gymapi.DOF_MODE_POS
            dp["stiffness"][:], dp["damping"][:] = 20.0, 1.0
            gym.set_actor_dof_properties(env, a, dp)
    if sensors:
        _sensor_every_body(gym, asset)
    return sim


@pytest.mark.parametrize("name", ["gimbal", "franka", "cube_pick", "ant"])
def test_sensors_leave_the_trajectory_alone(gym, name):
    """Two sims of one scene, one with a sensor on every articulation body: root,
    rigid-body and DOF states bit-identical after 60 frames."""
    n = 4
    runs = []
    for sensors in (False, True):
        sim = _traj_scene(gym, name, n, sensors)
        gym.prepare_sim(sim)
        fs = gymtorch.wrap_tensor(gym.acquire_force_sensor_tensor(sim))
        dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
        root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
        rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        assert N.lib.mg_num_force_sensors(sim.native) == fs.shape[0] and (fs.shape[0] > 0) == sensors
        before = _wave_targets(gym, sim, 0.1, 0.3)
        seen = 0.0
        for k in range(60):
            before(k)
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            gym.refresh_force_sensor_tensor(sim)
            seen = max(seen, float(fs.abs().max()) if sensors else 0.0)
        gym.refresh_dof_state_tensor(sim)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        runs.append((root.clone(), rb.clone(), dof.clone(), seen))
        gym.destroy_sim(sim)
    (ra, ba, da, _), (rb_, bb, db, seen) = runs
    assert torch.equal(ra, rb_) and torch.equal(ba, bb) and torch.equal(da, db)
    assert seen > 0.1 and math.isfinite(seen)


# ------------------------------------------- 8: graph capture, the CPU pipeline
def _eager_gimbal_rows(gym, gpu, frames=5):
    n = 4
    sim, envs = _gimbal(gym, n, use_gpu_pipeline=gpu)
    _sensor_every_body(gym, sim.assets[0])
    gym.prepare_sim(sim)
    fs = gymtorch.wrap_tensor(gym.acquire_force_sensor_tensor(sim))
    tg = torch.tensor([0.3, -0.2, 0.1] * n, dtype=torch.float32, device=DEV if gpu else "cpu")
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    return sim, envs, fs


def test_graph_capture_matches_eager(gym):
    """simulate + refresh_force_sensor_tensor captured into a graph and replayed
    5 times gives the eager readings bit for bit; the table cannot change
    after the capture."""
    sim, _, fs = _eager_gimbal_rows(gym, True)
    eager = []
    for _ in range(5):
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_force_sensor_tensor(sim)
        eager.append(fs.clone())
    gym.destroy_sim(sim)
    assert float(eager[0].abs().max()) == 0.0 and float(eager[4].abs().max()) > 0.1
    assert not torch.equal(eager[2], eager[4])

    sim, _, fs = _eager_gimbal_rows(gym, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            gym.refresh_force_sensor_tensor(sim)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(5):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(fs, eager[k]), "replay %d" % k
    assert N.lib.mg_set_force_sensors(sim.native, None, 0) == -3        # MG_ERR_STATE
    assert "captured into a graph" in N.last_error()
    assert N.lib.mg_num_force_sensors(sim.native) == fs.shape[0]
    gym.destroy_sim(sim)


def test_cpu_pipeline_matches_gpu_pipeline(gym):
    """use_gpu_pipeline = False: a page-locked host tensor with the GPU pipeline's values."""
    got = {}
    for gpu in (True, False):
        sim, envs, fs = _eager_gimbal_rows(gym, gpu)
        assert fs.device.type == ("cuda" if gpu else "cpu")
        if not gpu:
            assert fs.is_pinned()
        rows = []
        for _ in range(5):
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            assert gym.refresh_force_sensor_tensor(sim) is True
            rows.append(fs.cpu().numpy().copy())
        w = gym.get_actor_force_sensor(envs[2], 0, 1).get_forces()
        r = rows[-1][2 * 4 + 1]
        assert (np.float32(w.force.x), np.float32(w.force.y), np.float32(w.force.z)) == tuple(r[0:3])
        assert (np.float32(w.torque.x), np.float32(w.torque.y), np.float32(w.torque.z)) == tuple(r[3:6])
        got[gpu] = np.stack(rows)
        gym.destroy_sim(sim)
    assert np.abs(got[True]).max() > 0.1
    assert np.array_equal(got[True], got[False])
