"""Scenes that reach the step kernels' fixed capacities,
shared by tests/test_capacity_api.py (oracle, CPU) and
tests/test_capacity_gpu.py (the device's capacity report). Every builder adds
one env to a sim made by new_sim(); all use pile_scenes.sim_params (z-up, dt
1/60, 2 substeps, TGS 6/1, contact offset 0.01 unless given)."""
import os

import numpy as np

from isaacgym import gymapi
from test_isaacgym_amd import _native as N
import oracle
import pile_scenes as PS


def new_sim(gym, gpu, **kw):
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, PS.sim_params(gpu, **kw))
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, plane)
    return sim


def _env(gym, sim):
    return gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 1), 4)


def _fixed():
    o = gymapi.AssetOptions()
    o.fix_base_link = True
    return o


def add_sphere_layer(gym, sim, group, n):
    """An n x n layer of touching spheres (r 0.05, pitch 0.102) just above the
    ground: n^2 ground pairs + 2 n (n - 1) neighbour pairs, one point each.
    8 x 8: 176 active pairs against the 128 of a pile env; 6 x 6: 96."""
    ball = gym.create_sphere(sim, 0.05, gymapi.AssetOptions())
    env = _env(gym, sim)
    for k in range(n * n):
        gym.create_actor(env, ball, gymapi.Transform(gymapi.Vec3(0.102 * (k % n), 0.102 * (k // n), 0.051)),
                         None, group, 0)
    return env


def add_cube_block(gym, sim, group, n):
    """An n x n x n block of touching 0.1 m cubes on the ground
    (tests/test_pile_gpu.py test_overflowing_block_parity_gpu's scene; contact
    offset 0.02 there and here). 4 x 4 x 4: 16 ground pairs + 144 face pairs,
    4 points each = 640 candidate points against the 256 of a pile env."""
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    env = _env(gym, sim)
    for k in range(n ** 3):
        x, y, z = k % n, (k // n) % n, k // (n * n)
        gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.1 * x + 0.001 * group, 0.1 * y, 0.05 + 0.1 * z)),
                         None, group, 0)
    return env


def add_tray(gym, sim, group, nballs, fixed_box):
    """A free tray (body 0 of the env) that carries nballs spheres, rests on the
    ground and (fixed_box) leans on a fixed box: 1 + fixed_box + nballs active
    pairs on the tray against a pile env's 64 colours."""
    tray = gym.create_box(sim, 1.0, 1.0, 0.1, gymapi.AssetOptions())
    stop = gym.create_box(sim, 0.2, 0.2, 0.2, _fixed())
    ball = gym.create_sphere(sim, 0.04, gymapi.AssetOptions())
    env = _env(gym, sim)
    gym.create_actor(env, tray, gymapi.Transform(gymapi.Vec3(0, 0, 0.05)), "tray", group, 0)
    if fixed_box:
        gym.create_actor(env, stop, gymapi.Transform(gymapi.Vec3(0.602, 0, 0.1)), "stop", group, 0)
    for k in range(nballs):
        gym.create_actor(env, ball, gymapi.Transform(gymapi.Vec3(-0.385 + 0.11 * (k % 8), -0.385 + 0.11 * (k // 8),
                                                                 0.141)), None, group, 0)
    return env


# the coupled scene's boxes: half extents, centre (env frame)
TABLE = ((0.5, 0.5, 0.1), (0.0, 0.0, 0.1))
CUBES = (((0.05, 0.05, 0.05), (0.0, 0.0, 0.25)), ((0.05, 0.05, 0.05), (0.3, 0.0, 0.25)))
WALLS = (((0.4, 0.05, 0.15), (0.15, 0.101, 0.35)), ((0.05, 0.2, 0.15), (-0.101, 0.0, 0.35)),
         ((0.05, 0.2, 0.15), (0.401, 0.0, 0.35)))


def add_walled_cubes(gym, sim, group, nwalls):
    """A fixed table, two free cubes on it and nwalls of the three fixed walls
    within the contact offset of the cubes' faces: a coupled env (k_env_step)
    of 8 + 4 (nwalls + 1) contacts for nwalls >= 1 (16 / 20 / 24) against its
    table of 16. Bodies in order: table, cube A, cube B, the walls."""
    env = _env(gym, sim)
    h, c = TABLE
    gym.create_actor(env, gym.create_box(sim, 2 * h[0], 2 * h[1], 2 * h[2], _fixed()),
                     gymapi.Transform(gymapi.Vec3(*c)), "table", group, 0)
    for h, c in CUBES:
        gym.create_actor(env, gym.create_box(sim, 2 * h[0], 2 * h[1], 2 * h[2], gymapi.AssetOptions()),
                         gymapi.Transform(gymapi.Vec3(*c)), None, group, 0)
    for h, c in WALLS[:nwalls]:
        gym.create_actor(env, gym.create_box(sim, 2 * h[0], 2 * h[1], 2 * h[2], _fixed()),
                         gymapi.Transform(gymapi.Vec3(*c)), None, group, 0)
    return env


def walled_contacts(rows, nwalls, margin=0.01):
    """oracle.collide's contact count of one walled-cubes env from its
    rigid-body rows (table, cube A, cube B, walls): every cube against the
    table, the other cube and every wall."""
    half = [TABLE[0], CUBES[0][0], CUBES[1][0]] + [w[0] for w in WALLS[:nwalls]]
    shp = [np.concatenate([[N.MG_SHAPE_BOX], rows[i, 0:7], half[i]]).astype(np.float32) for i in range(3 + nwalls)]
    pairs = [(1, 0), (2, 0), (1, 2)] + [(c, 3 + w) for w in range(nwalls) for c in (1, 2)]
    return sum(len(oracle.collide(shp[a], shp[b], margin)) for a, b in pairs)


def slab_urdf(d, name, xs):
    """A free body of one collision box 0.2 x 0.2 x 0.1 at each x of xs (in
    that order), mass 1, as a URDF in d."""
    boxes = "".join('<collision><origin xyz="%g 0 0"/><geometry><box size="0.2 0.2 0.1"/></geometry></collision>' % x
                    for x in xs)
    with open(os.path.join(d, name + ".urdf"), "w") as f:
        f.write('<robot name="%s"><link name="body">%s<inertial><mass value="1"/><inertia ixx="0.0042" iyy="0.031" '
                'izz="0.033" ixy="0" ixz="0" iyz="0"/></inertial></link></robot>' % (name, boxes))
    return name + ".urdf"


def add_slab(gym, sim, group, d, xs):
    """The slab alone in its env (the free-body kernel's multi-shape launch),
    dropped from z = 0.052: 4 ground candidates per box against 8 slots."""
    asset = gym.load_asset(sim, d, slab_urdf(d, "slab%d" % len(xs), xs), gymapi.AssetOptions())
    env = _env(gym, sim)
    gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 0.052)), "slab", group, 0)
    return env


THREE_BOXES = (-0.2, 0.2, 0.0)
TWO_BOXES = (-0.2, 0.2)


def oracle_run(sim, frames):
    """`frames` oracle steps of the sim's model; returns the state and the
    last net contact forces."""
    A = sim.build_model()
    p, m = sim.mg_params(), sim.mg_model()
    st = A["body_state0"].copy()
    dof = A["dof_state0"].copy()
    cf = None
    for _ in range(frames):
        cf = oracle.step(p, m, st, dof)
    return st, cf
