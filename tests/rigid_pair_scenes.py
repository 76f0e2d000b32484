"""Scenes for tests/test_rigid_packed_geometry_gpu.py beside those of
tests/rigid_box_scenes.py (the one-round free-body step's
geometry on packed pairs):

  yup_ball   a ground vehicle and assets/urdf/ball.urdf per env on Isaac Gym's
             default y-up ground (UP_AXIS_Y, gravity -y, plane normal +y): the
             step takes the general ground basis, not the +Z specialisation.
             The vehicle stands upright (its z axis on +y).

OFFCENTRE and OFFCENTRE_POSED name assets for the `other` scenes of
rigid_box_scenes.build(): a box whose <inertial> is displaced and turned
against the link frame (a non-zero centre-of-mass offset and a principal frame
that is not the identity), as a plain box and with its shape posed."""
import math
import os

import numpy as np

from isaacgym import gymapi
from test_isaacgym_amd import scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFFCENTRE = (GOLDEN, "offcentre_box.urdf")
OFFCENTRE_POSED = (GOLDEN, "offcentre_posed_box.urdf")   # the same, its shape posed against the link frame
UPRIGHT = (-math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5))   # x y z w: the body's z axis on +y


def build_yup_ball(gym, num_envs):
    """Returns (sim, vehicle rows, ball rows): actor rows, vehicle then ball in every env."""
    sp = scenes.servo_sim_params(True)
    sp.up_axis = gymapi.UP_AXIS_Y
    sp.gravity = gymapi.Vec3(0.0, -9.8, 0.0)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 1, 0)
    plane.distance = 0
    plane.static_friction = 1
    plane.dynamic_friction = 1
    plane.restitution = 0
    gym.add_ground(sim, plane)
    opts = gymapi.AssetOptions()
    opts.armature = 0.01
    veh = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/ground_vehicle.urdf", opts)
    ball = gym.load_asset(sim, scenes.ASSET_ROOT, "urdf/ball.urdf", opts)
    assert veh is not None and ball is not None
    per_row = int(math.sqrt(num_envs))
    lower, upper = gymapi.Vec3(-20.0, -20.0, -20.0), gymapi.Vec3(20.0, 20.0, 20.0)
    for e in range(num_envs):
        env = gym.create_env(sim, lower, upper, per_row)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 2.0, 0.0)
        pose.r = gymapi.Quat(*UPRIGHT)
        gym.create_actor(env, veh, pose, "veh%d" % e, e, -1)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(4.0, 1.0, 6.0)
        gym.create_actor(env, ball, pose, "ball%d" % e, e, -1)
    rows = np.arange(num_envs, dtype=np.int64)
    return sim, 2 * rows, 2 * rows + 1
