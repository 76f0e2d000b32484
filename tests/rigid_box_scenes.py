"""Scenes for the tests of the free-body step's box-only build
(tests/test_rigid_box_only.py, tests/test_rigid_box_only_gpu.py; DESIGN.md
§3.2): two single-body actors per env on the servo scene's ground and grid, no
pair of which can touch (collision filter -1, as scenes.servo_scene).

  servo        UAV then vehicle in every env (the actors of scenes.servo_scene)
  alternating  even envs UAV then vehicle, odd envs vehicle then UAV
  ball         vehicle then assets/urdf/ball.urdf in every env
  other        vehicle then the URDF named by `other` = (root directory, file)

build() returns (sim, vehicle rows, ball rows): the actor rows of the vehicles
and of the balls."""
import math

import numpy as np

from isaacgym import gymapi
from test_isaacgym_amd import scenes

UAV, VEHICLE, BALL, OTHER = "servo/uav.urdf", "servo/ground_vehicle.urdf", "urdf/ball.urdf", "other"
POSE = {UAV: (-10.0, 0.0, 102.0), VEHICLE: (0.0, 0.0, 2.0), BALL: (4.0, 6.0, 1.0), OTHER: (4.0, 6.0, 1.0)}
ORDERS = {
    "servo": lambda e: (UAV, VEHICLE),
    "alternating": lambda e: (UAV, VEHICLE) if e % 2 == 0 else (VEHICLE, UAV),
    "ball": lambda e: (VEHICLE, BALL),
    "other": lambda e: (VEHICLE, OTHER),
}


def build(gym, kind, num_envs, use_gpu_pipeline=True, other=None):
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, scenes.servo_sim_params(use_gpu_pipeline))
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    plane.distance = 0
    plane.static_friction = 1
    plane.dynamic_friction = 1
    plane.restitution = 0
    gym.add_ground(sim, plane)
    assets = {}
    for f in sorted(set(ORDERS[kind](0)) | set(ORDERS[kind](1))):
        opts = gymapi.AssetOptions()
        opts.armature = 0.01
        root, name = other if f == OTHER else (scenes.ASSET_ROOT, f)
        assets[f] = gym.load_asset(sim, root, name, opts)
        assert assets[f] is not None
    per_row = int(math.sqrt(num_envs))
    lower, upper = gymapi.Vec3(-20.0, -20.0, -20.0), gymapi.Vec3(20.0, 20.0, 20.0)
    rows = {f: [] for f in POSE}
    row = 0
    for e in range(num_envs):
        env = gym.create_env(sim, lower, upper, per_row)
        for f in ORDERS[kind](e):
            pose = gymapi.Transform()
            pose.p = gymapi.Vec3(*POSE[f])
            gym.create_actor(env, assets[f], pose, "%s%d" % (f, e), e, -1)
            rows[f].append(row)
            row += 1
    return sim, np.array(rows[VEHICLE], np.int64), np.array(rows[BALL], np.int64)
