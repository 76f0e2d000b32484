"""DOF force tensor, host side (no device needed): the tensor's shape, dtype and
storage, and what enable_actor_dof_force_sensors answers."""
import numpy as np
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import scenes


def _box_scene(gym, n):
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -9.8)
    sp.use_gpu_pipeline = False
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    asset = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    envs, actors = [], []
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 2)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 0.0, 1.0)
        actors.append(gym.create_actor(env, asset, pose, "box", i, 0))
        envs.append(env)
    return sim, envs, actors


def test_gimbal_tensor_shape_and_storage():
    gym = gymapi.acquire_gym()
    n = 4
    sim, envs = scenes.gimbal_scene(gym, n, use_gpu_pipeline=False)
    try:
        assert gym.enable_actor_dof_force_sensors(envs[0], 0) is True
        assert gym.enable_actor_dof_force_sensors(envs[2], 0) is True
        gym.prepare_sim(sim)
        t = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
        assert t.dtype == torch.float32 and tuple(t.shape) == (3 * n,)
        assert tuple(t.view(n, 3).shape) == (n, 3)
        assert gym.get_sim_dof_count(sim) == 3 * n
        t2 = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
        assert t2.data_ptr() == t.data_ptr()
        assert float(t.abs().max()) == 0.0
        # after prepare_sim, before the first simulate: still allowed
        assert gym.enable_actor_dof_force_sensors(envs[1], 0) is True
        f = gym.get_actor_dof_forces(envs[0], 0)
        assert isinstance(f, np.ndarray) and f.dtype == np.float32 and f.shape == (3,)
    finally:
        gym.destroy_sim(sim)


def test_no_dofs_empty_tensor_and_enable_refused(capsys):
    gym = gymapi.acquire_gym()
    sim, envs, actors = _box_scene(gym, 2)
    try:
        assert gym.enable_actor_dof_force_sensors(envs[0], actors[0]) is False
        assert "no DOFs" in capsys.readouterr().err
        gym.prepare_sim(sim)
        t = gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim))
        assert t.dtype == torch.float32 and tuple(t.shape) == (0,) and t.numel() == 0
        assert gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim)).data_ptr() == t.data_ptr()
        assert gym.refresh_dof_force_tensor(sim) is True
        assert gym.get_actor_dof_forces(envs[0], actors[0]).shape == (0,)
    finally:
        gym.destroy_sim(sim)
