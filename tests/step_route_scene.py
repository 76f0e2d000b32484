"""The mixed-owner scene of tests/test_step_route_gpu.py, shared with the script
that recorded tests/golden/step_route_mixed.json: 3 uncoupled envs, each a
fixed-base servo/gimbal.urdf and a fixed-base 2-link hinge chain (one hinge); an attractor
on the camera link of env 1's gimbal, DOF friction on env 2's chain, DOF forces
reported by every actor. Owners of both kinds in different articulation groups of
one sim: both read the one split table."""
import numpy as np
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import scenes

from joint_friction64 import hinge_chain_urdf

ENVS, FRAMES, KEEP = 3, 20, (1, 10, 20)
ATTR_ENV, FRIC_ENV, TAU_F = 1, 2, 0.05
TENSORS = ("root", "rb", "dof", "frc")


def sim_params():
    sp = gymapi.SimParams()
    sp.dt = 1.0 / 60.0
    sp.substeps = 2
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.gravity = gymapi.Vec3(0.0, 0.0, -9.81)
    sp.physx.solver_type = 1
    sp.physx.num_position_iterations = 4
    sp.physx.num_velocity_iterations = 1
    sp.use_gpu_pipeline = True
    return sp


def build(gym, tmp_path):
    """-> sim, [(env, gimbal, chain)]; prepared, targets set."""
    (tmp_path / "hinge1.urdf").write_text(hinge_chain_urdf(1))
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sim_params())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.default_dof_drive_mode = gymapi.DOF_MODE_POS
    gimbal = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/gimbal.urdf", opts)
    copts = gymapi.AssetOptions()
    copts.fix_base_link = True
    copts.armature = 0.0
    chain = gym.load_asset(sim, str(tmp_path), "hinge1.urdf", copts)
    handles = []
    for i in range(ENVS):
        env = gym.create_env(sim, gymapi.Vec3(-1.0, -1.0, -1.0), gymapi.Vec3(1.0, 1.0, 1.0), 2)
        pose = gymapi.Transform()
        pose.p = gymapi.Vec3(0.0, 2.0, 3.0)
        hg = gym.create_actor(env, gimbal, pose, "gimbal", i, 1)
        props = gym.get_actor_dof_properties(env, hg)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:] = 50.0
        props["damping"][:] = 5.0
        gym.set_actor_dof_properties(env, hg, props)
        pose.p = gymapi.Vec3(0.0, -2.0, 6.0)
        hc = gym.create_actor(env, chain, pose, "chain", i, 1)
        props = gym.get_actor_dof_properties(env, hc)
        props["driveMode"][:] = gymapi.DOF_MODE_NONE
        for k in ("stiffness", "damping", "effort", "velocity"):
            props[k][:] = 0.0
        props["armature"][:] = 0.005
        props["friction"][:] = TAU_F if i == FRIC_ENV else 0.0
        gym.set_actor_dof_properties(env, hc, props)
        st = gym.get_actor_dof_states(env, hc, gymapi.STATE_ALL)
        st["pos"][:], st["vel"][:] = 0.3 + 0.1 * i, 1.5 - 0.5 * i
        gym.set_actor_dof_states(env, hc, st, gymapi.STATE_ALL)
        for h in (hg, hc):
            assert gym.enable_actor_dof_force_sensors(env, h) is True
        if i == ATTR_ENV:
            p = gymapi.AttractorProperties()
            p.stiffness, p.damping, p.axes = 200.0, 20.0, gymapi.AXIS_TRANSLATION
            p.rigid_handle = gym.find_actor_rigid_body_handle(env, hg, "camera_link")
            p.target = gymapi.Transform(gymapi.Vec3(0.05, 2.02, 3.1), None)
            assert gym.create_rigid_body_attractor(env, p) == 0
        handles.append((env, hg, hc))
    gym.prepare_sim(sim)
    nd = gym.get_sim_dof_count(sim)
    tg = torch.zeros(nd, dtype=torch.float32, device="cuda:0")
    tg.view(ENVS, 4)[:, :3] = torch.tensor([0.3, -0.2, 0.1], device="cuda:0")
    assert gym.set_dof_position_target_tensor(sim, gymtorch.unwrap_tensor(tg))
    return sim, handles


def run(gym, sim, graph_from=None):
    """The root, rigid-body, DOF-state and DOF-force tensors after frames KEEP, as
    int32 bit patterns: {frame: {name: array}}. graph_from: frames from that one on
    are replays of one captured frame."""
    t = dict(root=gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim)),
             rb=gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim)),
             dof=gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim)),
             frc=gymtorch.wrap_tensor(gym.acquire_dof_force_tensor(sim)))

    def frame():
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_dof_state_tensor(sim)
        gym.refresh_dof_force_tensor(sim)

    out, g = {}, None
    for k in range(1, FRAMES + 1):
        if graph_from is not None and k >= graph_from:
            if g is None:
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(g, stream=side):
                        frame()
                torch.cuda.current_stream().wait_stream(side)
            g.replay()
        else:
            frame()
        torch.cuda.synchronize()
        if k in KEEP:
            out[k] = {n: t[n].cpu().numpy().astype(np.float32).view(np.int32).copy() for n in TENSORS}
    return out


def add_attractor_on_friction_chain(gym, handles):
    env, _, hc = handles[FRIC_ENV]
    p = gymapi.AttractorProperties()
    p.stiffness, p.damping, p.axes = 100.0, 10.0, gymapi.AXIS_TRANSLATION
    p.rigid_handle = gym.find_actor_rigid_body_handle(env, hc, "r0")
    p.target = gymapi.Transform(gymapi.Vec3(0.0, -2.0, 5.8), None)
    assert gym.create_rigid_body_attractor(env, p) == 0
