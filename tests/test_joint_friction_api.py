"""Joint friction, host side (no device needed): the importers'
values reach column 9 of the packed DOF property record, a negative friction is
refused where it is set, and the library exports the routing diagnostic."""
import ctypes

import numpy as np
import pytest

from isaacgym import gymapi
from test_isaacgym_amd import _native as N

URDF = """<robot name="fr"><link name="base"/>
<link name="a"><inertial><origin xyz="0 0 -0.1"/><mass value="1"/>
  <inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
<link name="b"><inertial><origin xyz="0 0 -0.1"/><mass value="1"/>
  <inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
<joint name="ja" type="revolute"><parent link="base"/><child link="a"/><axis xyz="0 1 0"/>
  <limit lower="-1" upper="1" effort="10" velocity="5"/><dynamics damping="0.1" friction="0.035"/></joint>
<joint name="jb" type="prismatic"><parent link="a"/><child link="b"/><axis xyz="0 0 1"/>
  <limit lower="-1" upper="1" effort="10" velocity="5"/></joint>
</robot>"""

MJCF = """<mujoco model="fl"><worldbody><body name="torso" pos="0 0 1"><freejoint/>
<geom type="sphere" size="0.1"/>
<body name="arm" pos="0.2 0 0"><joint name="j" type="hinge" axis="0 1 0" frictionloss="0.07"/>
<geom type="sphere" size="0.05"/></body></body></worldbody></mujoco>"""


def _sim(gym):
    sp = gymapi.SimParams()
    sp.up_axis = gymapi.UP_AXIS_Z
    sp.use_gpu_pipeline = False
    return gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)


def _one_actor(gym, tmp_path, name, text, fixed):
    (tmp_path / name).write_text(text)
    sim = _sim(gym)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = fixed
    asset = gym.load_asset(sim, str(tmp_path), name, opts)
    assert asset is not None
    env = gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 1)
    h = gym.create_actor(env, asset, gymapi.Transform(gymapi.Vec3(0, 0, 1)), "a", 0, 1)
    return sim, env, h


def test_urdf_friction_reaches_column_9(gym, tmp_path):
    sim, env, h = _one_actor(gym, tmp_path, "fr.urdf", URDF, True)
    props = gym.get_actor_dof_properties(env, h)
    assert np.allclose(props["friction"], [0.035, 0.0])
    A = sim.build_model()
    assert A["dof_props"].shape[1] == N.MG_DOFPROP_N
    assert np.allclose(A["dof_props"][:, 9], [0.035, 0.0])
    props["friction"][:] = [0.5, 2.0]              # N m on the hinge, N on the slider
    gym.set_actor_dof_properties(env, h, props)
    assert np.allclose(sim.build_model()["dof_props"][:, 9], [0.5, 2.0])


def test_mjcf_frictionloss_reaches_column_9(gym, tmp_path):
    sim, env, h = _one_actor(gym, tmp_path, "fl.xml", MJCF, False)
    assert np.allclose(gym.get_actor_dof_properties(env, h)["friction"], [0.07])
    assert np.allclose(sim.build_model()["dof_props"][:, 9], [0.07])


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf")])
def test_negative_friction_is_a_value_error(gym, tmp_path, bad):
    sim, env, h = _one_actor(gym, tmp_path, "fr.urdf", URDF, True)
    props = gym.get_actor_dof_properties(env, h)
    props["friction"][1] = bad
    props["stiffness"][:] = 7.0
    with pytest.raises(ValueError, match="friction"):
        gym.set_actor_dof_properties(env, h, props)
    kept = gym.get_actor_dof_properties(env, h)          # nothing of the refused set was applied
    assert np.allclose(kept["friction"], [0.035, 0.0]) and not np.any(kept["stiffness"] == 7.0)


def test_abi_symbol():
    assert "mg_joint_friction_stats" in N.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(lib, "mg_joint_friction_stats")
    out = (ctypes.c_int32 * 3)(7, 7, 7)
    assert N.lib.mg_joint_friction_stats(None, out) < 0          # a null sim is refused, never dereferenced
    assert "upload" in N.last_error() or "sim" in N.last_error()
    assert list(out) == [7, 7, 7]
