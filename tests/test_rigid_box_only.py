"""The layout planner's box-only flag (mg_layout.cpp plan_free_flags, DESIGN.md
§3.2), read through mg_debug_layout_table's MG_LAYOUT_FREE_FLAGS with no
device: 1 when every single-shape free body's shape is a box at the body origin
with the body's orientation (or absent), which lets a one-round free-body
launch run the build whose candidate search is compiled for that box alone.

  - the servo scene (two box proxies) at 1, 33 and 96 envs, and with its actors
    created in alternating order: 1;
  - a vehicle and a ball per env (a sphere among the shapes): 0;
  - the vehicle beside a box whose collision origin is shifted, and beside one
    whose collision origin is turned: 0 (the box build skips the shape's pose);
    beside the same box at the origin: 1.

The planner has no affine description of the slot records (runs of slots with
base + step per field): the kernel build that would have used one was measured
and left out, so there is no such table to test."""
import ctypes

import pytest

from test_isaacgym_amd import _native as N
import rigid_box_scenes as RS

BOX = """<robot name="b"><link name="b"><collision><origin xyz="%s" rpy="%s"/>
<geometry><box size="1 2 0.5"/></geometry></collision>
<inertial><mass value="10"/><inertia ixx="1" iyy="1" izz="1" ixy="0" ixz="0" iyz="0"/></inertial></link></robot>"""


def _flags(gym, kind, n, other=None):
    sim, _, _ = RS.build(gym, kind, n, use_gpu_pipeline=False, other=other)
    m = sim.mg_model(sim.build_model())
    t = N.plan_layout(sim.mg_params(), m, tables=(N.MG_LAYOUT_SCALARS, N.MG_LAYOUT_FREE_FLAGS))
    head = t[N.MG_LAYOUT_SCALARS]
    assert head[3] == head[4] == 2 * n   # nf, nf1: every body a single-shape free body
    return t[N.MG_LAYOUT_FREE_FLAGS].tolist()


@pytest.mark.parametrize("kind,n", [("servo", 1), ("servo", 33), ("servo", 96), ("alternating", 33)])
def test_plain_boxes_set_the_flag(gym, kind, n):
    assert _flags(gym, kind, n) == [1]


def test_a_sphere_clears_the_flag(gym):
    assert _flags(gym, "ball", 33) == [0]


@pytest.mark.parametrize("xyz,rpy,want", [("0 0 0", "0 0 0", 1), ("0.1 0 0", "0 0 0", 0), ("0 0 0", "0 0 0.3", 0)])
def test_a_posed_box_clears_the_flag(gym, tmp_path, xyz, rpy, want):
    (tmp_path / "box.urdf").write_text(BOX % (xyz, rpy))
    assert _flags(gym, "other", 3, other=(str(tmp_path), "box.urdf")) == [want]


def test_abi_symbol():
    assert "mg_last_rigid_form" in N.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(N.LIB_PATH), "mg_last_rigid_form")
    assert N.lib.mg_last_rigid_form(None) == -1
