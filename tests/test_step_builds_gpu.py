"""Which step kernel builds a simulate launches (mg_debug_step_builds, DESIGN.md
§2.2), at the smallest scene that reaches each (tests/step_builds_scenes.py).

The truth is not this library's own answer: tests/golden/step_builds.json holds,
per case, the step kernels of one frame in launch order as (kernel name, integer
template parameter, form word), read off a kernel trace of the engine as it was
before the choosers (its `provenance` says how). Every frame of every case must
report exactly those rows, and mg_last_rigid_form the public bits of the
k_rigid_step1 row (-1 without one). Wide and one-lane forms are pinned on the
host through CU and instance counts (tests/step_forms_check.cpp), not here."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_isaacgym_amd import _native as N

import step_builds_scenes as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_builds.json")
RF_WIDE, RF_REC, RF_BOX = 4, 16, 64     # csrc/mg_forms.h
CAP = 16


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def builds(sim):
    buf = (ctypes.c_int32 * (N.MG_STEP_BUILD_N * CAP))()
    n = N.lib.mg_debug_step_builds(sim.native, buf, CAP)
    assert 0 <= n <= CAP
    rows = np.frombuffer(buf, np.int32)[:n * N.MG_STEP_BUILD_N].reshape(n, N.MG_STEP_BUILD_N)
    return [[N.MG_KERNEL_NAMES[k], int(z), int(f)] for k, z, f in rows]


def public_form(rows):
    for name, _, f in rows:
        if name == "k_rigid_step1":
            return ((N.MG_RIGID_FORM_WIDE if f & RF_WIDE else 0) | (N.MG_RIGID_FORM_REC if f & RF_REC else 0) |
                    (N.MG_RIGID_FORM_BOX if f & RF_BOX else 0))
    return -1


def check_scene(gym, tmp_path, golden, scene):
    sim, phases = S.SCENES[scene](gym, tmp_path)
    seen = []

    def after_frame(case):
        got = builds(sim)
        print(case, got)
        assert got == golden[case], "%s: %s, the trace holds %s" % (case, got, golden[case])
        assert N.lib.mg_last_rigid_form(sim.native) == public_form(golden[case])
        seen.append(case)

    try:
        assert builds(sim) == [] and N.lib.mg_last_rigid_form(sim.native) == -1     # no simulate yet
        S.run(gym, sim, phases, after_frame)
        assert seen == [name for name, _, frames in phases for _ in range(frames)]
        return sim
    except BaseException:
        gym.destroy_sim(sim)
        raise


def test_route_scene_reports_the_parent_traces_kernels(gym, tmp_path, golden):
    assert golden["route"] == [["k_artic_chain_q", 4, 10], ["k_artic_lanes", 16, 3], ["k_artic_chain_q", 2, 10],
                               ["k_artic_lanes", 4, 6]]
    sim = check_scene(gym, tmp_path, golden, "route")
    try:
        # a short buffer gets the first rows and the full count; null needs cap 0
        two = (ctypes.c_int32 * (N.MG_STEP_BUILD_N * 2 + 1))(*([-7] * (N.MG_STEP_BUILD_N * 2 + 1)))
        assert N.lib.mg_debug_step_builds(sim.native, two, 2) == 4
        assert list(two) == [N.MG_KERNEL_NAMES.index("k_artic_chain_q"), 4, 10, N.MG_KERNEL_NAMES.index("k_artic_lanes"), 16, 3, -7]
        assert N.lib.mg_debug_step_builds(sim.native, None, 0) == 4
        assert N.lib.mg_debug_step_builds(sim.native, None, 1) < 0 and N.lib.mg_debug_step_builds(None, two, 2) < 0
    finally:
        gym.destroy_sim(sim)


def test_coupled_group_with_sensor_and_reporting(gym, tmp_path, golden):
    EF_FRC, EF_SENS, EF_CREP = 2, 4, 8
    assert [f for _, _, f in golden["coupled_sensor_reporting"]] == [EF_FRC | EF_SENS | EF_CREP]
    sim = check_scene(gym, tmp_path, golden, "coupled")
    gym.destroy_sim(sim)


def test_pile_reporting_off_and_on(gym, tmp_path, golden):
    assert golden["pile"] == [["k_pile_step", 0, 0]] and golden["pile_reporting"] == [["k_pile_step", 0, 1]]
    sim = check_scene(gym, tmp_path, golden, "pile")
    gym.destroy_sim(sim)


def test_two_free_boxes_reporting_off_and_on(gym, tmp_path, golden):
    RF_UPZ, RF_CREP = 1, 32
    assert golden["boxes"] == [["k_rigid_step1", 0, 83]]
    assert golden["boxes_reporting"] == [["k_rigid_step1", 0, RF_UPZ | RF_CREP]]
    sim = check_scene(gym, tmp_path, golden, "boxes")
    gym.destroy_sim(sim)
