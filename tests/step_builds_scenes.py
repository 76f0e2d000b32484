"""The scenes of tests/test_step_builds_gpu.py, each the smallest that reaches its
step kernel builds, shared with the script that recorded the kernel traces behind
tests/golden/step_builds.json. A scene is build(gym, tmp_path) -> prepared sim and
a list of phases; a phase is (case name, contact reporting on or off, frames).

  route     tests/step_route_scene.py: 3 uncoupled envs, gimbal and hinge chain, an
            attractor owner, a friction owner, DOF forces on
  coupled   two envs of tests/test_contact_list_gpu.py's coupled scene (gimbal, static
            box, two free boxes), a force sensor on the gimbal's second link
  pile      tests/pile_scenes.py's heap, one env of three bodies on the fixed box
  boxes     tests/rigid_box_scenes.py's servo pair, one env: two free boxes"""
from isaacgym import gymapi

import pile_scenes as PS
import rigid_box_scenes as RS
import step_route_scene as SR

FRAMES = 2


def _route(gym, tmp_path):
    sim, _ = SR.build(gym, tmp_path)
    return sim, [("route", False, FRAMES)]


def _coupled(gym, tmp_path):
    import test_contact_list_gpu as CL
    sim = CL._sim(gym)
    assets = CL._coupled_assets(gym, sim)
    assert gym.create_asset_force_sensor(assets[0], 1, gymapi.Transform()) == 0
    for i in range(2):
        CL._add_coupled(gym, sim, assets, i)
    gym.set_rigid_contact_reporting(sim, True)
    gym.prepare_sim(sim)
    return sim, [("coupled_sensor_reporting", True, FRAMES)]


def _pile(gym, tmp_path):
    sim, _ = PS.mixed_pile_scene(gym, 1, True, counts=[3])
    gym.prepare_sim(sim)
    return sim, [("pile", False, FRAMES), ("pile_reporting", True, FRAMES)]


def _boxes(gym, tmp_path):
    sim, _, _ = RS.build(gym, "servo", 1)
    gym.prepare_sim(sim)
    return sim, [("boxes", False, FRAMES), ("boxes_reporting", True, FRAMES)]


SCENES = {"route": _route, "coupled": _coupled, "pile": _pile, "boxes": _boxes}


def run(gym, sim, phases, after_frame=None):
    """Steps the phases; after_frame(case name) is called after every frame."""
    for name, reporting, frames in phases:
        if gym.get_rigid_contact_reporting(sim) != reporting:
            gym.set_rigid_contact_reporting(sim, reporting)
        for _ in range(frames):
            gym.simulate(sim)
            gym.fetch_results(sim, True)
            if after_frame:
                after_frame(name)
