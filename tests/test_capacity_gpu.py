"""The contact capacity report on the device: scenes that
reach each fixed capacity of the step kernels (tests/capacity_scenes.py; what
the limits do to the physics: tests/test_capacity_api.py) must show up in
gym.get_contact_capacity_report with the exact counts, on the right envs, and
scenes within every capacity must leave it at zero. The counted steps stay
bit for bit the oracle's: counting changes no result."""
import ctypes

import numpy as np
import pytest
import torch

from isaacgym import gymtorch
from test_isaacgym_amd import _native as N, scenes
import oracle
import capacity_scenes as CS

pytestmark = pytest.mark.gpu

SUB = 2     # pile_scenes.sim_params: substeps


def _step(gym, sim, frames=1):
    for _ in range(frames):
        gym.simulate(sim)
        gym.fetch_results(sim, True)


def _counters(rep):
    return {k: rep[k] for k in N.CAPACITY_COUNTERS}


def _zero(rep):
    return rep["envs"] == {} and not any(_counters(rep).values())


class _Parity:
    """The sim's rigid-body tensor against the oracle stepped beside it."""

    def __init__(self, gym, sim):
        self.gym, self.sim = gym, sim
        self.rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        self.p, self.m = sim.mg_params(), sim.mg_model()
        self.st = sim.model_arrays["body_state0"].copy()
        self.dof = np.zeros((0, 2), np.float32)
        self.frame = 0

    def step(self):
        _step(self.gym, self.sim)
        oracle.step(self.p, self.m, self.st, self.dof)
        self.gym.refresh_rigid_body_state_tensor(self.sim)
        got = self.rb.cpu().numpy()
        if not np.array_equal(got, self.st):
            bad = np.argwhere(got != self.st)
            pytest.fail("frame %d: first differing body/field %s, max |diff| %g"
                        % (self.frame, bad[:3].tolist(), np.abs(got - self.st).max()))
        self.frame += 1


def _layers(gym):
    sim = CS.new_sim(gym, True)
    CS.add_sphere_layer(gym, sim, 0, 8)
    CS.add_sphere_layer(gym, sim, 1, 6)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_pile_envs(sim.native) == 2 and N.lib.mg_capacity_tracked(sim.native) == 1
    return sim


def test_pile_pair_cap_gpu(gym):
    sim = _layers(gym)
    par = _Parity(gym, sim)
    par.step()
    rep = gym.get_contact_capacity_report(sim)
    assert rep["PILE_OVERFLOW"] == SUB and rep["PILE_OVER_PAIRS"] == SUB and rep["PILE_OVER_POINTS"] == 0, rep
    assert rep["envs"] == {0: ["PILE_PAIRS"]}, rep
    assert sum(_counters(rep).values()) == 2 * SUB, rep
    assert gym.get_contact_capacity_report(sim, reset=True) == rep          # the read, then the reset
    assert _zero(gym.get_contact_capacity_report(sim))
    for _ in range(9):
        par.step()
    rep = gym.get_contact_capacity_report(sim)
    assert rep["PILE_OVERFLOW"] == 9 * SUB and rep["envs"] == {0: ["PILE_PAIRS"]}, rep
    gym.destroy_sim(sim)


def test_pile_point_cap_gpu(gym):
    sim = CS.new_sim(gym, True, npos=4, contact_offset=0.02)
    CS.add_cube_block(gym, sim, 0, 4)
    CS.add_cube_block(gym, sim, 1, 4)
    CS.add_cube_block(gym, sim, 2, 2)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_pile_envs(sim.native) == 3
    _step(gym, sim)
    rep = gym.get_contact_capacity_report(sim)
    assert rep["PILE_OVERFLOW"] == 2 * SUB and rep["PILE_OVER_POINTS"] == 2 * SUB, rep
    assert sorted(rep["envs"]) == [0, 1] and all("PILE_POINTS" in rep["envs"][e] for e in (0, 1)), rep
    gym.destroy_sim(sim)


def test_pile_colours_gpu(gym, capsys):
    """The tray owns 65 active pairs in env 0 and 64 in the controls: only env
    0 can run out of colours, by at most one pair a substep."""
    frames = 90
    sim = CS.new_sim(gym, True)
    CS.add_tray(gym, sim, 0, 63, True)
    CS.add_tray(gym, sim, 1, 63, False)
    CS.add_tray(gym, sim, 2, 62, True)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_pile_envs(sim.native) == 3
    par = _Parity(gym, sim)
    for _ in range(frames):
        par.step()
    rep = gym.get_contact_capacity_report(sim)
    with capsys.disabled():
        print("\ntray scene, %d frames: PILE_UNCOLOURED = %d" % (frames, rep["PILE_UNCOLOURED"]))
    assert 1 <= rep["PILE_UNCOLOURED"] <= frames * SUB, rep
    assert rep["PILE_UNVISITED"] == 0 and rep["PILE_OVERFLOW"] == 0, rep
    assert rep["envs"] == {0: ["PILE_COLOURS"]}, rep
    gym.destroy_sim(sim)


def test_coupled_contact_table_gpu(gym):
    sim = CS.new_sim(gym, True)
    for e in range(3):
        CS.add_walled_cubes(gym, sim, e, e + 1)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_coupled_envs(sim.native) == 3
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    first = [0, 4, 9]

    def counts():
        gym.refresh_rigid_body_state_tensor(sim)
        rows = rb.cpu().numpy()
        return [CS.walled_contacts(rows[first[e]:first[e] + 4 + e], e + 1) for e in range(3)]

    _step(gym, sim, 30)
    before = counts()
    gym.get_contact_capacity_report(sim, reset=True)
    frames = 10
    _step(gym, sim, frames)
    after = counts()
    assert before == after == [16, 20, 24], "the scene moved: contacts %s before, %s after the counted frames" % (
        before, after)
    rep = gym.get_contact_capacity_report(sim)
    assert rep["ENV_CONTACTS_DROPPED"] == frames * SUB * sum(max(0, c - 16) for c in after), rep
    assert rep["ENV_OVERFLOW"] == frames * SUB * 2, rep
    assert rep["ENV_ANCHORS_DROPPED"] == 0, rep
    assert rep["envs"] == {1: ["ENV_CONTACTS"], 2: ["ENV_CONTACTS"]}, rep
    gym.destroy_sim(sim)


def _slabs(gym, d):
    sim = CS.new_sim(gym, True)
    CS.add_slab(gym, sim, 0, d, CS.THREE_BOXES)
    CS.add_slab(gym, sim, 1, d, CS.TWO_BOXES)
    gym.prepare_sim(sim)
    assert N.lib.mg_num_free_bodies(sim.native) == 2 and N.lib.mg_capacity_tracked(sim.native) == 1
    _step(gym, sim, 30)
    gym.get_contact_capacity_report(sim, reset=True)
    return sim


def test_multi_shape_slots_gpu(gym, tmp_path):
    sim = _slabs(gym, str(tmp_path))
    frames = 10
    _step(gym, sim, frames)
    rep = gym.get_contact_capacity_report(sim)
    assert rep["RIGID_OVERFLOW"] == frames * SUB and rep["RIGID_CANDIDATES_DROPPED"] == frames * SUB * 4, rep
    assert rep["envs"] == {0: ["RIGID_SLOTS"]}, rep
    assert sum(_counters(rep).values()) == frames * SUB * 5, rep
    gym.destroy_sim(sim)


def test_quiet_scenes_report_nothing_gpu(gym):
    sim, _ = scenes.ball_pile_scene(gym, 4, use_gpu_pipeline=True)
    gym.prepare_sim(sim)
    assert N.lib.mg_capacity_tracked(sim.native) == 1
    _step(gym, sim, 60)
    assert _zero(gym.get_contact_capacity_report(sim))
    gym.destroy_sim(sim)
    sim, _ = scenes.servo_scene(gym, 8)
    gym.prepare_sim(sim)
    assert N.lib.mg_capacity_tracked(sim.native) == 0
    _step(gym, sim, 4)
    assert _zero(gym.get_contact_capacity_report(sim))
    gym.destroy_sim(sim)


def test_counters_advance_in_graph_replays_gpu(gym, tmp_path):
    sim = _slabs(gym, str(tmp_path))
    _step(gym, sim)
    eager = _counters(gym.get_contact_capacity_report(sim, reset=True))
    assert eager["RIGID_OVERFLOW"] == SUB and eager["RIGID_CANDIDATES_DROPPED"] == SUB * 4, eager
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    out = (ctypes.c_int64 * N.MG_CAP_N)()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gym.simulate(sim)
            rc = N.lib.mg_capacity_stats(sim.native, out, 0, sim.stream())
            code = N.lib.mg_last_error_code()
    torch.cuda.current_stream().wait_stream(side)
    assert rc == N.MG_ERR_STATE and code == N.MG_ERR_STATE
    torch.cuda.synchronize()
    assert _zero(gym.get_contact_capacity_report(sim))          # recorded, not run
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    rep = gym.get_contact_capacity_report(sim)
    assert _counters(rep) == {k: 5 * v for k, v in eager.items()}, rep
    assert rep["envs"] == {0: ["RIGID_SLOTS"]}, rep
    del g
    gym.destroy_sim(sim)


@pytest.mark.parametrize("check", ["default", "0"])
def test_automatic_warning_gpu(gym, capsys, monkeypatch, check):
    """fetch_results(sim, True) names the pile pair cap once in 8 frames (it
    looks at frames 1, 2, 4 and 8); MIGYM_CAPACITY_CHECK=0 at create_sim: never."""
    if check == "0":
        monkeypatch.setenv("MIGYM_CAPACITY_CHECK", "0")
    else:
        monkeypatch.delenv("MIGYM_CAPACITY_CHECK", raising=False)
    sim = _layers(gym)
    capsys.readouterr()
    _step(gym, sim, 8)
    err = capsys.readouterr().err
    lines = [ln for ln in err.splitlines() if "contact capacity exceeded" in ln]
    if check == "0":
        assert lines == []
    else:
        assert len(lines) == 1 and "pile env active-pair cap" in lines[0] and "(first env 0)" in lines[0], err
        assert lines[0].startswith("*** migym: contact capacity exceeded: ") and " in 1 envs " in lines[0], err
        assert lines[0].endswith("contacts were dropped; see gym.get_contact_capacity_report"), err
    assert gym.get_contact_capacity_report(sim)["PILE_OVERFLOW"] == 8 * SUB       # counted either way
    gym.destroy_sim(sim)
