"""Sleeping on the device: k_sleep_pass and the wake kernels
bit for bit against sleep_ref (oracle.step followed by the pass in numpy), the
frozen state of a sleeping island, the wakes of the set entries, off meaning off,
graph replay, and the DR ant's hips held within 2 degrees."""
import ctypes

import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
import oracle
import sleep_ref as SR

pytestmark = pytest.mark.gpu


class Dev:
    """A sim on the GPU pipeline with its state tensors."""

    def __init__(self, gym, sim, sleeping=True, **kw):
        self.gym, self.sim = gym, sim
        if sleeping:
            gym.set_sleeping(sim, True, **kw)
        gym.prepare_sim(sim)
        self.root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
        self.rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        self.dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))

    def step(self):
        self.gym.simulate(self.sim)
        self.gym.fetch_results(self.sim, True)

    def state(self):
        self.gym.refresh_rigid_body_state_tensor(self.sim)
        self.gym.refresh_dof_state_tensor(self.sim)
        return self.rb.cpu().numpy().copy(), self.dof.cpu().numpy().reshape(-1, 2).copy()

    def asleep(self):
        return self.gym.get_sleeping_actors(self.sim)

    def stats(self):
        return self.sim.sleep_stats()


def _same(dev, ref, what):
    rb, dof = dev.state()
    assert np.array_equal(rb, ref.st), "%s: rigid bodies, max |gpu - ref| %g" % (what, np.abs(rb - ref.st).max())
    assert np.array_equal(dof, ref.ds), "%s: DOF state" % what
    assert np.array_equal(dev.asleep(), ref.sleeping_actors()), "%s: sleeping actors" % what


PARITY = {
    "ant": (lambda gym: SR.ant_scene(gym, True, 1), 120, 1),
    "sphere_layer": (lambda gym: SR.sphere_layer_scene(gym, True, 2), 60, 1),
    "walled_cubes": (lambda gym: SR.walled_cubes_scene(gym, True, 2), 60, 1),
    "uncoupled": (lambda gym: SR.uncoupled_scene(gym, True, 2), 60, 2),
}


@pytest.mark.parametrize("name", sorted(PARITY))
def test_sleep_parity_gpu(gym, name):
    """Every frame: the rigid-body tensor, the DOF tensor and the sleeping actors
    equal the reference bit for bit, through landing, counting, falling asleep
    and staying asleep."""
    make, frames, launches = PARITY[name]
    dev = Dev(gym, make(gym))
    ref = SR.SleepRef(dev.sim)
    for f in range(1, frames + 1):
        dev.step()
        ref.step()
        _same(dev, ref, "%s frame %d" % (name, f))
    assert ref.asleep.all(), "%s: the scene is meant to be asleep after %d frames" % (name, frames)
    assert dev.stats() == (len(ref.isl), len(ref.isl), launches)
    gym.destroy_sim(dev.sim)


def test_sleeping_islands_are_frozen_gpu(gym):
    """Once an actor sleeps its rows are constant bit for bit and its velocities
    exactly 0, while the discarded step still reports the resting forces."""
    dev = Dev(gym, SR.uncoupled_scene(gym, True, 2))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(dev.sim))
    A = dev.sim.model_arrays
    bodies, adof = SR.actor_bodies(A), np.asarray(A["actor_dof"])
    prev, prev_asleep, frozen = None, None, 0
    for f in range(1, 61):
        dev.step()
        rb, dof = dev.state()
        asleep = dev.asleep()
        for a in np.nonzero(asleep)[0]:
            b, d = bodies[a], np.arange(adof[a], adof[a + 1])
            assert np.all(rb[b, 7:13] == 0.0) and np.all(dof[d, 1] == 0.0), "frame %d actor %d: velocities" % (f, a)
            if prev_asleep[a]:
                assert np.array_equal(rb[b], prev[0][b]) and np.array_equal(dof[d], prev[1][d]), "frame %d actor %d" % (f, a)
                frozen += 1
        prev, prev_asleep = (rb, dof), asleep
    assert asleep.all() and frozen >= 4 * 5
    gym.refresh_net_contact_force_tensor(dev.sim)
    box = bodies[0][0]
    assert abs(float(ncf[box, 2])) > 0.1     # the box's weight on the ground, still reported
    gym.destroy_sim(dev.sim)


def test_indexed_root_set_wakes_its_env_only_gpu(gym):
    dev = Dev(gym, SR.walled_cubes_scene(gym, True, 2))
    ref = SR.SleepRef(dev.sim)
    for _ in range(30):
        dev.step()
        ref.step()
    cubes = np.nonzero(ref.actor_island >= 0)[0]
    assert dev.asleep()[cubes].all() and ref.asleep.all()
    gym.refresh_actor_root_state_tensor(dev.sim)
    a = int(cubes[0])                     # cube A of env 0
    dev.root[a, 2] += 0.05
    idx = torch.tensor([a], dtype=torch.int32, device="cuda:0")
    assert gym.set_actor_root_state_tensor_indexed(dev.sim, gymtorch.unwrap_tensor(dev.root), gymtorch.unwrap_tensor(idx), 1)
    ref.set_root([a], dev.root[a].cpu().numpy()[None])
    want = ref.sleeping_actors()
    assert not want[cubes[:2]].any() and want[cubes[2:]].all()     # env 0 woke (both cubes: one island), env 1 sleeps
    assert np.array_equal(dev.asleep(), want)
    for f in range(3):
        dev.step()
        ref.step()
        _same(dev, ref, "after the root set, frame %d" % f)
    assert not dev.asleep()[cubes[:2]].any() and dev.asleep()[cubes[2:]].all()
    gym.destroy_sim(dev.sim)


def test_force_and_target_wakes_gpu(gym):
    """A non-zero force on one body wakes its island only; a full DOF target set
    wakes all; gym.wake_actors wakes by index."""
    dev = Dev(gym, SR.uncoupled_scene(gym, True, 2))
    ref = SR.SleepRef(dev.sim)
    for _ in range(60):
        dev.step()
        ref.step()
    assert dev.asleep().all() and ref.asleep.all()
    nb, nd = len(ref.st), len(ref.ds)
    # actors: box 0, gimbal 0, box 1, gimbal 1; a force on box 1
    ext = np.zeros((nb, 6), np.float32)
    ext[ref.roots[2], 0] = 0.5
    force = torch.from_numpy(ext[:, 0:3].copy()).to("cuda:0")
    assert gym.apply_rigid_body_force_tensors(dev.sim, gymtorch.unwrap_tensor(force), None, gymapi.ENV_SPACE)
    assert dev.asleep().tolist() == [True, True, False, True]
    dev.step()
    ref.step(ext=ext)
    _same(dev, ref, "after the force")
    assert dev.asleep().tolist() == [True, True, False, True]
    # wake by hand: gimbal 0
    gym.wake_actors(dev.sim, [1])
    ref.wake([1])
    assert dev.asleep().tolist() == [True, False, False, True]
    # a full DOF target set (the targets it already has) wakes everybody
    tg = torch.zeros(nd, dtype=torch.float32, device="cuda:0")
    assert gym.set_dof_position_target_tensor(dev.sim, gymtorch.unwrap_tensor(tg))
    assert not dev.asleep().any()
    dev.step()
    ref.step(tgt_set=True)
    _same(dev, ref, "after the target set")
    assert not dev.asleep().any()
    gym.destroy_sim(dev.sim)


def test_off_is_off_gpu(gym):
    """Without set_sleeping no pass runs; with a window nobody reaches the pass
    runs and changes nothing: both bit-exact to the plain oracle."""
    for window in (None, 1.0e6):
        dev = Dev(gym, SR.walled_cubes_scene(gym, True, 2), sleeping=window is not None,
                  **({} if window is None else {"window": window}))
        assert dev.stats() == ((0, 0, 0) if window is None else (2, 0, 1))
        assert N.lib.mg_step_out_supported(dev.sim.native) == 0   # a coupled scene either way
        A = dev.sim.model_arrays
        p, m = dev.sim.mg_params(), dev.sim.mg_model()
        st, ds = A["body_state0"].copy(), A["dof_state0"].copy()
        for f in range(30):
            dev.step()
            oracle.step(p, m, st, ds)
        rb, _ = dev.state()
        assert np.array_equal(rb, st), "window %r: max |gpu - oracle| %g" % (window, np.abs(rb - st).max())
        assert not dev.asleep().any()
        assert dev.stats() == ((0, 0, 0) if window is None else (2, 0, 1))
        gym.destroy_sim(dev.sim)


def test_sleeping_turned_on_after_upload_and_off_again_gpu(gym):
    dev = Dev(gym, SR.sphere_layer_scene(gym, True, 2), sleeping=False)
    ref = SR.SleepRef(dev.sim, on=False)
    for _ in range(3):
        dev.step()
        ref.step()
    gym.set_sleeping(dev.sim, True)       # timers at 0, anchors at the next pass
    ref.on = True
    for f in range(30):
        dev.step()
        ref.step()
        _same(dev, ref, "frame %d" % f)
    assert dev.asleep().all() and dev.stats() == (2, 2, 1)
    gym.set_sleeping(dev.sim, False)
    assert not dev.asleep().any() and dev.stats() == (0, 0, 0)
    gym.destroy_sim(dev.sim)


def test_graph_replay_equals_eager_gpu(gym):
    """The pass is captured with the step: 1 eager frame and 39 replays of a
    captured simulate equal 40 eager frames, asleep at the end; after the capture
    set_sleeping is refused."""
    eager = Dev(gym, SR.walled_cubes_scene(gym, True, 2))
    for _ in range(40):
        eager.step()
    want_rb, want_dof = eager.state()
    want_asleep = eager.asleep()
    assert want_asleep[np.nonzero(SR.SleepRef(eager.sim).actor_island >= 0)[0]].all()
    gym.destroy_sim(eager.sim)

    dev = Dev(gym, SR.walled_cubes_scene(gym, True, 2))
    dev.step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gym.simulate(dev.sim)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert N.lib.mg_set_sleeping(dev.sim.native, 5e-5, 0.4) == N.MG_ERR_STATE
    for _ in range(39):
        g.replay()
    torch.cuda.synchronize()
    rb, dof = dev.state()
    assert np.array_equal(rb, want_rb) and np.array_equal(dof, want_dof)
    assert np.array_equal(dev.asleep(), want_asleep)
    del g
    gym.destroy_sim(dev.sim)


def test_ant_hips_stay_within_two_degrees_gpu(gym):
    """VERDICT's figure on the device: asleep by frame 70, hips within 2 degrees
    at frame 400 (11.6 without sleeping)."""
    dev = Dev(gym, SR.ant_scene(gym, True, 1))
    for _ in range(70):
        dev.step()
    assert dev.asleep().all()
    _, dof70 = dev.state()
    for _ in range(70, 400):
        dev.step()
    _, dof = dev.state()
    hips = np.degrees(dof[0::2, 0])
    print("hips at frame 400 (deg):", hips)
    assert np.array_equal(dof, dof70)
    assert np.abs(hips).max() <= 2.0, hips
    gym.destroy_sim(dev.sim)
