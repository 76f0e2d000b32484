"""The step features' routing plan on the GPU at the smallest mixed
shape: owners of both kinds in different articulation groups of one sim, the case
the single split table makes new (tests/step_route_scene.py: 3 envs, an attractor
on env 1's gimbal, DOF friction on env 2's hinge chain, DOF forces on, 20 frames).

The truth is the engine as it was before the routing plan:
tests/golden/step_route_mixed.json holds its root, rigid-body, DOF-state and
DOF-force tensors after frames 1, 10 and 20 as bit patterns (its `provenance` says
how it was recorded). The run must reproduce them bit for bit, eager and with
its last 10 frames replayed from a captured graph; no tolerance applies."""
import json
import os

import numpy as np
import pytest

from test_isaacgym_amd import _native as N

import step_route_scene as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_route_mixed.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_bits(got, golden, what):
    for k in S.KEEP:
        for name in S.TENSORS:
            ref = np.array(golden["frames"][str(k)][name], dtype=np.int32)
            bits = got[k][name].reshape(-1)
            assert bits.shape == ref.shape, "%s frame %d %s: shape" % (what, k, name)
            bad = np.flatnonzero(bits != ref)
            assert bad.size == 0, "%s frame %d %s: %d of %d values differ, first at %d" % (
                what, k, name, bad.size, ref.size, bad[0])


def test_mixed_owners_eager_keeps_the_bits_and_refuses_the_unbuilt(gym, tmp_path, golden):
    sim, handles = S.build(gym, tmp_path)
    try:
        assert N.lib.mg_num_coupled_envs(sim.native) == 0
        assert sim.joint_friction_stats() == (1, 1, 0)
        got = S.run(gym, sim)
        check_bits(got, golden, "eager")
        # an attractor on the friction chain's own link: that group's friction build carries none
        S.add_attractor_on_friction_chain(gym, handles)
        with pytest.raises(N.MigymError) as e:
            gym.simulate(sim)
        assert golden["refusal"] in str(e.value)
        assert "is not built" in golden["refusal"]
    finally:
        gym.destroy_sim(sim)


def test_mixed_owners_replayed_from_a_graph_keeps_the_bits(gym, tmp_path, golden):
    sim, _ = S.build(gym, tmp_path)
    try:
        assert sim.joint_friction_stats() == (1, 1, 0)
        check_bits(S.run(gym, sim, graph_from=11), golden, "graph")
    finally:
        gym.destroy_sim(sim)
