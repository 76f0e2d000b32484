"""The contact capacity report's interface (include/migym.h)
without a device, and the oracle findings its scenes rest on
(tests/capacity_scenes.py): what each capacity limit of the step kernels does
to the physics when it is reached — the oracle restates the limits, so these
also keep the scenes valid as inputs of tests/test_capacity_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_isaacgym_amd import _native as N
import capacity_scenes as CS

NAMES = ("mg_capacity_stats", "mg_capacity_env_flags", "mg_capacity_tracked")


def test_symbols_in_header_and_binding():
    src = open(os.path.join(ROOT, "include", "migym.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in N.EXPORTED_SYMBOLS and hasattr(N.lib, name)
    # the counter and flag names of the binding are the header's, in its order
    cap = re.findall(r"#define MG_CAP_([A-Z_]+)\s+(\d+)", code)
    assert [n for n, _ in cap] == list(N.CAPACITY_COUNTERS) + ["N"]
    assert [int(v) for _, v in cap] == list(range(N.MG_CAP_N)) + [N.MG_CAP_N]
    capf = re.findall(r"#define MG_CAPF_([A-Z_]+)\s+(\d+)", code)
    assert [n for n, _ in capf] == list(N.CAPACITY_FLAGS)
    assert [int(v) for _, v in capf] == [1 << b for b in range(len(N.CAPACITY_FLAGS))]


def test_null_sim_is_refused():
    out = (ctypes.c_int64 * N.MG_CAP_N)()
    flags = (ctypes.c_int32 * 4)()
    assert N.lib.mg_capacity_stats(None, out, 0, None) == N.MG_ERR_ARG
    assert N.lib.mg_last_error_code() == N.MG_ERR_ARG
    assert N.lib.mg_capacity_env_flags(None, flags, 4, None) == N.MG_ERR_ARG
    assert N.lib.mg_capacity_tracked(None) == 0


def test_report_needs_a_device(gym):
    sim = CS.new_sim(gym, False)
    CS.add_sphere_layer(gym, sim, 0, 2)
    if N.device_count() > 0:     # served: nothing has stepped yet
        rep = gym.get_contact_capacity_report(sim)
        assert rep["envs"] == {} and all(rep[k] == 0 for k in N.CAPACITY_COUNTERS)
        gym.destroy_sim(sim)
        return
    with pytest.raises(N.MigymError):
        gym.get_contact_capacity_report(sim)
    assert gym.fetch_results(sim, True)      # the automatic check is silent without a device


def test_sphere_layer_past_the_pair_cap_sinks(gym):
    """176 active pairs against 128: the pairs past the cap are dropped every
    substep — the last ground pairs among them — and spheres 48..63 fall
    through the ground; 96 pairs (6 x 6) rest."""
    sim = CS.new_sim(gym, False)
    CS.add_sphere_layer(gym, sim, 0, 8)
    CS.add_sphere_layer(gym, sim, 1, 6)
    st, _ = CS.oracle_run(sim, 60)
    z8, z6 = st[:64, 2], st[64:, 2]
    assert np.all(z8[48:] < -4.0), z8[48:]
    assert np.all(np.abs(z8[:48] - 0.05) < 0.002), z8[:48]
    assert np.all(np.abs(z6 - 0.05) < 0.002), z6


def test_tray_sphere_past_the_colours_sinks(gym):
    """The tray's 65th active pair finds no colour and is never solved: the
    last sphere sinks into the tray (z 0.040 +- 0.002, its rest on the ground
    inside it); with 64 pairs — no fixed box, or 62 spheres — all rest on the
    tray at 0.140 +- 0.002."""
    sim = CS.new_sim(gym, False)
    CS.add_tray(gym, sim, 0, 63, True)
    CS.add_tray(gym, sim, 1, 63, False)
    CS.add_tray(gym, sim, 2, 62, True)
    st, _ = CS.oracle_run(sim, 90)
    a = st[2:65, 2]                 # env 0: tray, fixed box, 63 spheres
    b = st[66:129, 2]               # env 1: tray, 63 spheres
    c = st[131:193, 2]              # env 2: tray, fixed box, 62 spheres
    assert abs(a[-1] - 0.040) < 0.002, a[-1]
    assert np.all(np.abs(a[:-1] - 0.140) < 0.002), a
    assert np.all(np.abs(b - 0.140) < 0.002), b
    assert np.all(np.abs(c - 0.140) < 0.002), c


def test_walled_cubes_contact_counts(gym):
    """oracle.collide on the coupled scene as placed: 16 / 20 / 24 contacts with
    one, two and three walls (4 per touching pair, none between the cubes or
    with the far wall) against the table of 16."""
    for nwalls, want in ((1, 16), (2, 20), (3, 24)):
        sim = CS.new_sim(gym, False)
        CS.add_walled_cubes(gym, sim, 0, nwalls)
        rows = sim.build_model()["body_state0"]
        assert CS.walled_contacts(rows, nwalls) == want


def test_third_box_of_a_slab_never_touches(gym, tmp_path):
    """Three collision boxes have 12 ground candidates against 8 slots: the
    third box's corners are never contacts, and the body comes to the two-box
    body's state bit for bit (each alone in env 0 of its sim), at rest on the
    boxes' half height with its weight as the net contact force."""
    res = []
    for xs in (CS.THREE_BOXES, CS.TWO_BOXES):
        sim = CS.new_sim(gym, False)
        CS.add_slab(gym, sim, 0, str(tmp_path), xs)
        res.append(CS.oracle_run(sim, 60))
    (st3, cf3), (st2, cf2) = res
    assert np.array_equal(st3, st2)
    assert np.array_equal(cf3, cf2)
    assert abs(st3[0, 2] - 0.05) < 1e-4, st3[0, 2]
    assert abs(cf3[0, 2] - 9.8) < 0.01, cf3[0]
