"""Sleeping on the host: the layout plan's islands against
islands derived in Python from actors, kinds and collision groups; when the rule
fires on the CPU oracle (sleep_ref) and what it holds; the Python API's
argument checks and MIGYM_SLEEP. The device's pass is tests/test_sleep_gpu.py."""
import math

import numpy as np
import pytest

from test_isaacgym_amd import _native as N, _sim, scenes
import sleep_ref as SR

TABLES = (N.MG_LAYOUT_PERM, N.MG_LAYOUT_BODY_ISLAND, N.MG_LAYOUT_ACTOR_ISLAND, N.MG_LAYOUT_ISLAND_BODY0,
          N.MG_LAYOUT_ISLAND_BODY, N.MG_LAYOUT_ISLAND_DOF0, N.MG_LAYOUT_ISLAND_DOF, N.MG_LAYOUT_ISLAND_CLASS,
          N.MG_LAYOUT_BODY_K)


def _servo(gym, gpu):
    return scenes.servo_scene(gym, 3, use_gpu_pipeline=gpu)[0]


SCENES = {
    "servo": _servo,
    "walled_cubes": lambda gym, gpu: SR.walled_cubes_scene(gym, gpu, 2),
    "sphere_layer": lambda gym, gpu: SR.sphere_layer_scene(gym, gpu, 2),
    "ant": lambda gym, gpu: SR.ant_scene(gym, gpu, 2),
    "uncoupled": lambda gym, gpu: SR.uncoupled_scene(gym, gpu, 2),
}
# islands per scene: (islands, bodies of each)
EXPECT = {"servo": (6, 1), "walled_cubes": (2, 2), "sphere_layer": (2, 9), "ant": (2, 9), "uncoupled": (4, None)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_layout_islands_match_python(gym, name):
    sim = SCENES[name](gym, False)
    A = sim.build_model()
    T = N.plan_layout(sim.mg_params(), sim.mg_model(), tables=TABLES)
    perm = T[N.MG_LAYOUT_PERM]
    nb, nd = len(A["body_kind"]), len(A["dof_state0"])
    ref = SR.SleepRef(sim)
    assert len(ref.isl) == EXPECT[name][0]
    if EXPECT[name][1]:
        assert all(len(b) == EXPECT[name][1] for b in ref.isl_bodies)
    # the same partition of the bodies, the DOFs and the actors: an island is named by its smallest body
    body0, body = T[N.MG_LAYOUT_ISLAND_BODY0], T[N.MG_LAYOUT_ISLAND_BODY]
    dof0, dof = T[N.MG_LAYOUT_ISLAND_DOF0], T[N.MG_LAYOUT_ISLAND_DOF]
    ni = int(T[N.MG_LAYOUT_ISLAND_CLASS][0])
    assert ni == len(ref.isl) and len(body0) == ni + 1 and len(dof0) == ni + 1
    inv = np.argsort(perm)            # storage slot -> global body
    name_c = [int(inv[body[body0[i]:body0[i + 1]]].min()) for i in range(ni)]
    name_py = [int(b.min()) for b in ref.isl_bodies]
    got_body = np.array([name_c[i] if i >= 0 else -1 for i in T[N.MG_LAYOUT_BODY_ISLAND][perm]])
    want_body = np.array([name_py[i] if i >= 0 else -1 for i in ref.body_island])
    assert np.array_equal(got_body, want_body)
    got_actor = [name_c[i] if i >= 0 else -1 for i in T[N.MG_LAYOUT_ACTOR_ISLAND]]
    assert got_actor == [name_py[i] if i >= 0 else -1 for i in ref.actor_island]
    for i in range(ni):
        j = name_py.index(name_c[i])
        assert sorted(inv[body[body0[i]:body0[i + 1]]].tolist()) == sorted(ref.isl_bodies[j].tolist())
        assert dof[dof0[i]:dof0[i + 1]].tolist() == sorted(ref.isl_dofs[j].tolist())
        assert np.all(np.diff(body[body0[i]:body0[i + 1]]) > 0)
    assert body0[-1] == (ref.body_island >= 0).sum() and dof0[-1] == nd and len(perm) == nb
    # the order: size classes 1 / 2..16 / more, each in the order of its islands' first storage slot
    size = np.diff(body0)
    cls = np.where(size == 1, 0, np.where(size <= 16, 1, 2))
    c1, c2 = int(T[N.MG_LAYOUT_ISLAND_CLASS][1]), int(T[N.MG_LAYOUT_ISLAND_CLASS][2])
    assert np.all(cls[:c1] == 0) and np.all(cls[c1:c2] == 1) and np.all(cls[c2:] == 2)
    for lo, hi in ((0, c1), (c1, c2), (c2, ni)):
        assert np.all(np.diff(body[body0[lo:hi]]) > 0)
    # the radii: k_b bit for bit
    assert np.array_equal(T[N.MG_LAYOUT_BODY_K][perm], ref.k)
    assert np.all(ref.k[ref.body_island >= 0] > 0)
    gym.destroy_sim(sim)


def test_single_body_islands_are_their_slots(gym):
    """The free-body kernel's bodies: island i is storage slot i."""
    sim = _servo(gym, False)
    sim.build_model()
    T = N.plan_layout(sim.mg_params(), sim.mg_model(), tables=TABLES)
    assert T[N.MG_LAYOUT_BODY_ISLAND].tolist() == list(range(6))
    assert T[N.MG_LAYOUT_ISLAND_BODY].tolist() == list(range(6))
    gym.destroy_sim(sim)


def test_host_figures():
    """W and tol of the defaults at dt = 1/60: 24 frames, 4 mm."""
    class P:
        dt = 1.0 / 60.0
    W = max(1, int(math.floor(float(np.float32(0.4)) / float(np.float32(P.dt)) + 0.5)))
    assert W == 24
    assert abs(0.4 * math.sqrt(2 * 5e-5) - 0.004) < 1e-12


def _run(ref, frames):
    """Steps `ref`; returns per island the frame it fell asleep (0: never) and the
    largest distance of a body from its anchor while the timer ran."""
    at = np.zeros(len(ref.isl), int)
    far = np.zeros(len(ref.isl))
    for f in range(1, frames + 1):
        was = ref.asleep.copy()
        ref.step()
        for i, b in enumerate(ref.isl_bodies):
            if ref.asleep[i] and not was[i]:
                at[i] = f
            if not ref.asleep[i] and ref.timer[i] > 0:
                far[i] = max(far[i], np.linalg.norm((ref.st[b, 0:3] - ref.anchor[b, 0:3]).astype(np.float64), axis=1).max())
    return at, far


@pytest.mark.parametrize("name,frames,by", [("sphere_layer", 60, 40), ("walled_cubes", 60, 40)])
def test_reference_resting_scenes_fall_asleep(gym, name, frames, by):
    """The pile and the coupled cubes rest from the first frame: both fall asleep
    within a few frames of the window's 24, moving far less than the 4 mm
    tolerance meanwhile, and from then on their rows are constant bit for bit."""
    sim = SCENES[name](gym, False)
    ref = SR.SleepRef(sim)
    at, far = _run(ref, frames)
    print(name, "asleep at", at, "largest movement while counting", far)
    assert np.all(at > 0) and np.all(at <= by), at
    assert np.all(far <= 0.004 * (1 + 1e-6)), far   # the rule itself: counting means within tol
    st, ds = ref.st.copy(), ref.ds.copy()
    mov = ref.body_island >= 0
    assert np.all(st[mov, 7:13] == 0.0)
    for _ in range(5):
        ref.step()
        assert np.array_equal(ref.st, st) and np.array_equal(ref.ds, ds)
    # the resting forces are still reported: the discarded step's
    assert np.abs(ref.cforce[mov]).max() > 0.0
    gym.destroy_sim(sim)


def test_reference_ant_sleeps_before_it_twists(gym):
    """The DR ant lands, rests and is asleep by frame 70, before the twist of its
    unstable rest pose starts (near frame 90 without sleeping), so the hips stay
    within 2 degrees at frame 400 (11.6 without sleeping: tests/test_dr_fixture.py)."""
    sim = SR.ant_scene(gym, False, 1)
    ref = SR.SleepRef(sim)
    at, far = _run(ref, 70)
    print("ant asleep at", at, "largest movement while counting", far)
    assert ref.asleep.all() and 0 < at[0] <= 70, at
    hips70 = np.degrees(ref.ds[0::2, 0]).copy()
    for _ in range(70, 400):
        ref.step()
    hips = np.degrees(ref.ds[0::2, 0])
    print("hips at 70 / 400 (deg):", hips70, hips)
    assert ref.asleep.all()
    assert np.array_equal(hips, hips70)
    assert np.abs(hips).max() <= 2.0, hips
    gym.destroy_sim(sim)


def test_reference_wakes(gym):
    """An indexed root set wakes its actor's island only; a force one body's island."""
    sim = SR.walled_cubes_scene(gym, False, 2)
    ref = SR.SleepRef(sim)
    _run(ref, 40)
    assert ref.asleep.all()
    cube = [a for a in range(len(ref.roots)) if ref.actor_island[a] == 0][0]
    row = ref.st[ref.roots[cube]].copy()
    row[2] += 0.05
    ref.set_root([cube], row[None])
    ref.step()
    assert not ref.asleep[0] and ref.asleep[1]
    ext = np.zeros((len(ref.st), 6), np.float32)
    ext[ref.isl_bodies[1][0], 2] = 1.0
    ref.step(ext=ext)
    assert not ref.asleep.any()
    gym.destroy_sim(sim)


# ---------------------------------------------------------------- the Python API
@pytest.mark.parametrize("text,want", [(None, None), ("", None), ("0", None), ("1", _sim.SLEEP_DEFAULTS),
                                       ("1e-4,0.5", (1e-4, 0.5)), (" 2e-5 , 1 ", (2e-5, 1.0))])
def test_migym_sleep_forms(text, want):
    assert _sim.parse_sleep_env(text) == want


@pytest.mark.parametrize("text", ["yes", "2", "1,2,3", "0.1", "a,b", "-1,0.4", "5e-5,0", "nan,0.4", "5e-5,inf"])
def test_migym_sleep_refuses(text):
    with pytest.raises(ValueError):
        _sim.parse_sleep_env(text)


def test_migym_sleep_read_at_create_sim(gym, monkeypatch):
    monkeypatch.setenv("MIGYM_SLEEP", "1")
    sim = _servo(gym, False)
    assert gym.get_sleeping(sim) == _sim.SLEEP_DEFAULTS
    gym.destroy_sim(sim)
    monkeypatch.setenv("MIGYM_SLEEP", "1e-4,0.25")
    sim = _servo(gym, False)
    assert gym.get_sleeping(sim) == (1e-4, 0.25)
    gym.destroy_sim(sim)
    monkeypatch.delenv("MIGYM_SLEEP")
    sim = _servo(gym, False)
    assert gym.get_sleeping(sim) is None
    gym.destroy_sim(sim)
    monkeypatch.setenv("MIGYM_SLEEP", "on")
    with pytest.raises(ValueError):
        _servo(gym, False)


def test_set_sleeping_checks_its_arguments(gym):
    sim = _servo(gym, False)
    assert gym.get_sleeping(sim) is None            # off by default
    assert gym.set_sleeping(sim)
    assert gym.get_sleeping(sim) == (5e-5, 0.4)
    for bad in ((0.0, 0.4), (-1e-5, 0.4), (5e-5, 0.0), (5e-5, -1.0), (float("nan"), 0.4), (5e-5, float("inf")),
                (1e-60, 0.4), ("x", 0.4)):
        with pytest.raises(ValueError):
            gym.set_sleeping(sim, True, *bad)
        assert gym.get_sleeping(sim) == (5e-5, 0.4)  # a refused call changes nothing
    gym.set_sleeping(sim, True, threshold=1e-4, window=1.0)
    assert gym.get_sleeping(sim) == (1e-4, 1.0)
    gym.set_sleeping(sim, False, threshold=-1.0)    # off: the figures are not looked at
    assert gym.get_sleeping(sim) is None
    # nobody sleeps while it is off; indices are checked either way
    assert gym.get_sleeping_actors(sim).tolist() == [False] * 6
    assert gym.wake_actors(sim) and gym.wake_actors(sim, [0, 5])
    for bad in ([6], [-1], [0.5]):
        with pytest.raises(ValueError):
            gym.wake_actors(sim, bad)
    gym.destroy_sim(sim)


def test_entries_declared_and_bound():
    import ctypes
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("mg_set_sleeping", "mg_wake", "mg_sleep_state", "mg_sleep_stats"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    # without a sim every entry refuses with a message
    out = (ctypes.c_int32 * 3)()
    assert N.lib.mg_set_sleeping(None, 5e-5, 0.4) == N.MG_ERR_ARG
    assert N.lib.mg_wake(None, None, 0, 1, None) == N.MG_ERR_STATE
    assert N.lib.mg_sleep_state(None, None, 1, None) == N.MG_ERR_STATE
    assert N.lib.mg_sleep_stats(None, out) == N.MG_ERR_ARG
