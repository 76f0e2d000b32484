"""mg_upload_model is plan, then commit: a refused upload
leaves the sim as it was, so the same sim takes a good model afterwards and
steps exactly as a fresh sim does; and mg_set_contact_reporting builds its
buffers apart, so toggling it (with another capacity) reproduces a fresh
reporting sim's list. Through _native directly, bit for bit."""
import ctypes

import numpy as np
import pytest

from test_isaacgym_amd import _native as N
import layout_scenes as LS

pytestmark = pytest.mark.gpu


def _create(p):
    s = N.lib.mg_create_sim(0, ctypes.byref(p))
    assert s, N.last_error()
    return s


def _states(s, m):
    out = []
    for fn, rows, cols in ((N.lib.mg_refresh_actor_root_state, m.num_actors, N.MG_STATE_N),
                           (N.lib.mg_refresh_rigid_body_state, m.num_bodies, N.MG_STATE_N),
                           (N.lib.mg_refresh_dof_state, m.num_dofs, 2)):
        a = np.zeros((rows, cols), np.float32)
        N.check(fn(s, a.ctypes.data, 1, None), "refresh")
        out.append(a)
    return out


def _step(s, frames=3):
    for _ in range(frames):
        N.check(N.lib.mg_simulate(s, None), "mg_simulate")
        N.check(N.lib.mg_fetch_results(s, 1), "mg_fetch_results")


def _contacts(s):
    buf = np.zeros(4096, N.RIGID_CONTACT_DTYPE)
    total = ctypes.c_int32(-1)
    n = N.lib.mg_refresh_rigid_contacts(s, buf.ctypes.data, len(buf), 1, ctypes.byref(total), None)
    assert 0 < n == total.value, (n, total.value, N.last_error())
    return buf[:n]


def test_refused_upload_then_good_model_steps_like_a_fresh_sim(gym, tmp_path):
    _, pb, bad = LS.REFUSALS["pile_too_many"](gym, tmp_path)
    _, p, good = LS.chains_and_boxes(gym, tmp_path)
    s, fresh = _create(p), _create(p)
    try:
        assert N.lib.mg_upload_model(s, ctypes.byref(bad)) == -4
        assert N.last_error() == "env 0: 65 free / 0 static bodies in contact range; a pile env supports 64 / 4"
        assert N.lib.mg_num_free_bodies(s) == 0 and N.lib.mg_simulate(s, None) == -3     # nothing of it stayed
        for sim in (s, fresh):
            N.check(N.lib.mg_upload_model(sim, ctypes.byref(good)), "mg_upload_model")
            assert N.lib.mg_num_coupled_envs(sim) == 4
            _step(sim)
        for a, b in zip(_states(s, good), _states(fresh, good)):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
        # reporting on -> off -> on with another capacity, against a sim that
        # turned it on once (both step the same builds in the same frames)
        N.check(N.lib.mg_set_contact_reporting(s, 1, 7), "mg_set_contact_reporting")
        N.check(N.lib.mg_set_contact_reporting(fresh, 1, 4096), "mg_set_contact_reporting")
        _step(s, 1)
        _step(fresh, 1)
        N.check(N.lib.mg_set_contact_reporting(s, 0, 0), "mg_set_contact_reporting")
        assert N.lib.mg_contact_reporting(s) == 0
        N.check(N.lib.mg_set_contact_reporting(s, 1, 4096), "mg_set_contact_reporting")
        _step(s, 1)
        _step(fresh, 1)
        a, b = _contacts(s), _contacts(fresh)
        assert len(a) > 7 and a.tobytes() == b.tobytes()
    finally:
        N.lib.mg_destroy_sim(s)
        N.lib.mg_destroy_sim(fresh)
