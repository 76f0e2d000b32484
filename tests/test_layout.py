"""The host-only layout planner (csrc/mg_layout.cpp) through
mg_debug_plan_layout, with no device: every table of every case of
tests/layout_scenes.py equals tests/golden/layout_fixture.json, which was
recorded from the code before the planner existed (its "provenance" field says
how), and each case's point is asserted by name as well. The refusals' codes
and full messages are the fixture's too; the messages also stand in this file,
copied from that older source.

The issue's wide case — the narrow env with 3 free boxes, 19 velocity slots —
is no coupled env: the coupled step takes at most MG_ENV_MAXF = 2 free bodies,
so the model is refused (REFUSALS: coupled_three_boxes, checked like the
others). The 64-lane group is reached with a 5-hinge chain and 2 boxes (17
slots) instead."""
import ctypes
import json
import os

import numpy as np
import pytest

from test_isaacgym_amd import _native as N
import layout_scenes as LS

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "layout_fixture.json")))
H, GN, EN = N.MG_LAYOUT_HEAD_N, N.MG_LAYOUT_GROUP_N, N.MG_LAYOUT_ENVGROUP_N
HEAD = ("nb", "na", "nd", "nf", "nf1", "nf_rigid", "n_coupled", "n_pile", "max_actor_dofs", "roots_free",
        "step_out_ok", "groups", "env_groups")
GROUP = ("chain", "aff", "aff_b0", "aff_d0", "aff_ds", "out_aff", "out_g0", "out_r0", "offset", "count",
         "step_offset", "step_count", "uni_mass", "nl")
ENVGROUP = ("tmpl", "wide", "max_free", "offset", "count")


def _plan(gym, tmp_path, name):
    sim, p, m = LS.CASES[name](gym, tmp_path)
    return N.plan_layout(p, m)


def _scalars(t):
    s = t[N.MG_LAYOUT_SCALARS]
    head = dict(zip(HEAD, s[:H]))
    groups = [dict(zip(GROUP, s[H + GN * i:])) for i in range(head["groups"])]
    e0 = H + GN * head["groups"]
    envs = [dict(zip(ENVGROUP, s[e0 + EN * i:])) for i in range(head["env_groups"])]
    assert len(s) == e0 + EN * head["env_groups"]
    return head, groups, envs


@pytest.mark.parametrize("name", sorted(LS.CASES))
def test_tables_equal_the_recorded_ones(gym, tmp_path, name):
    t = _plan(gym, tmp_path, name)
    want = FIX["cases"][name]
    assert sorted(want) == sorted(str(k) for k in t)
    for k, got in t.items():
        assert got.tolist() == want[str(k)], "table %d" % k


def test_free_body_order(gym, tmp_path):
    t = _plan(gym, tmp_path, "free_order")
    head, _, _ = _scalars(t)
    # bodies: lo, hi, two, lo, hi. The template that starts higher comes first,
    # single-shape bodies before the two-shape one
    assert t[N.MG_LAYOUT_PERM].tolist() == [2, 0, 4, 3, 1]
    assert (head["nf"], head["nf1"], head["nf_rigid"]) == (5, 4, 5)
    assert head["roots_free"] == 0 and head["step_out_ok"] == 0
    head1, _, _ = _scalars(_plan(gym, tmp_path, "free_order_single"))
    assert (head1["nf"], head1["nf1"], head1["nf_rigid"], head1["roots_free"]) == (4, 4, 4, 1)


def test_blocked_chains(gym, tmp_path):
    t = _plan(gym, tmp_path, "chains65")
    head, (g,), envs = _scalars(t)
    assert not envs and head["step_out_ok"] == 1 and head["max_actor_dofs"] == 1
    assert (g["chain"], g["aff"], g["out_aff"], g["uni_mass"], g["nl"], g["count"], g["step_count"]) == (1, 1, 1, 1, 2, 65, 65)
    rows = t[N.MG_LAYOUT_ARTIC_STEP].reshape(65, N.MG_ARTIC_I_N)
    assert rows[:, 3].tolist() == [64] * 64 + [1]                  # the link stride: a full block, a tail of 1
    assert np.array_equal(t[N.MG_LAYOUT_ARTIC_SORTED], t[N.MG_LAYOUT_ARTIC_STEP])
    # link-major storage: global body 2 a + l of the block's instance j sits at base + l * count + j
    perm = t[N.MG_LAYOUT_PERM].reshape(65, 2)
    assert perm[:64, 0].tolist() == list(range(0, 64)) and perm[:64, 1].tolist() == list(range(64, 128))
    assert perm[64].tolist() == [128, 129]
    assert rows[:, 0].tolist() == list(range(64)) + [128] and rows[:, 1].tolist() == list(range(65))
    head, (g,), _ = _scalars(_plan(gym, tmp_path, "chains65_extra"))
    assert head["step_out_ok"] == 0 and (head["nf"], head["nf1"], g["aff"]) == (1, 0, 1)


def test_coupled_env_rows_and_pairs(gym, tmp_path):
    t = _plan(gym, tmp_path, "coupled_narrow")
    head, _, (eg,) = _scalars(t)
    row = t[N.MG_LAYOUT_ENV_FLAT]
    # art-free 0 and 1, free 0 / 1 - static 0; the free-free pair (bit 8) and the link-static pair (bit 4) masked out
    assert row[12] == (1 << 0) | (1 << 1) | (1 << 14) | (1 << 18)
    assert (row[2], row[7], row[13], row[14], row[15]) == (2, 1, 0, 0, 9)
    pairs = t[N.MG_LAYOUT_PAIRS].reshape(-1, 4)
    assert pairs[:, 0].tolist() == [64, 64, 64, 65, 65, 65, 1, 1, 1]   # free 0, free 1, then the moving link
    assert pairs[:, 2].tolist() == [-1, 80, 0, -1, 80, 0, -1, 64, 65]  # ground, static, fixed base; ground, frees
    assert (eg["wide"], eg["max_free"], eg["count"], head["n_coupled"]) == (0, 2, 1, 1)
    _, _, (eg,) = _scalars(_plan(gym, tmp_path, "coupled_wide"))
    assert (eg["wide"], eg["count"]) == (1, 1)
    t = _plan(gym, tmp_path, "coupled_narrow_and_wide")
    _, _, (e0, e1) = _scalars(t)
    assert [(e["wide"], e["offset"], e["count"]) for e in (e0, e1)] == [(0, 0, 1), (1, 1, 2)]
    assert t[N.MG_LAYOUT_CENV_ROW].tolist() == [1, 0, 2]
    rec16, rec64 = 8 + 24 * 16, N.lib.mg_env_ctab_floats()          # include/migym.h mg_debug_copy_env_ctab
    assert t[N.MG_LAYOUT_CENV_CTAB_OFF].tolist() == [rec64, 0, rec64 + rec64]
    assert rec16 < rec64


def test_floating_base_is_coupled_alone(gym, tmp_path):
    head, (g,), (eg,) = _scalars(_plan(gym, tmp_path, "floating"))
    assert head["n_coupled"] == 1 and g["step_count"] == 0 and g["count"] == 1 and eg["count"] == 1


def test_pile_envs_share_lists(gym, tmp_path):
    t = _plan(gym, tmp_path, "pile")
    head, _, _ = _scalars(t)
    rows = t[N.MG_LAYOUT_PILE_ROWS].reshape(3, -1)
    assert head["n_pile"] == 3 and rows[:, 1].tolist() == [3, 3, 3]
    assert (rows[0, 2], rows[0, 9]) == (rows[1, 2], rows[1, 9])      # built alike: one pair list, one slot table
    assert (rows[2, 2], rows[2, 9]) == (6, 3) and rows[:, 3].tolist() == [6, 6, 5]
    assert len(t[N.MG_LAYOUT_PILE_PAIRS]) == 11 and len(t[N.MG_LAYOUT_PILE_SLOTS]) == 2 * 6


# the messages as the source before the planner printed them (migym_capi.cpp's mg_upload_model)
MESSAGES = {
    "pile_too_many": (-4, "env 0: 65 free / 0 static bodies in contact range; a pile env supports 64 / 4"),
    "two_artics": (-4, "env 0: 2 articulations / 1 free / 0 static bodies in contact range; the coupled step "
                       "supports 1 / 2 / 4"),
    "actors_out_of_order": (-1, "actor_coll needs actors in body order"),
    "hull_edge_out_of_range": (-1, "shape 0: hull edge vertex out of range"),
    "links_not_topological": (-1, "articulation template 0: links not in topological order"),
    "floating_without_coll": (-4, "articulation template 0: a floating base steps in the coupled per-env kernel, "
                                  "which needs actor_coll"),
    "coupled_three_boxes": (-4, "env 0: 1 articulations / 3 free / 1 static bodies in contact range; the coupled "
                                "step supports 1 / 2 / 4"),
}


@pytest.mark.parametrize("name", sorted(LS.REFUSALS))
def test_refusals(gym, tmp_path, name):
    sim, p, m = LS.REFUSALS[name](gym, tmp_path)
    assert not N.lib.mg_debug_plan_layout(ctypes.byref(p), ctypes.byref(m))
    want = FIX["refusals"][name]
    assert (want["code"], want["error"]) == MESSAGES[name]
    assert N.last_error() == want["error"] and N.lib.mg_last_error_code() == want["code"]
    with pytest.raises(N.MigymError) as e:
        N.plan_layout(p, m)
    assert str(e.value) == want["error"]


def test_abi_symbols():
    for name in ("mg_debug_plan_layout", "mg_debug_layout_table", "mg_debug_free_layout"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(N.LIB_PATH), name)
    assert not N.lib.mg_debug_plan_layout(None, None) and "null" in N.last_error()
    N.lib.mg_debug_free_layout(None)
