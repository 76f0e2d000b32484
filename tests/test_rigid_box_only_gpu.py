"""GPU parity of the one-round free-body step's box-only build (mg_rigid.hip
k_rigid_step1 BOX): the candidate search compiled for a box at
the body origin alone, picked when the plan says every single-shape free body
is such a box. Every case steps the oracle (oracle/migym_oracle.c, its contact
cache kept from step to step) beside the GPU sim and compares bit for bit, every
frame: 20 frames of random teleports, then the vehicles (and balls) set down
and 20 frames of rest. mg_last_rigid_form says which build ran:

  - the servo scene at 1 env (62 dead lanes), 33 envs (wave 0 holds both
    templates) and 96 envs, STEP_FUSION_ALL: record + box-only;
  - 33 envs with fusion off, with the root tensor alone and with the rigid-body
    tensor alone: the same build with the SoA state as its source, or one of
    the fused outputs absent;
  - envs that alternate the creation order of their two actors (root rows and
    rigid-body rows no progression in the slot): record + box-only;
  - a vehicle and a ball per env: a sphere among the shapes, so the record
    build with the general candidates;
  - a captured graph of 4 fused steps replayed 3 times against 12 eager steps.
"""
import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N, scenes
import oracle
import rigid_box_scenes as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TELEPORTS, REST = 20, 20
NO_DOF = np.zeros((0, 2), np.float32)
REC_BOX = N.MG_RIGID_FORM_REC | N.MG_RIGID_FORM_BOX

_REF = {}


def _set_down(state, rows_of, veh, ball, quats):
    """Frame TELEPORTS: the vehicles just above their rest height with a yaw-only
    orientation, the balls just above theirs, all at rest."""
    state[rows_of(veh), 2] = 1.4
    state[rows_of(veh), 3:7] = quats
    state[rows_of(veh), 7:13] = 0.0
    if len(ball):
        state[rows_of(ball), 2] = 0.25
        state[rows_of(ball), 7:13] = 0.0


def _reference(gym, kind, n):
    """The oracle's trajectory of scene `kind` at n envs: per frame the body
    states and the net contact forces. Computed once per scene and size, shared
    by the cases that use it, read-only."""
    if (kind, n) not in _REF:
        sim, veh, ball = RS.build(gym, kind, n)
        gym.prepare_sim(sim)
        p, m = sim.mg_params(), sim.mg_model()
        cc = oracle.contact_cache(m)
        st = sim.model_arrays["body_state0"].copy()
        roots = sim.model_arrays["actor_root_body"]
        acts = scenes.servo_actions(n, TELEPORTS, DEV, seed=31).cpu().numpy()
        frames = []
        for k in range(TELEPORTS + REST):
            if k < TELEPORTS:
                st[roots, 3:10] = acts[k]
            elif k == TELEPORTS:
                _set_down(st, lambda r: roots[r], veh, ball, acts[k - 1][1::2, 0:4])
            cf = oracle.step(p, m, st, NO_DOF, contact_cache=cc)
            s, c = st.copy(), np.array(cf, copy=True)
            s.setflags(write=False)
            c.setflags(write=False)
            frames.append((s, c))
        gym.destroy_sim(sim)
        _REF[(kind, n)] = frames
    return _REF[(kind, n)]


def _run_against_reference(gym, kind, n, fusion, want_form, want_root=True, want_rb=True):
    frames = _reference(gym, kind, n)
    sim, veh, ball = RS.build(gym, kind, n)
    gym.prepare_sim(sim)
    if fusion:
        gym.set_step_fusion(sim, fusion)
    roots = sim.model_arrays["actor_root_body"]
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim)) if want_root else None
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim)) if want_rb else None
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    acts = scenes.servo_actions(n, TELEPORTS, DEV, seed=31)
    if want_root:
        gym.refresh_actor_root_state_tensor(sim)
        src = root
    else:
        src = torch.from_numpy(sim.model_arrays["body_state0"][roots].copy()).to(DEV)
    roots_t = torch.as_tensor(roots, device=DEV, dtype=torch.long)
    assert N.lib.mg_last_rigid_form(sim.native) == -1
    for k, (st, cf) in enumerate(frames):
        if k < TELEPORTS:
            src[:, 3:10] = acts[k]
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(src))
        elif k == TELEPORTS:
            _set_down(src, lambda r: torch.as_tensor(r, device=DEV), veh, ball, acts[k - 1][1::2, 0:4])
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(src))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        assert N.lib.mg_last_rigid_form(sim.native) == want_form
        if want_root:
            gym.refresh_actor_root_state_tensor(sim)
        if want_rb:
            gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        if want_rb:
            got = rb.cpu().numpy()
            assert np.array_equal(got, st), "frame %d: rigid-body state, max |diff| %g" % (k, np.abs(got - st).max())
            if not want_root:
                src.copy_(rb[roots_t])   # the caller's own root tensor follows the state
        if want_root:
            got = root.cpu().numpy()
            assert np.array_equal(got, st[roots]), "frame %d: root state, max |diff| %g" % (
                k, np.abs(got - st[roots]).max())
        assert np.array_equal(ncf.cpu().numpy(), cf), "frame %d: contact force" % k
    gym.destroy_sim(sim)


@pytest.mark.parametrize("n", [1, 33, 96])
def test_servo_box_only_bitexact(gym, n):
    _run_against_reference(gym, "servo", n, gymapi.STEP_FUSION_ALL, REC_BOX)


@pytest.mark.parametrize("binding", ["off", "root_only", "rb_only"])
def test_servo_box_only_bindings_bitexact(gym, binding):
    fusion = 0 if binding == "off" else gymapi.STEP_FUSION_ALL
    _run_against_reference(gym, "servo", 33, fusion, REC_BOX, want_root=binding != "rb_only",
                           want_rb=binding != "root_only")


def test_alternating_order_box_only_bitexact(gym):
    _run_against_reference(gym, "alternating", 33, gymapi.STEP_FUSION_ALL, REC_BOX)


def test_vehicle_and_ball_general_shapes_bitexact(gym):
    _run_against_reference(gym, "ball", 33, gymapi.STEP_FUSION_ALL, N.MG_RIGID_FORM_REC)


def test_graph_replay_matches_eager(gym):
    n, chunk, replays = 33, 4, 3
    acts = scenes.servo_actions(n, chunk * replays, DEV, seed=23)
    sims = []
    for _ in range(2):
        sim, _, _ = RS.build(gym, "servo", n)
        gym.prepare_sim(sim)
        gym.set_step_fusion(sim, gymapi.STEP_FUSION_ALL)
        root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
        rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
        gym.refresh_actor_root_state_tensor(sim)
        sims.append((sim, root, rb, torch.zeros(1, dtype=torch.long, device=DEV)))

    def step(sim, root, kdev):
        root[:, 3:10] = acts.index_select(0, kdev).squeeze(0)
        kdev.add_(1)
        gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(root))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)

    (sa, ra, rba, ka), (sb, rb_, rbb, kb) = sims
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # records without executing
        for _ in range(chunk):
            step(sa, ra, ka)
    assert N.lib.mg_last_rigid_form(sa.native) == REC_BOX
    for r in range(replays):
        g.replay()
        for _ in range(chunk):
            step(sb, rb_, kb)
        torch.cuda.synchronize()
        assert np.array_equal(ra.cpu().numpy(), rb_.cpu().numpy()), "replay %d: root state" % r
        assert np.array_equal(rba.cpu().numpy(), rbb.cpu().numpy()), "replay %d: rigid-body state" % r
    assert N.lib.mg_last_rigid_form(sb.native) == REC_BOX
    assert int(ka.item()) == chunk * replays and np.all(np.isfinite(rba.cpu().numpy()))
    for sim, _, _, _ in sims:
        gym.destroy_sim(sim)
