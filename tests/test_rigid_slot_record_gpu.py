"""GPU parity of the one-round free-body step's entry and exit (mg_rigid.hip
k_rigid_step1): the packed per-slot record (root row, template,
rigid-body row, actor row in one 16-byte load), the ground-patch record fetched
beside it and selected by the far test, the fused root rows read at their fixed
stride, and the fused output rows stored with no load before them. Every case
steps the oracle (oracle/migym_oracle.c, its contact cache kept from step to
step) beside the GPU sim and compares bit for bit, every frame:

  - partly filled and mixed waves: 1 env (one wave, 62 dead lanes), 33 envs
    (wave 0 holds both templates, wave 1 two live lanes), 96 envs (three full
    waves): 20 frames of random teleports, then the vehicles set down and 20
    frames of rest;
  - every binding of the fused paths at 33 envs: fusion off, STEP_FUSION_ALL
    with both state tensors acquired, with the root tensor alone, with the
    rigid-body tensor alone (the root set then comes from a tensor of the
    caller's own);
  - a stale patch behind a far body (64 envs): resting vehicles, every other
    one lifted to 50 m for two frames and set back: a fetched record used by a
    far body, or ignored by a near one, breaks parity;
  - the unfused source at 33 envs: an indexed root set on odd frames (no fused
    root rows: the SoA state is read at the top), the full fused set on even ones;
  - a captured graph of 4 fused steps replayed 3 times against 12 eager steps.
"""
import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import scenes
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TELEPORTS, REST = 20, 20
NO_DOF = np.zeros((0, 2), np.float32)

_REF = {}


def _reference(gym, n):
    """The oracle's trajectory of the n-env servo scene (TELEPORTS frames of
    scenes.servo_actions seed 31, the vehicles set down, REST frames): per frame
    the body states and the net contact forces. Computed once per size, shared
    by the cases of that size, read-only."""
    if n not in _REF:
        sim, _ = scenes.servo_scene(gym, n)
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
                st[roots[1::2], 2] = 1.4
                st[roots[1::2], 3:7] = acts[k - 1][1::2, 0:4]
                st[roots[1::2], 7:13] = 0.0
            cf = oracle.step(p, m, st, NO_DOF, contact_cache=cc)
            s, c = st.copy(), np.array(cf, copy=True)
            s.setflags(write=False)
            c.setflags(write=False)
            frames.append((s, c))
        gym.destroy_sim(sim)
        _REF[n] = frames
    return _REF[n]


def _run_against_reference(gym, n, fusion, want_root=True, want_rb=True):
    """The reference's trajectory on the GPU; the acquired state tensors and the
    net contact force equal the oracle's after every frame. Without the root
    tensor the root sets come from a tensor of the caller's own."""
    frames = _reference(gym, n)
    sim, _ = scenes.servo_scene(gym, n)
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
    for k, (st, cf) in enumerate(frames):
        if k < TELEPORTS:
            src[:, 3:10] = acts[k]
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(src))
        elif k == TELEPORTS:
            src[1::2, 2] = 1.4
            src[1::2, 3:7] = acts[k - 1][1::2, 0:4]
            src[1::2, 7:13] = 0.0
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(src))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
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
def test_partial_and_mixed_waves_bitexact(gym, n):
    _run_against_reference(gym, n, gymapi.STEP_FUSION_ALL)


@pytest.mark.parametrize("binding", ["off", "all", "root_only", "rb_only"])
def test_fused_bindings_bitexact(gym, binding):
    fusion = 0 if binding == "off" else gymapi.STEP_FUSION_ALL
    _run_against_reference(gym, 33, fusion, want_root=binding != "rb_only", want_rb=binding != "root_only")


@pytest.mark.parametrize("fusion", [0, gymapi.STEP_FUSION_ALL])
def test_stale_patch_behind_far_body_bitexact(gym, fusion):
    n = 64
    sim, _ = scenes.servo_scene(gym, n)
    gym.prepare_sim(sim)
    if fusion:
        gym.set_step_fusion(sim, fusion)
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    p, m = sim.mg_params(), sim.mg_model()
    cc = oracle.contact_cache(m)
    st = sim.model_arrays["body_state0"].copy()
    roots = sim.model_arrays["actor_root_body"]
    veh = roots[1::2]
    lifted = veh[0::2]
    rows = torch.arange(1, 2 * n, 4, device=DEV)   # the root rows of `lifted`
    gym.refresh_actor_root_state_tensor(sim)

    def frame(tag):
        # a full root set of the current state every frame: the fused source
        # path (with fusion) without a change of state
        assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(root))
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        cf = oracle.step(p, m, st, NO_DOF, contact_cache=cc)
        got = rb.cpu().numpy()
        assert np.array_equal(got, st), "%s: max |diff| %g" % (tag, np.abs(got - st).max())
        assert np.array_equal(root.cpu().numpy(), st[roots]), "%s: root state" % tag
        assert np.array_equal(ncf.cpu().numpy(), cf), "%s: contact force" % tag

    for k in range(90):   # the vehicles settle on two anchors each
        frame("settle %d" % k)
        if np.all(cc.body[veh, 0] == 2.0):
            break
    assert np.all(cc.body[veh, 0] == 2.0)
    # every other vehicle far above the ground for two frames: its record stays
    # in the table (fetched, never used), the oracle's cache drops to no anchor
    root[rows, 2] = 50.0
    root[rows, 7:13] = 0.0
    st[lifted, 2] = 50.0
    st[lifted, 7:13] = 0.0
    for k in range(2):
        frame("lifted %d" % k)
        assert np.all(cc.body[lifted, 0] == 0.0)
        assert np.all(cc.body[veh[1::2], 0] == 2.0)
    # back to just above the rest height, at rest: the stale record must not
    # come back; the anchors regrow from the new contacts
    root[rows, 2] = 1.4
    root[rows, 7:13] = 0.0
    st[lifted, 2] = 1.4
    st[lifted, 7:13] = 0.0
    for k in range(30):
        frame("back %d" % k)
    assert np.all(cc.body[lifted, 0] > 0.0)
    gym.destroy_sim(sim)


def test_unfused_source_alternating_bitexact(gym):
    n, frames = 33, 20
    sim, _ = scenes.servo_scene(gym, n)
    gym.prepare_sim(sim)
    gym.set_step_fusion(sim, gymapi.STEP_FUSION_ALL)
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    rb = gymtorch.wrap_tensor(gym.acquire_rigid_body_state_tensor(sim))
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(sim))
    acts = scenes.servo_actions(n, frames, DEV, seed=17)
    acts_h = acts.cpu().numpy()
    p, m = sim.mg_params(), sim.mg_model()
    cc = oracle.contact_cache(m)
    st = sim.model_arrays["body_state0"].copy()
    roots = sim.model_arrays["actor_root_body"]
    third = np.arange(0, 2 * n, 3)
    idx = torch.as_tensor(third, dtype=torch.int32, device=DEV)
    gym.refresh_actor_root_state_tensor(sim)
    for k in range(frames):
        if k % 2 == 1:   # an indexed set: applied at the call, the step reads the SoA state
            new = root.clone()
            new[:, 3:10] = acts[k]
            assert gym.set_actor_root_state_tensor_indexed(sim, gymtorch.unwrap_tensor(new),
                                                           gymtorch.unwrap_tensor(idx), len(third))
            st[roots[third], 3:10] = acts_h[k][third]
        else:            # the full set: read by the step from the tensor's rows
            root[:, 3:10] = acts[k]
            assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(root))
            st[roots, 3:10] = acts_h[k]
        gym.simulate(sim)
        gym.fetch_results(sim, True)
        gym.refresh_actor_root_state_tensor(sim)
        gym.refresh_rigid_body_state_tensor(sim)
        gym.refresh_net_contact_force_tensor(sim)
        cf = oracle.step(p, m, st, NO_DOF, contact_cache=cc)
        got = rb.cpu().numpy()
        assert np.array_equal(got, st), "frame %d: max |diff| %g" % (k, np.abs(got - st).max())
        assert np.array_equal(root.cpu().numpy(), st[roots]), "frame %d: root state" % k
        assert np.array_equal(ncf.cpu().numpy(), cf), "frame %d: contact force" % k
    gym.destroy_sim(sim)


def test_graph_replay_matches_eager(gym):
    n, chunk, replays = 33, 4, 3
    acts = scenes.servo_actions(n, chunk * replays, DEV, seed=23)
    sims = []
    for _ in range(2):
        sim, _ = scenes.servo_scene(gym, n)
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
    for r in range(replays):
        g.replay()
        for _ in range(chunk):
            step(sb, rb_, kb)
        torch.cuda.synchronize()
        assert np.array_equal(ra.cpu().numpy(), rb_.cpu().numpy()), "replay %d: root state" % r
        assert np.array_equal(rba.cpu().numpy(), rbb.cpu().numpy()), "replay %d: rigid-body state" % r
    assert int(ka.item()) == chunk * replays and np.all(np.isfinite(rba.cpu().numpy()))
    for sim, _, _, _ in sims:
        gym.destroy_sim(sim)
