"""Articulation forward dynamics on the GPU against float64: the
scenes, draws and tolerances of tests/test_dynamics_kat.py through the tensor
API — set_dof_state_tensor, set_actor_root_state_tensor (the ant),
set_dof_actuation_force_tensor, one simulate of one substep, the refreshes —
and the device result compared directly with tests/dynamics64.py, not with the
oracle: a failure here names physics. One test per kernel form, at the smallest
launch that reaches it; the form is asserted where the library tells
(mg_num_coupled_envs, mg_debug_artic_groups) and named in the docstring."""
import numpy as np
import pytest
import torch

from isaacgym import gymapi, gymtorch
from test_isaacgym_amd import _native as N
from test_dynamics_kat import ENVS, make_case, _wrench_case
from test_step_out_chain_gpu import _artic_groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _step(gym, c, before=None):
    """The case's state and efforts in, one simulate, the new state out:
    (dof (n, D, 2), roots (n, 13) or None)."""
    sim = c.sim
    dof = gymtorch.wrap_tensor(gym.acquire_dof_state_tensor(sim))
    root = gymtorch.wrap_tensor(gym.acquire_actor_root_state_tensor(sim))
    assert gym.set_dof_state_tensor(sim, gymtorch.unwrap_tensor(_dev(np.stack([c.q, c.u], axis=2).reshape(-1, 2))))
    if c.root is not None:
        assert root.shape[0] == c.n                                    # one actor per env
        assert gym.set_actor_root_state_tensor(sim, gymtorch.unwrap_tensor(_dev(c.root)))
    assert gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(_dev(c.tau.reshape(-1))))
    if before is not None:
        before()
    gym.simulate(sim)
    gym.fetch_results(sim, True)
    gym.refresh_dof_state_tensor(sim)
    gym.refresh_actor_root_state_tensor(sim)
    got = dof.cpu().numpy().reshape(c.n, c.D, 2)
    assert np.all(np.isfinite(got))
    return got, (root.cpu().numpy() if c.root is not None else None)


def _group(sim, n):
    """The one articulation group that steps (mg_debug_artic_groups)."""
    grp = [g for g in _artic_groups(sim) if g["step_count"] > 0]
    assert len(grp) == 1 and grp[0]["step_count"] == n, grp
    return grp[0]


@pytest.mark.parametrize("name", ["chain2", "chain3", "chain4", "gimbal"])
def test_chain_quad(gym, tmp_path, name):
    """k_artic_chain_q<NL> (four lanes per chain: 5 chains are 20 lanes of one
    wave), NL = 2, 3, 4 on the purpose-made chains under skew gravity and NL = 4
    on the stock gimbal, properties shared by all envs."""
    c = make_case(name, gym, str(tmp_path), ENVS[name], gpu=True)
    gym.prepare_sim(c.sim)
    g = _group(c.sim, c.n)
    assert (g["chain"], g["nl"], g["uni_mass"]) == (1, c.D + 1, 1), g
    assert c.n * 4 <= 64 * 1024                              # MG_CHAIN_QUAD_MAX: the four-lane launch
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)


def test_chain_quad_own_link_masses(gym):
    """k_artic_chain_q without shared constants: env 1's links three times as heavy."""
    c = make_case("gimbal", gym, None, ENVS["gimbal"], gpu=True, link_mass_env=1)
    gym.prepare_sim(c.sim)
    g = _group(c.sim, c.n)
    assert (g["chain"], g["nl"], g["uni_mass"]) == (1, 4, 0), g
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)


@pytest.mark.parametrize("form", ["aff", "own_masses"])
def test_chain_one_lane(gym, form):
    """k_artic_chain, one lane per chain: 16384 + 70 gimbals, just past the
    four-lane bound (MG_CHAIN_QUAD_MAX / 4). `aff`: shared properties, instance
    rows computed from the blocked layout (<4, EXT 0, UNI 1, AFF 1>);
    `own_masses`: one env's links heavier, so neither (<4, 0, 0, 0>, the
    non-affine form). One step; the float64 reference on 24 envs: the first
    wave, the last, partly filled one (70 = 64 + 6 lanes), the heavy env and
    random others."""
    n = 16384 + 70
    heavy = 16384 + 66
    rng = np.random.RandomState(5)
    sel = sorted({0, 1, 31, 63, n - 70, n - 7, n - 6, heavy, n - 2, n - 1} | set(rng.choice(n, 14, replace=False)))
    c = make_case("gimbal", gym, None, n, gpu=True, sel=sel, link_mass_env=heavy if form == "own_masses" else None)
    gym.prepare_sim(c.sim)
    g = _group(c.sim, n)
    assert (g["chain"], g["nl"], g["aff"]) == (1, 4, 1), g
    assert g["uni_mass"] == (1 if form == "aff" else 0), g
    assert n * 4 > 64 * 1024                                 # past MG_CHAIN_QUAD_MAX: the one-lane launch
    got, _ = _step(gym, c)
    assert np.count_nonzero(got[:, :, 1] != c.u) > 2 * n     # every chain stepped
    c.compare(got)
    gym.destroy_sim(c.sim)


def test_lanes_franka(gym, tmp_path):
    """k_artic_lanes (16 lanes per articulation, 4 per wavefront): 5 Frankas —
    one full wave and one with three idle groups; all 9 DOFs, gravity on."""
    c = make_case("franka", gym, str(tmp_path), ENVS["franka"], gpu=True)
    gym.prepare_sim(c.sim)
    assert N.lib.mg_num_coupled_envs(c.sim.native) == 0
    assert _group(c.sim, c.n)["chain"] == 0
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)


@pytest.mark.parametrize("at_pos", [False, True])
def test_lanes_franka_external_wrench(gym, tmp_path, at_pos):
    """k_artic_lanes' external-wrench form: apply_rigid_body_force_tensors (force
    at the COM + torque) and apply_rigid_body_force_at_pos_tensors (force at a
    world point) on panda_link4 and panda_hand; the reference adds J^T of the
    wrench at the point the API defines."""
    c = _wrench_case(gym, str(tmp_path), 5, gpu=True, at_pos=at_pos)
    gym.prepare_sim(c.sim)
    nb = c.A["body_state0"].shape[0]
    F, X = np.zeros((nb, 3)), np.zeros((nb, 3))
    for e, dyn in c.dyn.items():
        for b, (f, x) in ((c.ext_at if at_pos else c.ext)[e]).items():
            F[dyn.first_body + b], X[dyn.first_body + b] = f, x

    def apply():
        f, x = gymtorch.unwrap_tensor(_dev(F)), gymtorch.unwrap_tensor(_dev(X))
        if at_pos:
            assert gym.apply_rigid_body_force_at_pos_tensors(c.sim, f, x, gymapi.ENV_SPACE)
        else:
            assert gym.apply_rigid_body_force_tensors(c.sim, f, x, gymapi.ENV_SPACE)

    c.compare(*_step(gym, c, before=apply))
    gym.destroy_sim(c.sim)


def test_env_step_fixed_base(gym, tmp_path):
    """k_env_step with a fixed base: 5 coupled cube-pick envs (table, cube,
    gravity-free Franka), the arm clear of everything — no contact force on any
    of its links."""
    c = make_case("cubepick", gym, str(tmp_path), ENVS["cubepick"], gpu=True)
    gym.prepare_sim(c.sim)
    assert N.lib.mg_num_coupled_envs(c.sim.native) == c.n
    ncf = gymtorch.wrap_tensor(gym.acquire_net_contact_force_tensor(c.sim))
    got = _step(gym, c)
    gym.refresh_net_contact_force_tensor(c.sim)
    links = np.concatenate([d.first_body + np.arange(len(d.art.bodies())) for d in c.dyn.values()])
    assert not ncf.cpu().numpy()[links].any()
    c.compare(*got)
    gym.destroy_sim(c.sim)


def test_env_step_floating_base(gym, tmp_path):
    """k_env_step with a floating base: 5 ants 50 m up, random root attitude and
    twist; all 6 + 8 rows, the root's pose update included."""
    c = make_case("ant", gym, str(tmp_path), ENVS["ant"], gpu=True)
    gym.prepare_sim(c.sim)
    assert N.lib.mg_num_coupled_envs(c.sim.native) == c.n
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)


def test_lanes_ball_joint(gym, tmp_path):
    """k_artic_lanes with a ball joint's virtual links: 4 ball chains (3 sliders
    + 1 spherical joint), a rotation vector of 0.4..1.2 rad and an angular
    velocity across it."""
    c = make_case("ball", gym, str(tmp_path), ENVS["ball"], gpu=True)
    gym.prepare_sim(c.sim)
    assert N.lib.mg_num_coupled_envs(c.sim.native) == 0
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)


def test_lanes32_humanoid(gym, tmp_path):
    """k_artic_lanes<32, 64> (one articulation per wavefront): the fixed-base
    humanoid, 21 hinges in 25 kernel links — several hinges on one body, so
    virtual links."""
    c = make_case("humanoid", gym, str(tmp_path), ENVS["humanoid"], gpu=True)
    gym.prepare_sim(c.sim)
    assert N.lib.mg_num_coupled_envs(c.sim.native) == 0
    g = _group(c.sim, c.n)
    assert (g["chain"], g["nl"]) == (0, 25), g
    c.compare(*_step(gym, c))
    gym.destroy_sim(c.sim)
