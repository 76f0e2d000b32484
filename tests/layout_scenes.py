"""Small models for the layout planner's tests (tests/test_layout.py, DESIGN.md
§2.1), each the smallest shape at which one piece of the planner can go wrong.
Every builder returns (sim, mg_sim_params, mg_model); the sim keeps the arrays
alive. CASES are planned and compared table by table with
tests/golden/layout_fixture.json; REFUSALS are refused with a recorded code
and message."""
from isaacgym import gymapi
import pile_scenes as PS

CHAIN = """<robot name="ch%d"><link name="base"><collision><geometry><box size="0.1 0.1 0.1"/></geometry></collision>
<inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link>
%s</robot>"""
LINK = """<link name="l%d"><collision><origin xyz="0 0 0.1"/><geometry><box size="0.05 0.05 0.2"/></geometry></collision>
<inertial><origin xyz="0 0 0.1"/><mass value="0.5"/>
<inertia ixx="0.002" iyy="0.002" izz="0.001" ixy="0" ixz="0" iyz="0"/></inertial></link>
<joint name="j%d" type="revolute"><parent link="%s"/><child link="l%d"/><origin xyz="0 0 %g"/><axis xyz="0 1 0"/>
<limit lower="-1" upper="1" effort="10" velocity="5"/></joint>
"""
TWO = """<robot name="two"><link name="b">
<collision><origin xyz="0.06 0 0"/><geometry><box size="0.1 0.1 0.1"/></geometry></collision>
<collision><origin xyz="-0.06 0 0"/><geometry><sphere radius="0.05"/></geometry></collision>
<inertial><mass value="1"/><inertia ixx="0.01" iyy="0.01" izz="0.01" ixy="0" ixz="0" iyz="0"/></inertial></link></robot>"""
FLOAT = """<mujoco model="fl"><worldbody><body name="torso" pos="0 0 1"><freejoint/>
<geom type="sphere" size="0.1"/>
<body name="arm" pos="0.2 0 0"><joint name="j" type="hinge" axis="0 1 0"/>
<geom type="sphere" size="0.05"/></body></body></worldbody></mujoco>"""


def _sim(gym):
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, PS.sim_params(False))
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, plane)
    return sim


def _env(gym, sim):
    return gym.create_env(sim, gymapi.Vec3(-1, -1, 0), gymapi.Vec3(1, 1, 2), 8)


def _at(x, y, z):
    return gymapi.Transform(gymapi.Vec3(x, y, z))


def _asset(gym, sim, tmp, name, text, fixed=False):
    (tmp / name).write_text(text)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = fixed
    asset = gym.load_asset(sim, str(tmp), name, opts)
    assert asset is not None
    return asset


def _chain(gym, sim, tmp, hinges=1):
    """A fixed-base serial chain of `hinges` hinges (nl = hinges + 1)."""
    links = "".join(LINK % (k, k, "base" if k == 0 else "l%d" % (k - 1), k, 0.05 if k == 0 else 0.2)
                    for k in range(hinges))
    return _asset(gym, sim, tmp, "ch%d.urdf" % hinges, CHAIN % (hinges, links), fixed=True)


def _done(sim, edit=None, drop_coll=False):
    A = sim.build_model()
    if edit is not None:
        edit(A)
    m = sim.mg_model(A)
    if drop_coll:
        m.actor_coll = None
    return sim, sim.mg_params(), m


def free_order(gym, tmp, two_shape=True):
    """Two single-shape templates at different heights, interleaved in body
    order (the low one created first), and one two-shape body; filter 1 on all:
    nothing may touch, so every body steps in the free-body kernel."""
    sim = _sim(gym)
    lo = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    hi = gym.create_sphere(sim, 0.05, gymapi.AssetOptions())
    two = _asset(gym, sim, tmp, "two.urdf", TWO) if two_shape else None
    env = _env(gym, sim)
    for k, a in enumerate((lo, hi, two, lo, hi)):
        if a is not None:
            gym.create_actor(env, a, _at(0.3 * k, 0, 0.05 if a is lo else 2.0 if a is hi else 1.0), None, 0, 1)
    return _done(sim)


def free_order_single(gym, tmp):
    return free_order(gym, tmp, two_shape=False)


def chains65(gym, tmp, extra=False):
    """65 uncoupled one-hinge chains: a full block of 64 and a tail block of 1."""
    sim = _sim(gym)
    ch = _chain(gym, sim, tmp)
    two = _asset(gym, sim, tmp, "two.urdf", TWO) if extra else None
    for i in range(65):
        gym.create_actor(_env(gym, sim), ch, _at(0, 0, 0.5), None, i, 0)
    if extra:      # alone in its env: uncoupled, stepped by the multi-shape free-body kernel
        gym.create_actor(_env(gym, sim), two, _at(1, 0, 1.0), None, 65, 0)
    return _done(sim)


def chains65_extra(gym, tmp):
    return chains65(gym, tmp, extra=True)


def coupled(gym, tmp, hinges=1, boxes=2, more=()):
    """One env: a fixed-base chain, `boxes` free boxes, one static box. Filters:
    chain 1, static 1 (the link-static pair is masked out), boxes 2 (the
    free-free pairs are masked out); chain-box and box-static pairs collide.
    more: further envs of the same chain and that many boxes, all colliding."""
    sim = _sim(gym)
    ch = _chain(gym, sim, tmp, hinges)
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    fixed = gymapi.AssetOptions()
    fixed.fix_base_link = True
    table = gym.create_box(sim, 0.3, 0.3, 0.1, fixed)
    env = _env(gym, sim)
    gym.create_actor(env, ch, _at(0, 0, 0.05), "chain", 0, 1)
    for k in range(boxes):
        gym.create_actor(env, box, _at(0.5 + 0.2 * k, 0, 0.05), "box%d" % k, 0, 2)
    gym.create_actor(env, table, _at(0, 0.6, 0.05), "table", 0, 1)
    for i, nbox in enumerate(more):
        env = _env(gym, sim)
        gym.create_actor(env, ch, _at(0, 0, 0.05), "chain", 1 + i, 0)
        for k in range(nbox):
            gym.create_actor(env, box, _at(0.5 + 0.2 * k, 0, 0.05), None, 1 + i, 0)
    return sim


def coupled_narrow(gym, tmp):      # 1 DOF + 2 x 6 = 13 velocity slots
    return _done(coupled(gym, tmp))


def coupled_wide(gym, tmp):        # 5 DOFs + 2 x 6 = 17 velocity slots: a 64-lane env
    return _done(coupled(gym, tmp, hinges=5))


def coupled_narrow_and_wide(gym, tmp):
    """Three envs of one template, 17, 11 and 17 velocity slots: the groups
    split by width, the narrow env's row comes first and h_cenv_row differs
    from env order."""
    return _done(coupled(gym, tmp, hinges=5, more=(1, 2)))


def floating(gym, tmp, drop_coll=False):
    """One free-joint MJCF body alone in its env: coupled without a partner."""
    sim = _sim(gym)
    a = _asset(gym, sim, tmp, "fl.xml", FLOAT)
    gym.create_actor(_env(gym, sim), a, _at(0, 0, 1), None, 0, 0)
    return _done(sim, drop_coll=drop_coll)


def pile(gym, tmp):
    """Two envs of MG_ENV_MAXF + 1 = 3 spheres built alike (filters 1, 0, 0: all
    pairs collide), a third with one filter bit changed (1, 1, 0: pair (0, 1)
    masked out)."""
    sim = _sim(gym)
    ball = gym.create_sphere(sim, 0.05, gymapi.AssetOptions())
    for i, filters in enumerate(((1, 0, 0), (1, 0, 0), (1, 1, 0))):
        env = _env(gym, sim)
        for k, f in enumerate(filters):
            gym.create_actor(env, ball, _at(0.2 * k, 0, 0.05), None, i, f)
    return _done(sim)


def chains_and_boxes(gym, tmp, n=4):
    """n coupled envs of a one-hinge chain and two free boxes on the ground
    (tests/test_upload_retry_gpu.py's good model)."""
    sim = _sim(gym)
    ch = _chain(gym, sim, tmp)
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    for i in range(n):
        env = _env(gym, sim)
        gym.create_actor(env, ch, _at(0, 0, 0.05), "chain", i, 0)
        gym.create_actor(env, box, _at(0.3, 0, 0.05 + 0.01 * i), "a", i, 0)
        gym.create_actor(env, box, _at(0.3, 0, 0.16 + 0.01 * i), "b", i, 0)
    return _done(sim)


# ---- refusals

def pile_too_many(gym, tmp):
    """MG_PILE_MAXB + 1 = 65 free bodies in contact range in one env (and a
    chain in a second env: max_actor_dofs 1)."""
    sim = _sim(gym)
    ball = gym.create_sphere(sim, 0.02, gymapi.AssetOptions())
    env = _env(gym, sim)
    for k in range(65):
        gym.create_actor(env, ball, _at(0.05 * (k % 8), 0.05 * (k // 8), 0.5), None, 0, 0)
    gym.create_actor(_env(gym, sim), _chain(gym, sim, tmp, 5), _at(0, 0, 0.05), None, 1, 0)
    return _done(sim)


def two_artics(gym, tmp):
    sim = _sim(gym)
    ch = _chain(gym, sim, tmp)
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    env = _env(gym, sim)
    gym.create_actor(env, ch, _at(0, 0, 0.05), None, 0, 0)
    gym.create_actor(env, ch, _at(1, 0, 0.05), None, 0, 0)
    gym.create_actor(env, box, _at(0.5, 0, 0.05), None, 0, 0)
    return _done(sim)


def actors_out_of_order(gym, tmp):
    def edit(A):
        A["actor_root_body"][[0, 1]] = A["actor_root_body"][[1, 0]]
    sim = _sim(gym)
    box = gym.create_box(sim, 0.1, 0.1, 0.1, gymapi.AssetOptions())
    env = _env(gym, sim)
    for k in range(2):
        gym.create_actor(env, box, _at(0.5 * k, 0, 0.05), None, 0, 0)
    return _done(sim, edit)


def hull_edge_out_of_range(gym, tmp):
    def edit(A):
        h = A["hulls"]
        nv, nf = int(h[0]), int(h[1])
        h[4 + 3 * nv + 4 * nf] = nv
    sim = _sim(gym)
    a = gym.load_asset(sim, str(tmp), PS.hull_urdf(str(tmp)), gymapi.AssetOptions())
    gym.create_actor(_env(gym, sim), a, _at(0, 0, 0.5), None, 0, 0)
    return _done(sim, edit)


def links_not_topological(gym, tmp):
    def edit(A):
        A["tmpl_link_i"][1, 0] = 1
    sim = _sim(gym)
    gym.create_actor(_env(gym, sim), _chain(gym, sim, tmp, 2), _at(0, 0, 0.05), None, 0, 0)
    return _done(sim, edit)


def floating_without_coll(gym, tmp):
    return floating(gym, tmp, drop_coll=True)


def coupled_three_boxes(gym, tmp):
    """A chain and 3 free boxes (19 velocity slots): past MG_ENV_MAXF = 2."""
    return _done(coupled(gym, tmp, boxes=3))


CASES = {f.__name__: f for f in (free_order, free_order_single, chains65, chains65_extra, coupled_narrow,
                                 coupled_wide, coupled_narrow_and_wide, floating, pile)}
REFUSALS = {f.__name__: f for f in (pile_too_many, two_artics, actors_out_of_order, hull_edge_out_of_range,
                                    links_not_topological, floating_without_coll, coupled_three_boxes)}
