"""Sleeping restated on the host, shared by tests/test_sleep.py
(CPU) and tests/test_sleep_gpu.py (device parity): the islands derived from the
model's actors, body kinds and collision groups alone (never from the
library's layout plan), and the pass in numpy float32 on top of oracle.step,
with the wakes. Every float32 operation is one numpy operation, so it is
rounded on its own as on the device (-ffp-contract=off)."""
import math

import numpy as np

from isaacgym import gymapi
from test_isaacgym_amd import _native as N, scenes
import oracle
import capacity_scenes as CS

THRESHOLD, WINDOW = 5e-5, 0.4


# ---------------------------------------------------------------- scenes
def ant_scene(gym, gpu, n=1):
    sim, _, _, _ = scenes.dr_ant_scene(gym, n, use_gpu_pipeline=gpu)
    return sim


def sphere_layer_scene(gym, gpu, n=2):
    sim = CS.new_sim(gym, gpu)
    for e in range(n):
        CS.add_sphere_layer(gym, sim, e, 3)
    return sim


def walled_cubes_scene(gym, gpu, n=2):
    sim = CS.new_sim(gym, gpu)
    for e in range(n):
        CS.add_walled_cubes(gym, sim, e, 1)
    return sim


def uncoupled_scene(gym, gpu, n=2):
    """Per env a box dropped from 2 cm and the gimbal (fixed base, position
    drives at their targets of 0), which touch nothing: the free-body kernel and
    the articulation kernel, two single-actor islands per env."""
    sp = scenes.servo_sim_params(gpu)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    plane = gymapi.PlaneParams()
    plane.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, plane)
    box = gym.create_box(sim, 0.2, 0.3, 0.1, gymapi.AssetOptions())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.default_dof_drive_mode = gymapi.DOF_MODE_POS
    gimbal = gym.load_asset(sim, scenes.ASSET_ROOT, "servo/gimbal.urdf", opts)
    assert gimbal is not None
    for e in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-1, -1, -1), gymapi.Vec3(1, 1, 1), 2)
        gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.0, 0.0, 0.07)), "box", e, 1)
        h = gym.create_actor(env, gimbal, gymapi.Transform(gymapi.Vec3(0.0, 2.0, 3.0)), "gimbal", e, 1)
        props = gym.get_actor_dof_properties(env, h)
        props["driveMode"][:] = gymapi.DOF_MODE_POS
        props["stiffness"][:] = 50.0
        props["damping"][:] = 5.0
        gym.set_actor_dof_properties(env, h, props)
    return sim


# ---------------------------------------------------------------- islands
def _collide(acoll, a, b):
    ga, gb, fa, fb = acoll[a, 1], acoll[b, 1], acoll[a, 2], acoll[b, 2]
    return (ga == gb or ga == -1 or gb == -1) and (int(fa) & int(fb)) == 0


def actor_bodies(A):
    """Per actor its global bodies: rows are env-major, actor order, tree order."""
    root = np.asarray(A["actor_root_body"])
    end = np.append(root[1:], len(A["body_kind"]))
    return [np.arange(root[a], end[a]) for a in range(len(root))]


def islands(A):
    """The islands as lists of actors, in order of their first actor: the moving
    actors of an env in which two bodies may touch (or that holds a
    floating-base articulation) together, every other moving actor alone."""
    root, kind, acoll = np.asarray(A["actor_root_body"]), np.asarray(A["body_kind"]), np.asarray(A["actor_coll"])
    floating = {}
    for r0, _, t, _ in np.asarray(A["artic_i"]).reshape(-1, N.MG_ARTIC_I_N):
        floating[int(r0)] = np.asarray(A["artic_tmpl_i"]).reshape(-1, N.MG_ATMPL_I_N)[t, 3] == 0
    out, of_env = [], {}
    envs = {}
    for a in range(len(root)):
        envs.setdefault(int(acoll[a, 0]), []).append(a)
    coupled = {}
    for e, acts in envs.items():
        mov = [a for a in acts if kind[root[a]] != N.MG_BODY_STATIC]
        stc = [a for a in acts if kind[root[a]] == N.MG_BODY_STATIC]
        c = any(_collide(acoll, a, b) for i, a in enumerate(mov) for b in mov[i + 1:] + stc)
        coupled[e] = c or any(floating.get(int(root[a]), False) for a in mov)
    for a in range(len(root)):
        if kind[root[a]] == N.MG_BODY_STATIC:
            continue
        e = int(acoll[a, 0])
        if not coupled[e]:
            out.append([a])
        elif e in of_env:
            out[of_env[e]].append(a)
        else:
            of_env[e] = len(out)
            out.append([a])
    return out


def body_k(A):
    """k_b = 4 r_b^2 per global body, float32: r_b the largest |p_s| + extent_s
    over the body's shapes, in double; a body without shapes takes its actor's
    largest."""
    tbi, shapes, tmpl = np.asarray(A["tmpl_body_i"]), np.asarray(A["shapes"]), np.asarray(A["body_tmpl"])

    def reach(sr):
        s = [float(v) for v in sr]
        t = int(s[0])
        ext = {N.MG_SHAPE_SPHERE: s[1], N.MG_SHAPE_BOX: math.sqrt(s[1] * s[1] + s[2] * s[2] + s[3] * s[3]),
               N.MG_SHAPE_CAPSULE: s[1] + s[2], N.MG_SHAPE_CONVEX: s[1]}.get(t, 0.0)
        return math.sqrt(s[4] * s[4] + s[5] * s[5] + s[6] * s[6]) + ext

    nb = len(tmpl)
    r = np.full(nb, -1.0)
    for b in range(nb):
        s0, ns = tbi[tmpl[b], 0], tbi[tmpl[b], 1]
        for s in range(s0, s0 + ns):
            r[b] = max(r[b], reach(shapes[s]))
    k = np.zeros(nb, np.float32)
    for bodies in actor_bodies(A):
        most = max(0.0, max(r[b] for b in bodies))
        for b in bodies:
            rb = r[b] if r[b] >= 0.0 else most
            k[b] = np.float32(4.0 * rb * rb)
    return k


# ---------------------------------------------------------------- the rule
class SleepRef:
    """oracle.step followed by the sleep pass, frame by frame, with the wakes of
    the sets. State: st [nb, 13], ds [nd, 2] (global order, as the tensors)."""

    def __init__(self, sim, threshold=THRESHOLD, window=WINDOW, on=True):
        A = sim.model_arrays if sim.finalized else sim.build_model()
        self.A = A
        self.p, self.m = sim.mg_params(), sim.mg_model()
        self.st, self.ds, self.props = A["body_state0"].copy(), A["dof_state0"].copy(), A["dof_props"]
        self.roots = np.asarray(A["actor_root_body"])
        bodies, adof = actor_bodies(A), np.asarray(A["actor_dof"])
        self.isl = islands(A)
        self.isl_bodies = [np.concatenate([bodies[a] for a in acts]) for acts in self.isl]
        self.isl_dofs = [np.concatenate([np.arange(adof[a], adof[a + 1]) for a in acts]).astype(int) for acts in self.isl]
        self.actor_island = np.full(len(self.roots), -1)
        for i, acts in enumerate(self.isl):
            self.actor_island[acts] = i
        self.body_island = np.full(len(self.st), -1)
        for i, b in enumerate(self.isl_bodies):
            self.body_island[b] = i
        self.k = body_k(A)
        self.on = on
        # the host's part, in double, from the float32 values the library is handed
        thr, win = float(np.float32(threshold)), float(np.float32(window))
        self.W = max(1, int(math.floor(win / float(np.float32(self.p.dt)) + 0.5)))
        tol = win * math.sqrt(2.0 * thr)
        self.tol2 = np.float32(tol * tol)
        n = len(self.isl)
        self.timer = np.zeros(n, int)
        self.fresh = np.ones(n, bool)      # no anchor taken yet
        self.asleep = np.zeros(n, bool)
        self.anchor = np.zeros((len(self.st), 7), np.float32)
        self.dof_q = np.zeros(len(self.ds), np.float32)
        self.cforce = None

    # ---- wakes
    def wake(self, actors=None):
        isl = range(len(self.isl)) if actors is None else [self.actor_island[a] for a in np.atleast_1d(actors)]
        for i in isl:
            if i >= 0:
                self.asleep[i] = False
                self.timer[i] = 0

    def set_root(self, actors, rows):
        """An indexed root set: the actors' root rows, and their islands wake."""
        self.st[self.roots[np.atleast_1d(actors)]] = rows
        self.wake(actors)

    # ---- a frame
    def step(self, tgt=None, ext=None, tgt_set=False):
        """tgt: the DOF targets in force [nd, 3]; tgt_set: a full target set was
        made this frame (wakes all); ext [nb, 6]: applied this frame (wakes the
        islands of its non-zero rows)."""
        if tgt_set:
            self.wake()
        if ext is not None:
            for i in set(self.body_island[np.any(np.asarray(ext) != 0, axis=1)].tolist()) - {-1}:
                self.asleep[i] = False
                self.timer[i] = 0
        self.cforce = oracle.step(self.p, self.m, self.st, self.ds, tgt=tgt, props=self.props, ext=ext)
        if self.on:
            self.sleep_pass()

    def moved(self, b):
        st, an = self.st, self.anchor
        d = st[b, 0:3] - an[b, 0:3]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        c = ((st[b, 3] * an[b, 3] + st[b, 4] * an[b, 4]) + st[b, 5] * an[b, 5]) + st[b, 6] * an[b, 6]
        s2 = np.float32(1.0) - c * c
        return (d2 > self.tol2) | (self.k[b] * s2 > self.tol2)

    def sleep_pass(self):
        st, ds = self.st, self.ds
        for i, (b, d) in enumerate(zip(self.isl_bodies, self.isl_dofs)):
            if self.asleep[i]:
                st[b, 0:7] = self.anchor[b]
                st[b, 7:13] = 0.0
                ds[d, 0] = self.dof_q[d]
                ds[d, 1] = 0.0
            elif self.fresh[i] or self.moved(b).any():
                self.anchor[b] = st[b, 0:7]
                self.timer[i] = 0
                self.fresh[i] = False
            else:
                self.timer[i] += 1
                if self.timer[i] >= self.W:
                    self.asleep[i] = True
                    self.anchor[b] = st[b, 0:7]
                    self.dof_q[d] = ds[d, 0]
                    st[b, 7:13] = 0.0
                    ds[d, 1] = 0.0

    def sleeping_actors(self):
        out = np.zeros(len(self.roots), bool)
        ok = self.actor_island >= 0
        out[ok] = self.asleep[self.actor_island[ok]]
        return out
