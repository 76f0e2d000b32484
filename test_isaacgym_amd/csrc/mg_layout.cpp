// mg_layout.cpp — the host-only layout planner (mg_layout.h): validates a model
// and derives its storage order, launch groups and index tables. Pure integer
// and float logic on host vectors; mg_upload_model commits the result to the
// device.
#include "mg_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>

namespace {

using Row = std::vector<int>;

// tables the steps hand on to each other, in global body ids until `perm` exists
struct Work {
    std::string* err;
    std::vector<char> coupled_body;   // free roots / articulation roots of coupled envs
    std::vector<Row> env_rows;        // [..][env_i_n]
    std::vector<int> env_tmpl;
    std::vector<Row> pile_rows;       // [..][pile_i_n]
    // envs built alike (the same shapes, filters and order) share one slot table
    // and pair list: 4096 pyramids read one 2 KB list through L2
    std::map<std::pair<std::vector<int>, std::vector<unsigned>>, std::pair<int, int>> pile_list_at;
    std::vector<int> artic_of_root;
    std::vector<char> placed;
};

int fail(Work& w, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(Work& w, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *w.err = buf;
    return code;
}

// free-free pair (i, j), i < j, of a coupled env -> its bit of the collision mask (from bit 8)
const int pair_bit[4][4] = {{-1, 0, 1, 2}, {-1, -1, 3, 4}, {-1, -1, -1, 5}, {-1, -1, -1, -1}};

void shape_range(const mg_model* m, int b, int* s0, int* ns) {
    const int* t = m->tmpl_body_i + (size_t)m->body_tmpl[b] * MG_TBODY_I_N;
    *s0 = t[0];
    *ns = t[1];
}

// the actor_coll rule (migym.h): may actors a and b touch?
bool collide(const mg_model* m, int a, int b) {
    const int ga = m->actor_coll[(size_t)a * MG_ACOLL_N + 1], gb = m->actor_coll[(size_t)b * MG_ACOLL_N + 1];
    const int fa = m->actor_coll[(size_t)a * MG_ACOLL_N + 2], fb = m->actor_coll[(size_t)b * MG_ACOLL_N + 2];
    return (ga == gb || ga == -1 || gb == -1) && (fa & fb) == 0;
}

// instances that step in k_artic_chain (one lane per articulation) are laid out
// link-major in blocks of 64
bool blocked(const MgArticGroup& g) { return g.chain && g.nl >= 2 && g.nl <= 4; }

// Shape-frame box of a shape (the coupled step's pair screen, mg_env.hip
// obb_apart; oracle: shape_obb_): centre and half extents; a hull's from the
// min / max of its vertices
void shape_obb(const float* sh, const float* hulls, float* o, int obb_n) {
    const int t = (int)sh[0];
    for (int k = 0; k < obb_n; ++k) o[k] = 0.0f;
    if (t == MG_SHAPE_CONVEX && hulls) {
        const float* hv = hulls + (int)sh[2];
        const int nv = (int)hv[0];
        float lo[3], hi[3];
        for (int c = 0; c < 3; ++c) { lo[c] = hv[MG_HULL_HEADER + c]; hi[c] = lo[c]; }
        for (int i = 1; i < nv; ++i)
            for (int c = 0; c < 3; ++c) {
                const float v = hv[MG_HULL_HEADER + 3 * i + c];
                lo[c] = std::min(lo[c], v);
                hi[c] = std::max(hi[c], v);
            }
        for (int c = 0; c < 3; ++c) {
            o[c] = 0.5f * (lo[c] + hi[c]);
            o[3 + c] = 0.5f * (hi[c] - lo[c]);
        }
    } else if (t == MG_SHAPE_BOX) {
        o[3] = sh[1]; o[4] = sh[2]; o[5] = sh[3];
    } else if (t == MG_SHAPE_CAPSULE) {
        o[3] = sh[1] + sh[2]; o[4] = sh[1]; o[5] = sh[1];
    } else {
        o[3] = sh[1]; o[4] = sh[1]; o[5] = sh[1];
    }
}

// ---- step 1: validate indices on the host before anything reaches a kernel
int validate(const mg_model* m, MgLayout& L, Work& w) {
    if (m->num_bodies < 0 || m->num_actors < 0 || m->num_dofs < 0) return fail(w, MG_ERR_ARG, "negative sizes");
    const int nb = m->num_bodies, na = m->num_actors, nd = m->num_dofs;
    L.nenv = m->num_envs; L.na = na; L.nb = nb; L.nd = nd;
    L.ntb = m->num_tmpl_bodies; L.ns = m->num_shapes;
    L.nartic = m->num_artics; L.ntl = m->num_tmpl_links;
    L.nhull_floats = m->hulls ? m->num_hull_floats : 0;
    for (int b = 0; b < nb; ++b) {
        const int t = m->body_tmpl[b];
        if (t < 0 || t >= L.ntb) return fail(w, MG_ERR_ARG, "body %d: template %d out of range", b, t);
        const int s0 = m->tmpl_body_i[t * MG_TBODY_I_N + 0], sc = m->tmpl_body_i[t * MG_TBODY_I_N + 1];
        if (s0 < 0 || sc < 0 || s0 + sc > L.ns) return fail(w, MG_ERR_ARG, "template body %d: bad shape range", t);
    }
    for (int k = 0; k < L.ns; ++k) {
        const float* sh = m->shapes + (size_t)k * MG_SHAPE_STRIDE;
        const int t = (int)sh[0];
        if (t < MG_SHAPE_SPHERE || t > MG_SHAPE_CONVEX) return fail(w, MG_ERR_ARG, "shape %d: unknown type %d", k, t);
        if (t != MG_SHAPE_CONVEX) continue;
        const long off = (long)sh[2], nh = m->hulls ? m->num_hull_floats : 0;
        if (off < 0 || off + MG_HULL_HEADER > nh) return fail(w, MG_ERR_ARG, "shape %d: hull offset %ld out of range", k, off);
        const int nv = (int)m->hulls[off], nfc = (int)m->hulls[off + 1], ned = (int)m->hulls[off + 2];
        if (nv < 4 || nv > MG_HULL_MAX_VERTS || nfc < 4 || nfc > MG_HULL_MAX_FACES || ned < 0 ||
            ned > 3 * MG_HULL_MAX_VERTS || off + MG_HULL_HEADER + 3L * nv + 4L * nfc + 2L * ned > nh)
            return fail(w, MG_ERR_ARG, "shape %d: bad hull record (%d vertices, %d faces, %d edges)", k, nv, nfc, ned);
        for (int e = 0; e < 2 * ned; ++e) {
            const float vi = m->hulls[off + MG_HULL_HEADER + 3L * nv + 4L * nfc + e];
            if (!(vi >= 0.0f && vi < (float)nv)) return fail(w, MG_ERR_ARG, "shape %d: hull edge vertex out of range", k);
        }
    }
    for (int a = 0; a < na; ++a) {
        if (m->actor_root_body[a] < 0 || m->actor_root_body[a] >= nb) return fail(w, MG_ERR_ARG, "actor %d: bad root", a);
        if (m->actor_dof[a] > m->actor_dof[a + 1]) return fail(w, MG_ERR_ARG, "actor_dof not monotone");
        L.max_actor_dofs = std::max(L.max_actor_dofs, m->actor_dof[a + 1] - m->actor_dof[a]);
    }
    if (na > 0 && (m->actor_dof[0] != 0 || m->actor_dof[na] != nd)) return fail(w, MG_ERR_ARG, "actor_dof must span [0, num_dofs]");
    return MG_OK;
}

// ---- step 2: classify envs. Envs where two bodies may touch (actor_coll rule,
// see migym.h) step in the per-env kernel (plan_coupled_env) or, without an
// articulation and with more than env_maxf free bodies, as a pile
// (plan_pile_env); everything else in the free-body / articulation kernels

// a pile (mg_pile.hip): lane k = free body k; pairs per free
// body k and shape of k: the ground, the static bodies it may touch, the later
// free bodies it may touch
int plan_pile_env(const mg_model* m, const MgLayoutSizes& z, bool ground, int e, const std::vector<int>& fr,
                  const std::vector<int>& stc, MgLayout& L, Work& w) {
    if ((int)fr.size() > z.pile_maxb || (int)stc.size() > z.env_maxs)
        return fail(w, MG_ERR_UNSUPPORTED,
                    "env %d: %zu free / %zu static bodies in contact range; a pile env supports %d / %d",
                    e, fr.size(), stc.size(), z.pile_maxb, z.env_maxs);
    Row row(z.pile_i_n, 0);
    row[0] = (int)L.pile_body.size();
    row[1] = (int)fr.size();
    row[4] = (int)stc.size();
    for (size_t t = 0; t < stc.size(); ++t) row[5 + t] = m->actor_root_body[stc[t]];
    for (int f : fr) {
        L.pile_body.push_back(m->actor_root_body[f]);
        w.coupled_body[m->actor_root_body[f]] = 1;
    }
    // local shape slots: the free bodies' shapes in body order, then the statics'
    std::vector<int> slots;
    std::vector<int> first_slot(fr.size() + stc.size());
    for (size_t k = 0; k < fr.size() + stc.size(); ++k) {
        const bool st = k >= fr.size();
        int sb0, nsb;
        shape_range(m, m->actor_root_body[st ? stc[k - fr.size()] : fr[k]], &sb0, &nsb);
        first_slot[k] = (int)slots.size() / 2;
        for (int sb = sb0; sb < sb0 + nsb; ++sb) {
            slots.push_back(st ? z.pile_st0 + (int)(k - fr.size()) : (int)k);
            slots.push_back(sb);
        }
    }
    if ((int)slots.size() / 2 > z.pile_maxsh)
        return fail(w, MG_ERR_UNSUPPORTED, "env %d: %zu collision shapes; a pile env supports %d", e,
                    slots.size() / 2, z.pile_maxsh);
    std::vector<unsigned> plist;
    for (int k = 0; k < (int)fr.size(); ++k) {
        int sa0, nsa;
        shape_range(m, m->actor_root_body[fr[k]], &sa0, &nsa);
        for (int sa = sa0; sa < sa0 + nsa; ++sa) {
            const unsigned la = (unsigned)(first_slot[k] + (sa - sa0));
            auto push = [&](int owner, int sb, int sb0) {
                plist.push_back(la | (unsigned)(first_slot[owner] + (sb - sb0)) << 8);
            };
            if (ground) plist.push_back(la | (unsigned)z.pile_ground << 8);
            for (int t = 0; t < (int)stc.size(); ++t) {
                if (!collide(m, fr[k], stc[t])) continue;
                int sb0, nsb;
                shape_range(m, m->actor_root_body[stc[t]], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push((int)fr.size() + t, sb, sb0);
            }
            for (int j = k + 1; j < (int)fr.size(); ++j) {
                if (!collide(m, fr[k], fr[j])) continue;
                int sb0, nsb;
                shape_range(m, m->actor_root_body[fr[j]], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(j, sb, sb0);
            }
        }
    }
    row[3] = (int)plist.size();
    row[10] = (int)slots.size() / 2;
    if (row[3] > z.pile_maxpairs)
        return fail(w, MG_ERR_UNSUPPORTED, "env %d: %d candidate shape pairs; a pile env supports %d", e,
                    row[3], z.pile_maxpairs);
    auto key = std::make_pair(slots, plist);
    auto it = w.pile_list_at.find(key);
    if (it != w.pile_list_at.end()) {
        row[2] = it->second.first;
        row[9] = it->second.second;
    } else {
        row[2] = (int)L.pile_pairs.size();
        row[9] = (int)L.pile_slots.size() / 2;
        w.pile_list_at.emplace(std::move(key), std::make_pair(row[2], row[9]));
        L.pile_pairs.insert(L.pile_pairs.end(), plist.begin(), plist.end());
        L.pile_slots.insert(L.pile_slots.end(), slots.begin(), slots.end());
    }
    w.pile_rows.push_back(row);
    L.pile_env.push_back(e);
    return MG_OK;
}

// a coupled env's row (mg_internal.h MgEnvArgs) and its candidate shape pairs
int plan_coupled_env(const mg_model* m, const MgLayoutSizes& z, bool ground, int e, const std::vector<int>& art,
                     const std::vector<int>& fr, const std::vector<int>& stc, MgLayout& L, Work& w) {
    if (art.size() > 1 || (int)fr.size() > z.env_maxf || (int)stc.size() > z.env_maxs)
        return fail(w, MG_ERR_UNSUPPORTED,
                    "env %d: %zu articulations / %zu free / %zu static bodies in contact range; the "
                    "coupled step supports 1 / %d / %d", e, art.size(), fr.size(), stc.size(),
                    z.env_maxf, z.env_maxs);
    int art_nl = 0, art_nd = 0, art_fb = 0, art_fl = 0;
    if (!art.empty()) {
        const int k = w.artic_of_root[m->actor_root_body[art[0]]];
        const int t = k >= 0 ? m->artic_i[(size_t)k * MG_ARTIC_I_N + 2] : -1;
        if (t < 0 || t >= m->num_artic_tmpls) return fail(w, MG_ERR_ARG, "env %d: bad articulation", e);
        art_nl = m->artic_tmpl_i[t * MG_ATMPL_I_N + 1];
        art_nd = m->artic_tmpl_i[t * MG_ATMPL_I_N + 2];
        art_fb = m->artic_tmpl_i[t * MG_ATMPL_I_N + 3] ? 0 : 1;
        const int fl = m->artic_tmpl_i[t * MG_ATMPL_I_N + 0];
        if (fl < 0 || art_nl < 1 || fl + art_nl > m->num_tmpl_links)
            return fail(w, MG_ERR_ARG, "env %d: bad articulation template %d", e, t);
        art_fl = fl;
    }
    if (art_nd + 6 * art_fb + 6 * (int)fr.size() > z.env_slots_wide || art_nl > z.max_links)
        return fail(w, MG_ERR_UNSUPPORTED, "env %d: %d links, %d DOFs%s + %zu free bodies exceed the %d links / %d "
                    "velocity slots of the coupled step", e, art_nl, art_nd, art_fb ? " + a floating base" : "",
                    fr.size(), z.max_links, z.env_slots_wide);
    Row row(z.env_i_n, 0);
    row[0] = -1;
    int tmpl = -1;
    if (!art.empty()) {
        const int r0 = m->actor_root_body[art[0]];
        const int k = w.artic_of_root[r0];
        if (k < 0) return fail(w, MG_ERR_ARG, "env %d: articulated actor without articulation record", e);
        row[0] = r0;
        row[1] = m->artic_i[(size_t)k * MG_ARTIC_I_N + 1];
        tmpl = m->artic_i[(size_t)k * MG_ARTIC_I_N + 2];
        w.coupled_body[r0] = 1;
    }
    row[2] = (int)fr.size();
    for (size_t i = 0; i < fr.size(); ++i) {
        row[3 + i] = m->actor_root_body[fr[i]];
        w.coupled_body[row[3 + i]] = 1;
    }
    row[7] = (int)stc.size();
    for (size_t i = 0; i < stc.size(); ++i) row[8 + i] = m->actor_root_body[stc[i]];
    int mask = 0;
    for (size_t i = 0; i < fr.size(); ++i) {
        if (!art.empty() && collide(m, art[0], fr[i])) mask |= 1 << i;
        for (size_t j = i + 1; j < fr.size(); ++j)
            if (collide(m, fr[i], fr[j])) mask |= 1 << (8 + pair_bit[i][j]);
        for (size_t t = 0; t < stc.size(); ++t)
            if (collide(m, fr[i], stc[t])) mask |= 1 << (14 + 4 * i + t);
    }
    for (size_t t = 0; t < stc.size(); ++t)
        if (!art.empty() && collide(m, art[0], stc[t])) mask |= 1 << (4 + t);
    row[12] = mask;
    row[13] = tmpl;
    // candidate shape pairs, in the order the step solves them
    std::vector<int>& pairs = L.pairs;
    auto push = [&pairs](int a, int sa, int b, int sb) {
        pairs.push_back(a); pairs.push_back(sa); pairs.push_back(b); pairs.push_back(sb);
    };
    row[14] = (int)(pairs.size() / 4);
    for (int k = 0; k < (int)fr.size(); ++k) {
        int sa0, nsa;
        shape_range(m, row[3 + k], &sa0, &nsa);
        for (int sa = sa0; sa < sa0 + nsa; ++sa) {
            if (ground) push(z.env_free0 + k, sa, -1, -1);
            for (int t = 0; t < (int)stc.size(); ++t) {
                if (!((mask >> (14 + 4 * k + t)) & 1)) continue;
                int sb0, nsb;
                shape_range(m, row[8 + t], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(z.env_free0 + k, sa, z.env_static0 + t, sb);
            }
            for (int j = k + 1; j < (int)fr.size(); ++j) {
                if (!((mask >> (8 + pair_bit[k][j])) & 1)) continue;
                int sb0, nsb;
                shape_range(m, row[3 + j], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(z.env_free0 + k, sa, z.env_free0 + j, sb);
            }
            if (row[0] >= 0 && !art_fb && ((mask >> k) & 1)) {   // the fixed base (static)
                int sb0, nsb;
                shape_range(m, row[0], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(z.env_free0 + k, sa, 0, sb);
            }
        }
    }
    for (int l = art_fb ? 0 : 1; l < art_nl; ++l) {     // moving links (a floating base moves)
        // the link's body (virtual links of ball / multi-axis joints: none)
        const int bl = m->tmpl_link_i[(size_t)(art_fl + l) * MG_LINK_I_N + 3];
        if (bl < 0) continue;
        int sa0, nsa;
        shape_range(m, row[0] + bl, &sa0, &nsa);
        for (int sa = sa0; sa < sa0 + nsa; ++sa) {
            if (ground) push(l, sa, -1, -1);
            for (int t = 0; t < (int)stc.size(); ++t) {
                if (!((mask >> (4 + t)) & 1)) continue;
                int sb0, nsb;
                shape_range(m, row[8 + t], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(l, sa, z.env_static0 + t, sb);
            }
            for (int k = 0; k < (int)fr.size(); ++k) {
                if (!((mask >> k) & 1)) continue;
                int sb0, nsb;
                shape_range(m, row[3 + k], &sb0, &nsb);
                for (int sb = sb0; sb < sb0 + nsb; ++sb) push(l, sa, z.env_free0 + k, sb);
            }
        }
    }
    row[15] = (int)(pairs.size() / 4) - row[14];
    w.env_rows.push_back(row);
    L.cenv_env.push_back(e);
    w.env_tmpl.push_back(tmpl);
    return MG_OK;
}

int classify_envs(const mg_sim_params& p, const mg_model* m, const MgLayoutSizes& z, MgLayout& L, Work& w) {
    const int nb = L.nb, na = L.na;
    w.coupled_body.assign(nb, 0);
    if (!(m->actor_coll && na > 0)) return MG_OK;
    for (int a = 0; a + 1 < na; ++a)
        if (m->actor_root_body[a + 1] <= m->actor_root_body[a])
            return fail(w, MG_ERR_ARG, "actor_coll needs actors in body order");
    w.artic_of_root.assign(nb, -1);
    for (int k = 0; k < m->num_artics; ++k) {
        const int r0 = m->artic_i[(size_t)k * MG_ARTIC_I_N + 0];
        if (r0 < 0 || r0 >= nb) return fail(w, MG_ERR_ARG, "articulation %d: bad first body", k);
        w.artic_of_root[r0] = k;
    }
    const int ne = m->num_envs;
    std::vector<std::vector<int>> env_actors(ne > 0 ? ne : 0);
    for (int a = 0; a < na; ++a) {
        const int e = m->actor_coll[(size_t)a * MG_ACOLL_N + 0];
        if (e < 0 || e >= ne) return fail(w, MG_ERR_ARG, "actor %d: env %d out of range", a, e);
        env_actors[e].push_back(a);
    }
    const bool ground = p.has_ground != 0;
    for (int e = 0; e < ne; ++e) {
        std::vector<int> art, fr, stc;
        for (int a : env_actors[e]) {
            const int r0 = m->actor_root_body[a];
            const int kind = m->body_kind[r0];
            if (kind == MG_BODY_LINK) art.push_back(a);
            else if (kind == MG_BODY_FREE) fr.push_back(a);
            else stc.push_back(a);
        }
        bool coupled = false;
        for (size_t i = 0; i < fr.size(); ++i) {
            for (int t : stc) coupled = coupled || collide(m, fr[i], t);
            for (size_t j = i + 1; j < fr.size(); ++j) coupled = coupled || collide(m, fr[i], fr[j]);
        }
        for (int a : art) {
            for (int t : stc) coupled = coupled || collide(m, a, t);
            for (int f : fr) coupled = coupled || collide(m, a, f);
            // a floating-base articulation always steps here (ground contacts,
            // the root's own dynamics)
            const int k = w.artic_of_root[m->actor_root_body[a]];
            if (k >= 0 && !m->artic_tmpl_i[m->artic_i[(size_t)k * MG_ARTIC_I_N + 2] * MG_ATMPL_I_N + 3])
                coupled = true;
        }
        if (!coupled) continue;
        const int rc = art.empty() && (int)fr.size() > z.env_maxf ? plan_pile_env(m, z, ground, e, fr, stc, L, w)
                                                                   : plan_coupled_env(m, z, ground, e, art, fr, stc, L, w);
        if (rc) return rc;
    }
    return MG_OK;
}

// ---- step 3: order bodies. Free bodies ordered by template body (stable):
// bodies of one kind share waves, so e.g. the servo scene's airborne UAVs and
// grounded vehicles do not interleave lane by lane (results do not depend on
// the order). Templates whose instances start farthest from the ground plane
// come first: a launch larger than one resident round dispatches the array back
// to front (mg_launch_rigid_step), i.e. the likely-in-contact (long) waves
// first and the airborne (short) ones last, filling the last round's tail.
// Free bodies of coupled envs come last (the per-env kernel reads them).
void order_free_bodies(const mg_sim_params& p, const mg_model* m, MgLayout& L, Work& w) {
    const int nb = L.nb;
    std::vector<int> free_ids, free_cpl;
    for (int b = 0; b < nb; ++b)
        if (m->body_kind[b] == MG_BODY_FREE) (w.coupled_body[b] ? free_cpl : free_ids).push_back(b);
    auto nshapes = [m](int b) { return m->tmpl_body_i[m->body_tmpl[b] * MG_TBODY_I_N + 1]; };
    std::vector<double> clear_sum(m->num_tmpl_bodies, 0.0);
    std::vector<int> clear_n(m->num_tmpl_bodies, 0);
    {
        float gn[3] = {0.0f, 0.0f, 0.0f};
        float gd = 0.0f;
        if (p.has_ground) {
            for (int k = 0; k < 3; ++k) gn[k] = p.ground_normal[k];
            gd = p.ground_distance;
        } else {
            gn[p.up_axis == 0 ? 1 : 2] = 1.0f;
        }
        for (int b : free_ids) {
            const float* x = m->body_state0 + (size_t)b * MG_STATE_N;
            clear_sum[m->body_tmpl[b]] += (double)gn[0] * x[0] + (double)gn[1] * x[1] + (double)gn[2] * x[2] + gd;
            clear_n[m->body_tmpl[b]] += 1;
        }
    }
    auto clearance = [&](int t) { return clear_n[t] ? clear_sum[t] / clear_n[t] : 0.0; };
    std::stable_sort(free_ids.begin(), free_ids.end(), [&](int a, int b) {
        const bool ma = nshapes(a) > 1, mb = nshapes(b) > 1;   // single-shape bodies first
        if (ma != mb) return !ma;
        const int ta = m->body_tmpl[a], tb = m->body_tmpl[b];
        if (ta == tb) return false;
        const double ca = clearance(ta), cb = clearance(tb);
        if (ca != cb) return ca > cb;
        return ta < tb;
    });
    L.nf1 = 0;
    for (int b : free_ids) L.nf1 += nshapes(b) <= 1 ? 1 : 0;
    L.nf_rigid = (int)free_ids.size();
    free_ids.insert(free_ids.end(), free_cpl.begin(), free_cpl.end());
    L.nf = (int)free_ids.size();
    // internal storage order: free bodies (as above), articulation links
    // (instance by instance, template by template), everything else
    L.order = free_ids;
    w.placed.assign(nb, 0);
    for (int b : free_ids) w.placed[b] = 1;
}

// the stepped instances' link mass rows and gravity flags agree (k_artic_chain's
// shared constants, mg_chainlink.h; set once: mass properties are fixed after upload)
bool chain_mass_uniform(const mg_model* m, const MgArticGroup& g) {
    const int b0 = g.step_body0[0];
    bool ok = true;
    const float grav = m->tmpl_body_f[(size_t)m->body_tmpl[b0] * MG_TBODY_F_N + 4];
    for (size_t i = 1; i < g.step_body0.size() && ok; ++i) {
        const int bi = g.step_body0[i];
        ok = m->tmpl_body_f[(size_t)m->body_tmpl[bi] * MG_TBODY_F_N + 4] == grav;
        for (int l = 1; l < g.nl && ok; ++l)
            ok = std::memcmp(m->body_mass + (size_t)(bi + l) * MG_MASS_N, m->body_mass + (size_t)(b0 + l) * MG_MASS_N,
                             MG_MASS_N * sizeof(float)) == 0;
    }
    return ok;
}

// articulation template t's group header, checked
int artic_template(const mg_model* m, const MgLayoutSizes& z, int t, const MgLayout& L, MgArticGroup& g, Work& w) {
    g.tmpl = t;
    g.first_link = m->artic_tmpl_i[t * MG_ATMPL_I_N + 0];
    g.nl = m->artic_tmpl_i[t * MG_ATMPL_I_N + 1];
    g.ndof = m->artic_tmpl_i[t * MG_ATMPL_I_N + 2];
    g.fixed_base = m->artic_tmpl_i[t * MG_ATMPL_I_N + 3];
    if (g.nl < 1 || g.nl > z.max_links || g.ndof > g.nl || g.ndof > z.max_dofs || g.first_link < 0 ||
        g.first_link + g.nl > L.ntl)
        return fail(w, MG_ERR_UNSUPPORTED, "articulation template %d: %d links / %d dofs unsupported", t, g.nl, g.ndof);
    g.nbody = 0;
    for (int l = 0; l < g.nl; ++l) {
        const int* li = m->tmpl_link_i + (size_t)(g.first_link + l) * MG_LINK_I_N;
        if (li[0] >= l || (l > 0 && li[0] < 0) || (l == 0 && li[0] != -1))
            return fail(w, MG_ERR_ARG, "articulation template %d: links not in topological order", t);
        if (li[2] >= g.ndof) return fail(w, MG_ERR_ARG, "articulation template %d: bad dof index", t);
        // real links carry bodies 0, 1, 2, ... in link order; virtual links
        // (the first two of a ball joint) are revolute with a DOF and no body
        if (li[3] >= 0) {
            if (li[3] != g.nbody) return fail(w, MG_ERR_ARG, "articulation template %d: link bodies out of order", t);
            g.nbody++;
        } else if (l == 0 || li[1] != MG_JOINT_REVOLUTE || li[2] < 0) {
            return fail(w, MG_ERR_ARG, "articulation template %d: bad virtual link %d", t, l);
        }
    }
    g.chain = g.fixed_base && g.ndof == g.nl - 1 && g.nbody == g.nl;
    for (int l = 1; l < g.nl && g.chain; ++l) {
        const int* li = m->tmpl_link_i + (size_t)(g.first_link + l) * MG_LINK_I_N;
        g.chain = li[0] == l - 1 && li[2] == l - 1 && (li[1] == MG_JOINT_REVOLUTE || li[1] == MG_JOINT_PRISMATIC);
    }
    return MG_OK;
}

// articulation instances grouped by template
int order_artic_groups(const mg_model* m, const MgLayoutSizes& z, MgLayout& L, Work& w) {
    const int nb = L.nb, nd = L.nd;
    std::vector<int>&artic_sorted = L.artic_sorted, &artic_step = L.artic_step, &order = L.order;
    L.body_class.assign(nb, ATTR_NONE);
    L.body_grp.assign(nb, -1);
    L.body_inst.assign(nb, -1);
    L.body_artic.assign(nb, -1);
    L.link_i.assign(m->tmpl_link_i, m->tmpl_link_i + (size_t)L.ntl * MG_LINK_I_N);
    L.atmpl.assign(m->artic_tmpl_i, m->artic_tmpl_i + (size_t)m->num_artic_tmpls * MG_ATMPL_I_N);
    for (int t = 0; t < m->num_artic_tmpls; ++t) {
        MgArticGroup g;
        if (int rc = artic_template(m, z, t, L, g, w)) return rc;
        g.offset = (int)artic_sorted.size() / MG_ARTIC_I_N;
        g.count = 0;
        g.step_offset = (int)artic_step.size() / MG_ARTIC_I_N;
        g.step_count = 0;
        // Link stride (row field 3): link l of an instance is body first + l * stride.
        // Instances that step in k_artic_chain (one lane per articulation) are laid
        // out link-major in blocks of 64, the kernel's wavefront: link l of the
        // block's instances are 64 consecutive slots, so every per-link load and
        // store of a wave is one contiguous 256-B access (link-contiguous storage
        // strides the lanes nl * 4 B apart). Everything else: stride 1.
        std::vector<int> blk_k, blk_sorted, blk_step;
        for (int k = 0; k < m->num_artics; ++k) {
            const int* ai = m->artic_i + (size_t)k * MG_ARTIC_I_N;
            if (ai[2] != t) continue;
            if (ai[0] < 0 || ai[0] + g.nbody > nb || ai[1] < 0 || ai[1] + g.ndof > nd)
                return fail(w, MG_ERR_ARG, "articulation %d out of range", k);
            const bool cpl = w.coupled_body[ai[0]] != 0;
            const bool blk = blocked(g) && !cpl;
            for (int l = 0; l < g.nbody; ++l) L.body_artic[ai[0] + l] = (int)L.artic_info.size();
            L.artic_info.push_back({ai[0], ai[1], t, cpl ? 1 : 0});
            if (blk) {
                blk_k.push_back(k);
                blk_sorted.push_back((int)artic_sorted.size());
                blk_step.push_back((int)artic_step.size());
            }
            for (int j = 0; j < MG_ARTIC_I_N; ++j) artic_sorted.push_back(j == 3 ? 1 : ai[j]);
            if (!cpl) {
                for (int j = 0; j < MG_ARTIC_I_N; ++j) artic_step.push_back(j == 3 ? 1 : ai[j]);
                g.step_count++;
                g.step_body0.push_back(ai[0]);
                g.step_dof0.push_back(ai[1]);
            }
            for (int l = 0; l < g.nbody; ++l) {
                if (w.placed[ai[0] + l]) return fail(w, MG_ERR_ARG, "articulation %d overlaps another body", k);
                w.placed[ai[0] + l] = 1;
                if (!blk) order.push_back(ai[0] + l);
                L.body_class[ai[0] + l] = cpl ? ATTR_ENV_LINK : ATTR_LINK;
                if (!cpl) {
                    L.body_grp[ai[0] + l] = (int)L.groups.size();
                    L.body_inst[ai[0] + l] = g.step_count - 1;
                }
            }
            g.count++;
        }
        for (size_t i0 = 0; i0 < blk_k.size(); i0 += 64) {
            const int cnt = (int)std::min<size_t>(64, blk_k.size() - i0);
            for (int l = 0; l < g.nbody; ++l)
                for (int j = 0; j < cnt; ++j) order.push_back(m->artic_i[(size_t)blk_k[i0 + j] * MG_ARTIC_I_N] + l);
            for (int j = 0; j < cnt; ++j) {
                artic_sorted[blk_sorted[i0 + j] + 3] = cnt;
                artic_step[blk_step[i0 + j] + 3] = cnt;
            }
        }
        if (!g.fixed_base && g.step_count > 0)
            return fail(w, MG_ERR_UNSUPPORTED, "articulation template %d: a floating base steps in the coupled "
                        "per-env kernel, which needs actor_coll", t);
        if (blocked(g) && g.step_count > 0) g.uni_mass = chain_mass_uniform(m, g);
        L.groups.push_back(g);
    }
    return MG_OK;
}

// the rest of the order, `perm`, and the chain groups whose stepped rows follow
// the blocked layout from one base slot and one DOF stride: the kernel
// computes them (MgArticArgs::aff)
void finish_order(MgLayout& L, const Work& w) {
    const int nb = L.nb;
    std::vector<int>&artic_sorted = L.artic_sorted, &artic_step = L.artic_step, &order = L.order, &perm = L.perm;
    perm.assign(nb, -1);
    for (int b = 0; b < nb; ++b)
        if (!w.placed[b]) order.push_back(b);
    for (int i = 0; i < nb; ++i) perm[order[i]] = i;
    for (size_t k = 0; k < artic_sorted.size(); k += MG_ARTIC_I_N) artic_sorted[k] = perm[artic_sorted[k]];
    for (size_t k = 0; k < artic_step.size(); k += MG_ARTIC_I_N) artic_step[k] = perm[artic_step[k]];
    for (MgArticGroup& g : L.groups) {
        g.aff = 0;
        if (!blocked(g) || g.step_count == 0) continue;
        const int* r0 = artic_step.data() + (size_t)g.step_offset * MG_ARTIC_I_N;
        const int B = r0[0], D = r0[1];
        const int DS = g.step_count > 1 ? r0[MG_ARTIC_I_N + 1] - D : 0;
        bool ok = true;
        for (int k = 0; k < g.step_count && ok; ++k) {
            const int* r = r0 + (size_t)k * MG_ARTIC_I_N;
            const int blk = k / 64, j = k % 64, cnt = std::min(64, g.step_count - blk * 64);
            ok = r[0] == B + blk * 64 * g.nbody + j && r[3] == cnt && r[1] == D + k * DS;
        }
        if (ok) { g.aff = 1; g.aff_b0 = B; g.aff_d0 = D; g.aff_ds = DS; }
    }
}

// ---- step 4: coupled env rows: internal slots, grouped by articulation
// template (-1 first) (and by lane width: an env of more than 16 links or
// velocity slots runs 64 lanes wide, mg_env.hip; the oracle decides per env the
// same way); the pile tables in internal slots; the free bodies' classes
void plan_env_groups(const mg_model* m, const MgLayoutSizes& z, MgLayout& L, Work& w) {
    const int nb = L.nb;
    const std::vector<int>& perm = L.perm;
    std::vector<Row>& env_rows = w.env_rows;
    std::vector<int>& env_flat = L.env_flat;
    L.cenv_ctab_off.assign(env_rows.size(), -1);
    L.cenv_ctab_n.assign(env_rows.size(), 0);
    L.cenv_row.assign(env_rows.size(), 0);
    for (int t = -1; t < m->num_artic_tmpls; ++t)
    for (int wide = 0; wide < 2; ++wide) {
        MgEnvGroup g{};
        g.tmpl = t;
        g.wide = wide;
        if (t >= 0) {
            g.first_link = m->artic_tmpl_i[t * MG_ATMPL_I_N + 0];
            g.nl = m->artic_tmpl_i[t * MG_ATMPL_I_N + 1];
            g.ndof = m->artic_tmpl_i[t * MG_ATMPL_I_N + 2];
            g.floating = m->artic_tmpl_i[t * MG_ATMPL_I_N + 3] ? 0 : 1;
        }
        g.offset = (int)env_flat.size() / z.env_i_n;
        for (size_t r = 0; r < env_rows.size(); ++r) {
            if (w.env_tmpl[r] != t) continue;
            const int slots = (t >= 0 ? g.ndof + 6 * g.floating : 0) + 6 * env_rows[r][2];
            if ((g.nl > 16 || slots > 16) != (wide != 0)) continue;
            Row row = env_rows[r];
            g.max_free = std::max(g.max_free, row[2]);
            if (row[0] >= 0) row[0] = perm[row[0]];
            for (int i = 0; i < row[2]; ++i) row[3 + i] = perm[row[3 + i]];
            for (int i = 0; i < row[7]; ++i) row[8 + i] = perm[row[8 + i]];
            env_flat.insert(env_flat.end(), row.begin(), row.end());
            // k_env_np writes env j of the group at the group's base + j records
            L.cenv_ctab_off[r] = (long long)g.offset * z.env_ctab_floats +
                                 (long long)g.count * z.env_ctab_record_floats[wide];
            L.cenv_ctab_n[r] = z.env_ctab_record_floats[wide];
            L.cenv_row[r] = g.offset + g.count;
            g.count++;
        }
        if (g.count > 0) L.env_groups.push_back(g);
    }
    L.n_coupled = (int)env_rows.size();
    L.env_d0.assign(env_rows.size(), 0);
    for (size_t r = 0; r < env_rows.size(); ++r) L.env_d0[r] = env_flat[r * z.env_i_n + 1];
    L.n_pile = (int)w.pile_rows.size();
    for (Row& r : w.pile_rows) {
        for (int t = 0; t < r[4]; ++t) r[5 + t] = perm[r[5 + t]];
        L.pile_rows.insert(L.pile_rows.end(), r.begin(), r.end());
    }
    for (int& b : L.pile_body) b = perm[b];
    for (int b = 0; b < nb; ++b)
        if (m->body_kind[b] == MG_BODY_FREE && perm[b] < L.nf)
            L.body_class[b] = perm[b] < L.nf_rigid ? ATTR_FREE : ATTR_ENV_FREE;
    for (int slot : L.pile_body) L.body_class[L.order[slot]] = ATTR_PILE;
}

// ---- step 5: per-slot tables and the template records

// compact template records of the single-shape kernel: template floats, then
// the first shape record (type -1: no shape)
void plan_trec(const mg_model* m, const MgLayoutSizes& z, MgLayout& L) {
    const int nb = L.nb;
    std::vector<float>& trec = L.trec;
    trec.assign((size_t)L.ntb * z.trec_n, 0.0f);
    for (int t = 0; t < L.ntb; ++t) {
        float* r = &trec[(size_t)t * z.trec_n];
        std::memcpy(r, m->tmpl_body_f + (size_t)t * MG_TBODY_F_N, MG_TBODY_F_N * sizeof(float));
        const int s0 = m->tmpl_body_i[t * MG_TBODY_I_N + 0], sc = m->tmpl_body_i[t * MG_TBODY_I_N + 1];
        if (sc > 0) {
            const float* sr = m->shapes + (size_t)s0 * MG_SHAPE_STRIDE;
            std::memcpy(r + MG_TBODY_F_N, sr, MG_SHAPE_STRIDE * sizeof(float));
            // pad[0] of the copy: bounding radius of the shape about the body
            // origin (k_rigid_step1 skips the candidates of a wave whose bodies
            // all clear the ground by more than it); -1: unknown, never skipped
            double ext = -1.0;
            switch ((int)sr[0]) {
                case MG_SHAPE_SPHERE: ext = sr[1]; break;
                case MG_SHAPE_BOX: ext = std::sqrt((double)sr[1] * sr[1] + (double)sr[2] * sr[2] + (double)sr[3] * sr[3]); break;
                case MG_SHAPE_CAPSULE: ext = (double)sr[1] + sr[2]; break;
                case MG_SHAPE_CONVEX: ext = sr[1]; break;
                default: break;
            }
            const double po = std::sqrt((double)sr[4] * sr[4] + (double)sr[5] * sr[5] + (double)sr[6] * sr[6]);
            r[MG_TBODY_F_N + 13] = (ext >= 0.0 && std::isfinite(ext + po)) ? (float)((ext + po) * (1.0 + 1e-6)) : -1.0f;
        } else {
            r[MG_TBODY_F_N] = -1.0f;
        }
    }
    // one mass row per template when all its free bodies share it (the kernel
    // then reads it from the record instead of 44 B per body)
    std::vector<int> seen(L.ntb, 0), uniform(L.ntb, 1);
    for (int b = 0; b < nb; ++b) {
        if (m->body_kind[b] != MG_BODY_FREE) continue;
        const int t = m->body_tmpl[b];
        const float* mr = m->body_mass + (size_t)b * MG_MASS_N;
        float* r = &trec[(size_t)t * z.trec_n];
        if (!seen[t]) {
            std::memcpy(r + z.trec_mass, mr, MG_MASS_N * sizeof(float));
            seen[t] = 1;
        } else if (std::memcmp(r + z.trec_mass, mr, MG_MASS_N * sizeof(float)) != 0) {
            uniform[t] = 0;
        }
    }
    for (int t = 0; t < L.ntb; ++t) trec[(size_t)t * z.trec_n + 5] = seen[t] && uniform[t] ? 1.0f : 0.0f;
    L.shape_obb.assign((size_t)std::max(L.ns, 1) * z.obb_n, 0.0f);
    for (int k = 0; k < L.ns; ++k)
        shape_obb(m->shapes + (size_t)k * MG_SHAPE_STRIDE, m->hulls, &L.shape_obb[(size_t)k * z.obb_n], z.obb_n);
}

void plan_slot_tables(const mg_model* m, MgLayout& L) {
    const int nb = L.nb, na = L.na;
    const std::vector<int>&order = L.order, &perm = L.perm, &artic_step = L.artic_step;
    std::vector<int>&root_int = L.root_int, &tmpl_int = L.tmpl_int, &slot_actor = L.slot_actor;
    root_int.resize(na);
    tmpl_int.resize(nb);
    for (int a = 0; a < na; ++a) root_int[a] = perm[m->actor_root_body[a]];
    for (int i = 0; i < nb; ++i) tmpl_int[i] = m->body_tmpl[order[i]];
    L.state0.resize((size_t)nb * MG_STATE_N);
    L.mass0.resize((size_t)nb * MG_MASS_N);
    for (int i = 0; i < nb; ++i) {
        for (int f = 0; f < MG_STATE_N; ++f) L.state0[(size_t)f * nb + i] = m->body_state0[(size_t)order[i] * MG_STATE_N + f];
        for (int f = 0; f < MG_MASS_N; ++f) L.mass0[(size_t)f * nb + i] = m->body_mass[(size_t)order[i] * MG_MASS_N + f];
    }
    L.body_actor.assign(nb, -1);
    for (int a = 0; a < na; ++a) L.body_actor[m->actor_root_body[a]] = a;
    // the per-slot indices of the free-body step packed into one record per slot
    // (the same values as root_row, tmpl_int, order, slot_actor)
    L.slot_rec.assign((size_t)std::max(nb, 1), {-1, 0, 0, -1});
    {
        // fusable root sets: every actor root is a single-shape free body of the
        // free-body kernel (internal slots 0..nf1-1), and that kernel steps all
        // free bodies (no multi-shape ones, no articulations, no coupled envs)
        std::vector<int>& row = L.root_row;
        row.assign(nb, -1);
        bool ok = L.nf1 == L.nf_rigid && L.nf_rigid == L.nf && L.nartic == 0 && L.n_coupled == 0 &&
                  L.n_pile == 0 && na > 0;
        for (int a = 0; a < na && ok; ++a) {
            const int slot = root_int[a];
            ok = slot >= 0 && slot < L.nf1 && row[slot] < 0;
            if (ok) row[slot] = a;
        }
        L.roots_free = ok;
        for (int i = 0; i < nb; ++i) L.slot_rec[i][0] = row[i];
    }
    // rows the step kernels write with the refresh fused into them
    // (MG_FUSE_STEP_OUT): internal slot -> rigid-body row / actor row
    slot_actor.assign(nb, -1);
    for (int a = 0; a < na; ++a) slot_actor[root_int[a]] = a;
    // the env of each actor root's slot (the contact list's env column)
    L.slot_env.assign((size_t)std::max(nb, 1), 0);
    if (m->actor_coll)
        for (int a = 0; a < na; ++a) L.slot_env[root_int[a]] = m->actor_coll[(size_t)a * MG_ACOLL_N + 0];
    for (int i = 0; i < nb; ++i) {
        L.slot_rec[i][1] = tmpl_int[i];
        L.slot_rec[i][2] = order[i];
        L.slot_rec[i][3] = slot_actor[i];
    }
    // chain groups whose fused-refresh rows are affine in the instance
    for (MgArticGroup& g : L.groups) {
        g.out_aff = 0;
        if (!g.aff) continue;
        const int* r0 = artic_step.data() + (size_t)g.step_offset * MG_ARTIC_I_N;
        const int G0 = order[r0[0]], A0 = slot_actor[r0[0]];
        bool ok = A0 >= 0;
        for (int k = 0; k < g.step_count && ok; ++k) {
            const int* r = r0 + (size_t)k * MG_ARTIC_I_N;
            ok = slot_actor[r[0]] == A0 + k;
            for (int l = 0; l < g.nl && ok; ++l) ok = order[r[0] + l * r[3]] == G0 + k * g.nl + l;
        }
        if (ok) { g.out_aff = 1; g.out_g0 = G0; g.out_r0 = A0; }
    }
    long long covered = L.nf1 == L.nf_rigid && L.nf_rigid == L.nf ? L.nf1 : -1;
    for (const MgArticGroup& g : L.groups) {
        if (covered < 0) break;
        if (g.count == 0) continue;
        if (!blocked(g) || g.step_count != g.count) covered = -1;
        else covered += (long long)g.step_count * g.nbody;
    }
    L.step_out_ok = L.n_coupled == 0 && L.n_pile == 0 && nb > 0 && covered == nb;
    L.actor_dof.assign(m->actor_dof, m->actor_dof + (na > 0 ? na + 1 : 0));
    L.body_tmpl.assign(m->body_tmpl, m->body_tmpl + nb);
    L.tbi.assign(m->tmpl_body_i, m->tmpl_body_i + (size_t)L.ntb * MG_TBODY_I_N);
}

// Facts about the single-shape free bodies that pick the free-body kernel's
// build (MgLayout::free_flags). [0], box_only: every such body's shape is a box
// at the body origin with the body's orientation, or absent.
void plan_free_flags(const MgLayoutSizes& z, MgLayout& L) {
    // shape records as plan_trec copied them: type at [0] (< 0: none), the
    // shape's position at [4..6], its rotation (x, y, z, w) at [7..10]
    bool box_only = true;
    for (int i = 0; i < L.nf1 && box_only; ++i) {
        const float* sh = &L.trec[(size_t)L.slot_rec[i][1] * z.trec_n + MG_TBODY_F_N];
        if (sh[0] < 0.0f) continue;
        box_only = (int)sh[0] == MG_SHAPE_BOX && sh[4] == 0.0f && sh[5] == 0.0f && sh[6] == 0.0f && sh[7] == 0.0f &&
                   sh[8] == 0.0f && sh[9] == 0.0f && sh[10] == 1.0f;
    }
    L.free_flags.assign(1, box_only ? 1 : 0);
}

// ---- step 6: sleeping islands

// a shape's reach about its body's origin, |p_s| + extent_s (the extents of plan_trec)
double shape_reach(const float* sr) {
    double ext = 0.0;
    switch ((int)sr[0]) {
        case MG_SHAPE_SPHERE: ext = sr[1]; break;
        case MG_SHAPE_BOX: ext = std::sqrt((double)sr[1] * sr[1] + (double)sr[2] * sr[2] + (double)sr[3] * sr[3]); break;
        case MG_SHAPE_CAPSULE: ext = (double)sr[1] + sr[2]; break;
        case MG_SHAPE_CONVEX: ext = sr[1]; break;
        default: break;
    }
    return std::sqrt((double)sr[4] * sr[4] + (double)sr[5] * sr[5] + (double)sr[6] * sr[6]) + ext;
}

void plan_islands(const mg_model* m, MgLayout& L, const Work& w) {
    const int nb = L.nb, na = L.na;
    // the bodies of each actor (global ids first .. first + count - 1)
    std::vector<int> first(na), count(na, 1);
    for (int a = 0; a < na; ++a) {
        first[a] = m->actor_root_body[a];
        const int k = L.body_artic[first[a]];
        if (k >= 0) {
            first[a] = L.artic_info[k].g0;
            count[a] = L.groups[L.artic_info[k].tmpl].nbody;
        }
    }
    // bounding radii
    std::vector<double> reach(nb, -1.0);
    for (int b = 0; b < nb; ++b) {
        int s0, ns;
        shape_range(m, b, &s0, &ns);
        for (int s = s0; s < s0 + ns; ++s)
            reach[b] = std::max(reach[b], shape_reach(m->shapes + (size_t)s * MG_SHAPE_STRIDE));
    }
    L.body_k.assign(nb, 0.0f);
    for (int a = 0; a < na; ++a) {
        double most = 0.0;
        for (int b = first[a]; b < first[a] + count[a]; ++b) most = std::max(most, reach[b]);
        for (int b = first[a]; b < first[a] + count[a]; ++b) {
            const double r = reach[b] >= 0.0 ? reach[b] : most;
            L.body_k[L.perm[b]] = std::isfinite(r) ? (float)(4.0 * r * r) : 0.0f;
        }
    }
    // the islands as their actors, in actor order: one per coupled or pile env, one per other moving actor
    std::vector<std::vector<int>> members;
    std::map<int, int> of_env;
    for (int a = 0; a < na; ++a) {
        const int r0 = m->actor_root_body[a];
        if (m->body_kind[r0] == MG_BODY_STATIC) continue;
        if (w.coupled_body[r0]) {
            const int e = m->actor_coll[(size_t)a * MG_ACOLL_N + 0];
            auto it = of_env.find(e);
            if (it == of_env.end()) {
                it = of_env.emplace(e, (int)members.size()).first;
                members.emplace_back();
            }
            members[it->second].push_back(a);
        } else {
            members.push_back({a});
        }
    }
    struct Isl { int cls, slot0; std::vector<int> slots, dofs; const std::vector<int>* actors; };
    std::vector<Isl> isl(members.size());
    for (size_t i = 0; i < members.size(); ++i) {
        Isl& I = isl[i];
        I.actors = &members[i];
        for (int a : members[i]) {
            for (int b = first[a]; b < first[a] + count[a]; ++b) I.slots.push_back(L.perm[b]);
            for (int d = m->actor_dof[a]; d < m->actor_dof[a + 1]; ++d) I.dofs.push_back(d);
        }
        std::sort(I.slots.begin(), I.slots.end());
        I.slot0 = I.slots[0];
        I.cls = I.slots.size() == 1 ? 0 : I.slots.size() <= 16 ? 1 : 2;
    }
    std::sort(isl.begin(), isl.end(), [](const Isl& x, const Isl& y) { return x.cls != y.cls ? x.cls < y.cls : x.slot0 < y.slot0; });
    L.n_island = (int)isl.size();
    L.body_island.assign(nb, -1);
    L.actor_island.assign(na, -1);
    L.island_body0.assign(1, 0);
    L.island_dof0.assign(1, 0);
    for (int c = 0; c < 4; ++c) L.island_class0[c] = L.n_island;
    for (int i = 0; i < L.n_island; ++i) {
        const Isl& I = isl[i];
        for (int c = 0; c <= I.cls; ++c) L.island_class0[c] = std::min(L.island_class0[c], i);
        for (int s : I.slots) L.body_island[s] = i;
        for (int a : *I.actors) L.actor_island[a] = i;
        L.island_body.insert(L.island_body.end(), I.slots.begin(), I.slots.end());
        L.island_dof.insert(L.island_dof.end(), I.dofs.begin(), I.dofs.end());
        L.island_body0.push_back((int)L.island_body.size());
        L.island_dof0.push_back((int)L.island_dof.size());
    }
}

}  // namespace

int mg_plan_layout(const mg_sim_params& p, const mg_model& model, const MgLayoutSizes& z, MgLayout& L, std::string& err) {
    const mg_model* m = &model;
    L = MgLayout();
    Work w;
    w.err = &err;
    if (int rc = validate(m, L, w)) return rc;
    if (int rc = classify_envs(p, m, z, L, w)) return rc;
    order_free_bodies(p, m, L, w);
    if (int rc = order_artic_groups(m, z, L, w)) return rc;
    finish_order(L, w);
    plan_env_groups(m, z, L, w);
    plan_trec(m, z, L);
    plan_slot_tables(m, L);
    plan_free_flags(z, L);
    plan_islands(m, L, w);
    return MG_OK;
}
