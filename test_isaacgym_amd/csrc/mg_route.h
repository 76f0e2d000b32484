// mg_route.h — the routing plan of the step features: which launches a simulate
// issues, which instances each covers, which optional features each carries, and which feature
// combinations are refused. Plain C++17: no HIP, no device header (tests/step_route_check.cpp
// includes it alone). mg_plan_route is a pure function of the layout plan and the current feature
// tables: the attractor table, the force sensor table, contact reporting on or off, the DOF
// property table (friction is field 9) and the count of DOFs that report forces. Every call that
// changes one of them plans a fresh MgRoute from all of them and commits it with its device
// buffers (migym_capi.cpp); mg_simulate reports the route's refusal, then walks its launches.
//
// Of MgLayout it reads: nb, nd, nf1, nf_rigid, n_pile, step_out_ok; perm; artic_step; groups (chain, uni_mass,
// nl, ndof, fixed_base, aff, out_aff, step_offset, step_count); env_groups (tmpl, nl, ndof, floating,
// max_free, offset, count); trec, slot_rec, free_flags (their sizes, free_flags[0]); body_class, body_grp,
// body_inst, body_artic, artic_info, env_d0, actor_dof, atmpl, link_i.
//
// The next feature: one RT_* bit, one routing term in mg_plan_route (which launches get the bit),
// one term in its family's chooser in mg_forms.h (which build carries it, which pointer that build
// needs), and one entry in the alphabet of tests/step_route_check.cpp. Which kernel and form a
// launch runs is not written here: mg_route_builds asks the chooser, for the refusals below and
// for mg_simulate alike.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "mg_forms.h"
#include "mg_layout.h"

// a launch's features: attractors, DOF force rows, contact moments (force sensors), contact
// reporting, joint friction (k_env_step's form bits, by value)
enum : unsigned { RT_ATTR = EF_ATTR, RT_FRC = EF_FRC, RT_SENS = EF_SENS, RT_CREP = EF_CREP, RT_JFR = EF_JFR };
// articulation group (k_artic_chain / k_artic_lanes), coupled env group (k_env_step), pile envs, free bodies
enum MgFamily { MG_FAM_ARTIC, MG_FAM_ENV, MG_FAM_PILE, MG_FAM_FREE };

struct MgLaunch {
    int family, group;   // group: of MgLayout::groups / env_groups (0: pile, free bodies)
    // ARTIC: rows of MgRoute::split when `split`, else of artic_step (rows computed where the
    // group allows: aff, out_aff); ENV: rows of env_flat; PILE, FREE: all of them
    int row0, count;
    unsigned feat;       // RT_*
    bool split;
    bool operator==(const MgLaunch& o) const {
        return std::tie(family, group, row0, count, feat, split) == std::tie(o.family, o.group, o.row0, o.count, o.feat, o.split);
    }
};

// the force sensor tables' columns (mg_internal.h's MG_SENS_I_*, MG_SENS_F_N, MG_SART_I_N: migym_capi.cpp asserts them equal)
enum { RS_G0, RS_LINK0, RS_LINK, RS_MASK, RS_FLAGS, RS_ART, RS_OUT, RS_HIST, RS_OWNER, RS_I_N, RS_F_N = 7, RS_ART_N = 4 };

struct MgRouteIn {
    const mg_attractor* attrs = nullptr;
    int n_attr = 0;
    const mg_force_sensor* sensors = nullptr;
    int n_sens = 0;
    bool crep = false;
    const float* dof_props = nullptr;   // [nd][MG_DOFPROP_N] global DOF order; null: no DOF has friction
    int dof_frc_n = 0;
    bool sleep = false;                 // sleeping is on (mg_set_sleeping): k_sleep_pass rewrites rows after the step
};

struct MgRoute {
    std::vector<MgLaunch> launches;   // in launch order: articulation groups, coupled groups, piles, free bodies
    // One split table for every articulation group, or empty when no stepped instance is an
    // owner. Group g's rows step_offset .. hold its plain instances, then those that hold a
    // friction DOF, then those that own an attractor, each in stepped order.
    std::vector<int> split;           // [step rows][MG_ARTIC_I_N]
    std::vector<int> attr_idx;        // [max(nb, 1)] internal slot -> attractor record, -1: none
    // A table this build cannot honour is refused by mg_simulate, never ignored: the first of an
    // attractor on a body class that cannot carry one, the sensor refusal, a launch whose
    // features have no build. mg_refresh_force_sensor reports the sensor one.
    int refusal = MG_OK;
    std::string refusal_msg, sens_refusal;
    // the inputs' echo: attractors, contact reporting, DOFs that report forces
    int n_attr = 0, dof_frc_n = 0;
    bool crep = false;
    // the step may write its rows itself (the fused refresh, the host stage): every kernel that
    // steps a body writes its rows, none is an attractor, reporting or joint-friction build, and
    // no sleep pass follows the step (it restores the rows of sleeping islands)
    bool step_writes_rows = false;
    // mg_joint_friction_stats: friction DOFs, instances in the lanes friction launches, envs of coupled friction groups
    int jfr_ndof = 0, jfr_lanes = 0, jfr_envs = 0;
    // the force sensor tables' host form (MgSensorArgs): lanes in sensor slot (its place among
    // its articulation's sensors) major, articulation minor, templates apart
    int n_sens = 0, n_sart = 0, sens_nhb = 0, sens_nsave = 0;
    std::vector<int> si, sart, hist0;   // [RS_I_N][n_sens], [n_sart][RS_ART_N], [n_sart]
    std::vector<float> sf;              // [RS_F_N][n_sens]

    bool operator==(const MgRoute& o) const {
        return launches == o.launches && split == o.split && attr_idx == o.attr_idx && refusal == o.refusal &&
               refusal_msg == o.refusal_msg && sens_refusal == o.sens_refusal &&
               std::tie(n_attr, dof_frc_n, crep, step_writes_rows, jfr_ndof, jfr_lanes, jfr_envs, n_sens, n_sart, sens_nhb, sens_nsave) ==
                   std::tie(o.n_attr, o.dof_frc_n, o.crep, o.step_writes_rows, o.jfr_ndof, o.jfr_lanes, o.jfr_envs, o.n_sens, o.n_sart,
                            o.sens_nhb, o.sens_nsave) &&
               si == o.si && sart == o.sart && hist0 == o.hist0 && sf == o.sf;
    }
    // the same kernels over the same instances: what a captured graph replays (mg_set_dof_props)
    bool same_launches(const MgRoute& o) const { return launches == o.launches && split == o.split; }
};

inline int mg_route_msg(std::string& out, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int mg_route_msg(std::string& out, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    out = buf;
    return code;
}

// The build(s) launch `l` runs under `run`: the group's shape out of the layout, handed to its
// family's chooser (mg_forms.h). The free bodies' launch has up to two, every other one `one`.
inline MgBuilds mg_route_builds(const MgLayout& L, const MgLaunch& l, const MgRun& run) {
    MgBuilds b;
    if (l.family == MG_FAM_ARTIC) {
        const MgArticGroup& g = L.groups[l.group];
        b.one = mg_choose_artic(g.nl, g.ndof, g.fixed_base, g.chain, g.uni_mass, g.aff, g.out_aff, l.split, l.count, l.feat, run);
    } else if (l.family == MG_FAM_ENV) {
        const MgEnvGroup& g = L.env_groups[l.group];
        const bool art = g.tmpl >= 0;
        b.one = mg_choose_env(art ? g.nl : 0, art ? g.ndof : 0, art && g.floating, g.max_free, l.feat, run);
    } else if (l.family == MG_FAM_PILE) {
        b.one = mg_choose_pile(l.feat, run);
    } else {
        b = mg_choose_free(L.nf1, L.nf_rigid, L.trec.size() * sizeof(float), !L.slot_rec.empty(),
                           !L.free_flags.empty() && L.free_flags[0], l.feat, run);
    }
    return b;
}

// Every MgRun a simulate can form for `l`, in turn: both ground bases, a wrench pending or not,
// refreshed rows written or not, and a device on each side of k_rigid_step1's wide threshold for
// the launch's blocks (0 CUs: every launch is wide; one CU per block: none is). fn(run) -> false stops.
template <class Fn>
inline bool mg_route_each_run(const MgLayout& L, const MgLaunch& l, Fn&& fn) {
    const int blocks = l.family == MG_FAM_FREE ? (L.nf1 + 63) / 64 : 0;
    for (int m = 0; m < 16; ++m)
        if (!fn(MgRun{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0, m & 8 ? blocks : 0})) return false;
    return true;
}

// Plans the route. Returns MG_OK, or a table's validation error with its message in `err` (then
// `R` is unspecified). A refusal is no error: it is part of the route.
inline int mg_plan_route(const MgLayout& L, const MgRouteIn& in, MgRoute& R, std::string& err) {
    R = MgRoute();
    R.n_attr = in.n_attr;
    R.crep = in.crep;
    R.dof_frc_n = in.dof_frc_n;
    const size_t ntmpl = L.atmpl.size() / MG_ATMPL_I_N;
    std::string attr_refusal, launch_refusal;
    // per stepped instance of each articulation group: RT_ATTR (owns an attractor) | RT_JFR (holds a friction DOF)
    std::vector<std::vector<unsigned char>> owner(L.groups.size());
    for (size_t gi = 0; gi < L.groups.size(); ++gi) owner[gi].assign((size_t)L.groups[gi].step_count, 0);

    // ---- attractors: the table, then what steps each body
    R.attr_idx.assign((size_t)std::max(L.nb, 1), -1);
    for (int i = 0; i < in.n_attr; ++i) {
        const mg_attractor& a = in.attrs[i];
        if (a.body < 0 || a.body >= L.nb) return mg_route_msg(err, MG_ERR_ARG, "attractor %d: body %d out of range", i, a.body);
        if (!(std::isfinite(a.stiffness) && a.stiffness >= 0.0f && std::isfinite(a.damping) && a.damping >= 0.0f))
            return mg_route_msg(err, MG_ERR_ARG, "attractor %d: stiffness and damping must be finite and non-negative", i);
        bool fin = true;
        for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(a.offset_p[k]) && std::isfinite(a.target_p[k]);
        for (int k = 0; k < 4; ++k) fin = fin && std::isfinite(a.offset_q[k]) && std::isfinite(a.target_q[k]);
        if (!fin) return mg_route_msg(err, MG_ERR_ARG, "attractor %d: offset and target must be finite", i);
        int& rec = R.attr_idx[L.perm[a.body]];
        if (rec >= 0)
            return mg_route_msg(err, MG_ERR_UNSUPPORTED, "attractor %d: body %d already owns attractor %d (one attractor per body)",
                                i, a.body, rec);
        rec = i;
    }
    bool attr_free = false, attr_env = false, attr_link = false;
    std::vector<char> tmpl_attr(ntmpl, 0);   // templates whose coupled instances own an attractor
    for (int i = 0; i < in.n_attr; ++i) {
        const int b = in.attrs[i].body;
        const char* why = nullptr;
        switch (L.body_class[b]) {
            case ATTR_FREE: attr_free = true; break;
            case ATTR_ENV_LINK: attr_env = true; tmpl_attr[L.artic_info[L.body_artic[b]].tmpl] = 1; break;
            case ATTR_LINK: attr_link = true; owner[L.body_grp[b]][L.body_inst[b]] |= RT_ATTR; break;
            case ATTR_ENV_FREE: why = "a free body of a coupled env"; break;
            case ATTR_PILE: why = "a body of a pile env"; break;
            default: why = "not a dynamic body"; break;
        }
        if (why && attr_refusal.empty())
            mg_route_msg(attr_refusal, 0, "attractor %d on rigid body %d: %s cannot carry an attractor in this build", i, b, why);
    }

    // ---- force sensors: the table, the refusal, the kernels' tables
    for (int i = 0; i < in.n_sens; ++i) {
        const mg_force_sensor& f = in.sensors[i];
        if (f.body < 0 || f.body >= L.nb) return mg_route_msg(err, MG_ERR_ARG, "force sensor %d: body %d out of range", i, f.body);
        bool fin = true;
        float q2 = 0.0f;
        for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(f.p[k]);
        for (int k = 0; k < 4; ++k) { fin = fin && std::isfinite(f.q[k]); q2 += f.q[k] * f.q[k]; }
        if (!fin || !(q2 > 0.0f))
            return mg_route_msg(err, MG_ERR_ARG, "force sensor %d: the local pose must be finite, its rotation not zero", i);
        if (L.body_artic[f.body] < 0 && R.sens_refusal.empty())
            mg_route_msg(R.sens_refusal, 0, "force sensor %d on rigid body %d: a single-body actor has no joint to measure "
                         "(and the free-body and pile kernels keep no contact moment); force sensors sit on bodies of "
                         "articulations", i, f.body);
    }
    struct Lane { int tmpl, slot, art, row; };
    std::vector<Lane> lanes;
    std::vector<int> art_slot(L.artic_info.size(), 0), art_id(L.artic_info.size(), -1);
    std::vector<char> tmpl_sens(ntmpl, 0);   // templates whose coupled instances carry a sensor
    if (R.sens_refusal.empty())
        for (int i = 0; i < in.n_sens; ++i) {
            const int a = L.body_artic[in.sensors[i].body];
            const MgArticInfo& ai = L.artic_info[a];
            if (art_id[a] < 0) {
                art_id[a] = (int)R.hist0.size();
                const int ndof = L.atmpl[ai.tmpl * MG_ATMPL_I_N + 2];
                const int nl = L.atmpl[ai.tmpl * MG_ATMPL_I_N + 1], l0 = L.atmpl[ai.tmpl * MG_ATMPL_I_N + 0];
                int nbody = 0;
                for (int l = 0; l < nl; ++l) nbody += L.link_i[(size_t)(l0 + l) * MG_LINK_I_N + 3] >= 0 ? 1 : 0;
                const int row[RS_ART_N] = {L.perm[ai.g0], ai.d0, ndof, R.sens_nsave};
                R.sart.insert(R.sart.end(), row, row + RS_ART_N);
                R.hist0.push_back(R.sens_nhb);
                R.sens_nhb += nbody;
                R.sens_nsave += MG_STATE_N + 2 * ndof;
                if (ai.coupled) tmpl_sens[ai.tmpl] = 1;
            }
            lanes.push_back({ai.tmpl, art_slot[a]++, art_id[a], i});
        }
    std::stable_sort(lanes.begin(), lanes.end(), [](const Lane& x, const Lane& y) {
        return x.tmpl != y.tmpl ? x.tmpl < y.tmpl : (x.slot != y.slot ? x.slot < y.slot : x.art < y.art);
    });
    const int nl_ = (int)lanes.size();
    R.n_sens = nl_;
    R.n_sart = (int)R.hist0.size();
    R.si.assign((size_t)RS_I_N * std::max(nl_, 1), 0);
    R.sf.assign((size_t)RS_F_N * std::max(nl_, 1), 0.0f);
    for (int t = 0; t < nl_; ++t) {
        const Lane& ln = lanes[t];
        const mg_force_sensor& f = in.sensors[ln.row];
        const MgArticInfo& ai = L.artic_info[L.body_artic[f.body]];
        const int l0 = L.atmpl[ai.tmpl * MG_ATMPL_I_N + 0], nl = L.atmpl[ai.tmpl * MG_ATMPL_I_N + 1];
        // the sensor body's link, and its subtree (links in topological order:
        // a link joins when its parent is in)
        int ls = -1;
        for (int l = 0; l < nl; ++l)
            if (L.link_i[(size_t)(l0 + l) * MG_LINK_I_N + 3] == f.body - ai.g0) ls = l;
        if (ls < 0) return mg_route_msg(err, MG_ERR_ARG, "force sensor %d: body %d is no link of its articulation", ln.row, f.body);
        unsigned mask = 1u << ls;
        for (int l = ls + 1; l < nl; ++l) {
            const int p = L.link_i[(size_t)(l0 + l) * MG_LINK_I_N + 0];
            if (p >= 0 && ((mask >> p) & 1u)) mask |= 1u << l;
        }
        R.si[(size_t)RS_G0 * nl_ + t] = ai.g0;
        R.si[(size_t)RS_LINK0 * nl_ + t] = l0;
        R.si[(size_t)RS_LINK * nl_ + t] = ls;
        R.si[(size_t)RS_MASK * nl_ + t] = (int)mask;
        R.si[(size_t)RS_FLAGS * nl_ + t] = f.flags & (MG_SENSOR_FORWARD | MG_SENSOR_CONSTRAINT | MG_SENSOR_WORLD);
        R.si[(size_t)RS_ART * nl_ + t] = ln.art;
        R.si[(size_t)RS_OUT * nl_ + t] = ln.row;
        R.si[(size_t)RS_HIST * nl_ + t] = R.hist0[ln.art];
        R.si[(size_t)RS_OWNER * nl_ + t] = ln.slot == 0 ? 1 : 0;
        const float qn = 1.0f / std::sqrt(f.q[0] * f.q[0] + f.q[1] * f.q[1] + f.q[2] * f.q[2] + f.q[3] * f.q[3]);
        for (int k = 0; k < 3; ++k) R.sf[(size_t)k * nl_ + t] = f.p[k];
        for (int k = 0; k < 4; ++k) R.sf[(size_t)(3 + k) * nl_ + t] = f.q[k] * qn;
    }

    // ---- joint friction: the table; the uncoupled instances and the coupled groups that hold a DOF with friction > 0
    for (int d = 0; in.dof_props && d < L.nd; ++d) {
        const float f = in.dof_props[(size_t)d * MG_DOFPROP_N + 9];
        if (!(std::isfinite(f) && f >= 0.0f))
            return mg_route_msg(err, MG_ERR_ARG, "DOF %d: friction %g must be finite and non-negative", d, (double)f);
        if (f > 0.0f) R.jfr_ndof++;
    }
    auto fric_dof = [&](int d0, int n) {
        for (int j = 0; j < n; ++j)
            if (in.dof_props[(size_t)(d0 + j) * MG_DOFPROP_N + 9] > 0.0f) return d0 + j;
        return -1;
    };
    auto actor_of = [&](int d) { return (int)(std::upper_bound(L.actor_dof.begin(), L.actor_dof.end(), d) - L.actor_dof.begin()) - 1; };
    // the actor of a group's first friction DOF, for a refusal's message
    std::vector<int> artic_jactor(L.groups.size(), -1), env_jactor(L.env_groups.size(), -1);
    for (size_t gi = 0; R.jfr_ndof > 0 && gi < L.groups.size(); ++gi) {
        const MgArticGroup& g = L.groups[gi];
        for (int k = 0; k < g.step_count; ++k) {
            const int d = fric_dof(L.artic_step[(size_t)(g.step_offset + k) * MG_ARTIC_I_N + 1], g.ndof);
            if (d < 0) continue;
            owner[gi][k] |= RT_JFR;
            R.jfr_lanes++;
            if (artic_jactor[gi] < 0) artic_jactor[gi] = actor_of(d);
        }
    }
    for (size_t gi = 0; R.jfr_ndof > 0 && gi < L.env_groups.size(); ++gi) {
        const MgEnvGroup& g = L.env_groups[gi];
        for (int r = g.offset; g.tmpl >= 0 && r < g.offset + g.count && env_jactor[gi] < 0; ++r) {
            const int d = fric_dof(L.env_d0[r], g.ndof);
            if (d >= 0) env_jactor[gi] = actor_of(d);
        }
        if (env_jactor[gi] >= 0) R.jfr_envs += g.count;
    }

    // ---- the launches. DOF force rows: while the sim reports DOF forces, and by every
    // contact-moment, reporting and joint-friction build (the refresh masks the other rows)
    const unsigned frc = in.dof_frc_n > 0 ? RT_FRC : 0;
    auto with_frc = [&](unsigned f) { return f | (f & (RT_SENS | RT_CREP | RT_JFR) ? RT_FRC : frc); };
    if (attr_link || R.jfr_lanes > 0) R.split.resize(L.artic_step.size());
    for (size_t gi = 0; gi < L.groups.size(); ++gi) {
        const MgArticGroup& g = L.groups[gi];
        // Owners step apart, in k_artic_lanes' joint-friction and attractor-aware builds. Both
        // owner launches of a group carry the kinds of all its owners: a group with owners of
        // both kinds is refused as a whole, as it always was.
        unsigned kinds = 0;
        for (unsigned char o : owner[gi]) kinds |= o;
        int row = g.step_offset;
        for (int pass = 0; pass < 3; ++pass) {   // plain, friction owners, attractor owners
            const int row0 = row;
            for (int k = 0; k < g.step_count; ++k) {
                const unsigned o = owner[gi][k];
                if ((pass == 0 ? o == 0 : pass == 1 ? (o & RT_JFR) != 0 : o == RT_ATTR) && !R.split.empty())
                    std::memcpy(&R.split[(size_t)row * MG_ARTIC_I_N], &L.artic_step[(size_t)(g.step_offset + k) * MG_ARTIC_I_N],
                                MG_ARTIC_I_N * sizeof(int));
                if (pass == 0 ? o == 0 : pass == 1 ? (o & RT_JFR) != 0 : o == RT_ATTR) row++;
            }
            if (row > row0) R.launches.push_back({MG_FAM_ARTIC, (int)gi, row0, row - row0, with_frc(pass ? kinds : 0), kinds != 0});
        }
    }
    for (size_t gi = 0; gi < L.env_groups.size(); ++gi) {
        const MgEnvGroup& g = L.env_groups[gi];
        const bool jfr = env_jactor[gi] >= 0;
        // every group without friction gets the attractor build as soon as any coupled link owns
        // an attractor; a friction group only for an attractor of its own (and is then refused)
        const bool attr = attr_env && (!jfr || (g.tmpl >= 0 && tmpl_attr[g.tmpl]));
        const bool sens = g.tmpl >= 0 && tmpl_sens[g.tmpl];
        R.launches.push_back({MG_FAM_ENV, (int)gi, g.offset, g.count,
                              with_frc((attr ? RT_ATTR : 0) | (sens ? RT_SENS : 0) | (in.crep ? RT_CREP : 0) | (jfr ? RT_JFR : 0)), false});
    }
    if (L.n_pile > 0) R.launches.push_back({MG_FAM_PILE, 0, 0, L.n_pile, in.crep ? RT_CREP : 0u, false});
    if (L.nf_rigid > 0)
        R.launches.push_back({MG_FAM_FREE, 0, 0, L.nf_rigid, (attr_free ? RT_ATTR : 0u) | (in.crep ? RT_CREP : 0u), false});

    // ---- a launch whose build does not exist, or drops a feature routed to it
    // under any MgRun a simulate can form: the first such run's loss words the refusal
    for (const MgLaunch& l : R.launches) {
        unsigned lost = 0;
        if (mg_route_each_run(L, l, [&](const MgRun& run) {
                const MgBuilds b = mg_route_builds(L, l, run);
                lost = l.feat & ~mg_build_carried(b);
                return b.built() && !lost;
            }))
            continue;
        if (l.family == MG_FAM_ARTIC && (l.feat & RT_JFR) && lost == RT_ATTR)
            mg_route_msg(launch_refusal, 0, "actor %d: joint friction (DOF friction > 0) together with an attractor on an "
                         "articulation of the same group is not built", artic_jactor[l.group]);
        else if (l.family == MG_FAM_ENV && (l.feat & RT_JFR) && lost)
            mg_route_msg(launch_refusal, 0, "actor %d: joint friction (DOF friction > 0) together with %s on the same "
                         "coupled group is not built", env_jactor[l.group],
                         lost & RT_CREP ? "contact reporting" : lost & RT_SENS ? "a force sensor" : "an attractor");
        else
            mg_route_msg(launch_refusal, 0, "step launch of family %d, group %d: features 0x%x are not built together", l.family,
                         l.group, l.feat);
        break;
    }
    R.refusal_msg = !attr_refusal.empty() ? attr_refusal : !R.sens_refusal.empty() ? R.sens_refusal : launch_refusal;
    R.refusal = R.refusal_msg.empty() ? MG_OK : MG_ERR_UNSUPPORTED;
    R.step_writes_rows = L.step_out_ok && in.n_attr == 0 && !in.crep && R.jfr_ndof == 0 && !in.sleep;
    return MG_OK;
}
