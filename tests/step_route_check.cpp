// step_route_check.cpp — stand-alone host check of the step features' routing plan
// (test_isaacgym_amd/csrc/mg_route.h, included alone). One small layout built by
// hand, every combination of the feature alphabet below, and for each the properties a route
// must have: every stepped instance in exactly one launch, owners in their owner launch, the
// split rows a stable permutation of the stepped rows, every launch's build (mg_route_builds: the
// choosers of mg_forms.h, under every MgRun) built and carrying exactly the routed features or
// else a refusal, the same across all MgRun, needing no buffer the plan's inputs do not allocate,
// and the refusals' full texts and precedence as the engine has always reported them.
// Prints "0 failures". The next feature adds one entry to the alphabet (main) and its expectation.
#include "mg_route.h"

static int failures = 0;
static long cases = 0;
#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            if (++failures <= 20) {                                \
                printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #c); \
                printf(__VA_ARGS__);                               \
                printf("\n");                                      \
            }                                                      \
        }                                                          \
    } while (0)

// global bodies of the layout
enum { B_FREE1 = 0, B_FREE2 = 1, B_CHAIN0 = 2, B_NC0 = 11, B_CA = 17, B_CA_FREE = 19, B_CB = 20, B_CB_FREE = 22,
       B_EF0 = 23, B_PILE0 = 25, B_STATIC = 28, NB = 29, ND = 12 };

// The members mg_route.h's opening comment lists, and no other:
//   group 0: chain template 0 (3 links, 2 DOFs), 3 uncoupled instances, bodies 2.., DOFs 0..
//   group 1: non-chain template 1 (3 links, 2 DOFs), 2 uncoupled instances, bodies 11.., DOFs 6..
//   group 2: template 2 (2 links, 1 DOF), stepped in coupled envs only: env group 0, 2 envs,
//            each with one free body; env group 1: one env of 2 free bodies, no articulation
//   free bodies 0 (single-shape) and 1 (multi-shape); one pile env of 3 bodies; static body 28
static MgLayout make_layout(bool step_out_ok) {
    MgLayout L;
    L.nb = NB; L.nd = ND; L.nf1 = 1; L.nf_rigid = 2; L.n_pile = 1; L.n_coupled = 3;
    L.step_out_ok = step_out_ok;
    L.perm.resize(NB);
    for (int b = 0; b < NB; ++b) L.perm[b] = NB - 1 - b;   // any permutation
    L.body_class.assign(NB, ATTR_NONE);
    L.body_grp.assign(NB, -1); L.body_inst.assign(NB, -1); L.body_artic.assign(NB, -1);
    L.body_class[B_FREE1] = L.body_class[B_FREE2] = ATTR_FREE;
    L.atmpl = {0, 3, 2, 0, 3, 3, 2, 0, 6, 2, 1, 0};                       // first link, links, DOFs, pad
    L.link_i = {-1, 0, -1, 0, 0, 0, 0, 1, 1, 0, 1, 2,                     // parent, type, dof, body
                -1, 0, -1, 0, 0, 0, 0, 1, 0, 0, 1, 2,
                -1, 0, -1, 0, 0, 0, 0, 1};
    auto artic = [&](int g0, int d0, int tmpl, int nl, bool coupled, int grp, int inst) {
        for (int l = 0; l < nl; ++l) {
            L.body_class[g0 + l] = coupled ? ATTR_ENV_LINK : ATTR_LINK;
            L.body_artic[g0 + l] = (int)L.artic_info.size();
            if (!coupled) { L.body_grp[g0 + l] = grp; L.body_inst[g0 + l] = inst; }
        }
        L.artic_info.push_back({g0, d0, tmpl, coupled ? 1 : 0});
        if (!coupled) L.artic_step.insert(L.artic_step.end(), {g0, d0, tmpl, 0});
    };
    for (int i = 0; i < 3; ++i) artic(B_CHAIN0 + 3 * i, 2 * i, 0, 3, false, 0, i);
    for (int i = 0; i < 2; ++i) artic(B_NC0 + 3 * i, 6 + 2 * i, 1, 3, false, 1, i);
    artic(B_CA, 10, 2, 2, true, 2, 0);
    artic(B_CB, 11, 2, 2, true, 2, 1);
    for (int b : {(int)B_CA_FREE, (int)B_CB_FREE, (int)B_EF0, B_EF0 + 1}) L.body_class[b] = ATTR_ENV_FREE;
    for (int b = B_PILE0; b < B_STATIC; ++b) L.body_class[b] = ATTR_PILE;
    MgArticGroup g{};
    g.fixed_base = 1;   // uncoupled articulations stand on a fixed base (a floating one steps in a coupled env)
    g.chain = 1; g.uni_mass = true; g.tmpl = 0; g.nl = 3; g.ndof = 2; g.aff = 1; g.step_offset = 0; g.step_count = 3;
    L.groups.push_back(g);
    g.chain = 0; g.uni_mass = false; g.tmpl = 1; g.aff = 0; g.step_offset = 3; g.step_count = 2;
    L.groups.push_back(g);
    g.tmpl = 2; g.nl = 2; g.ndof = 1; g.step_offset = 5; g.step_count = 0;
    L.groups.push_back(g);
    L.env_groups.push_back({2, 6, 2, 1, 0, 0, 1, 0, 2});    // tmpl, first_link, nl, ndof, floating, wide, max_free, offset, count
    L.env_groups.push_back({-1, 0, 0, 0, 0, 0, 2, 2, 1});
    L.env_d0 = {10, 11, 0};
    // actors in body order: 2 free, 5 articulations, coupled A + its free body, coupled B + its, 2 + 3 + 1 single bodies
    L.actor_dof = {0, 0, 0, 2, 4, 6, 8, 10, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12};
    return L;
}

// an attractor on: a free body, a link of each uncoupled instance, a coupled link, a coupled free body, a pile body, the static body
static const int kAttrSite[] = {B_FREE1, B_CHAIN0 + 1, B_CHAIN0 + 4, B_CHAIN0 + 7, B_NC0 + 1, B_NC0 + 4,
                                B_CA + 1, B_CA_FREE, B_PILE0, B_STATIC};
static const int kSensSite[] = {-1, B_CHAIN0 + 1, B_CA + 1, B_FREE1};   // none, an uncoupled link, a coupled link, the free body
static const int kFricDof[] = {-1, 0, 2, 5, 6, 9, 11};   // none, a DOF of each uncoupled instance, the second coupled env's DOF

static mg_attractor attractor(int body) {
    mg_attractor a{};
    a.body = body; a.axes = 63; a.stiffness = 10.0f; a.damping = 1.0f;
    a.offset_q[3] = a.target_q[3] = 1.0f;
    return a;
}

// What a simulate can hand the choosers for launch `l`: every MgRun, with devices on both sides of
// k_rigid_step1's wide threshold. Per launch the builds must not depend on it in what the route
// relies on: built or not, and the routed features carried. Returns those two; `needs`: the
// pointers any of the builds dereferences.
static unsigned builds_of(const MgLayout& L, const MgLaunch& l, bool& built, unsigned& needs) {
    const MgBuilds b0 = mg_route_builds(L, l, MgRun{false, false, false, 0});
    built = b0.built();
    needs = 0;
    for (int m = 0; m < 8; ++m)
        for (int cus : {0, 1, 256, 1 << 20}) {
            const MgBuilds b = mg_route_builds(L, l, MgRun{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0, cus});
            CHECK(b.built() == built && mg_build_carried(b) == mg_build_carried(b0),
                  "family %d group %d feat 0x%x: run %d, %d CUs changes built %d -> %d or carried 0x%x -> 0x%x", l.family, l.group,
                  l.feat, m, cus, (int)built, (int)b.built(), mg_build_carried(b0), mg_build_carried(b));
            CHECK((l.family == MG_FAM_FREE) == (b.multi.kernel != MG_K_NONE) && b.one.kernel != MG_K_NONE, "kernels of family %d", l.family);
            needs |= mg_build_needs(b.one) | mg_build_needs(b.multi);
        }
    return mg_build_carried(b0);
}

static void run_case(const MgLayout& L, const std::vector<int>& attr_bodies, int sens_body, bool crep, int fric_dof, bool frc) {
    ++cases;
    std::vector<mg_attractor> attrs;
    for (int b : attr_bodies) attrs.push_back(attractor(b));
    std::vector<mg_force_sensor> sens;
    if (sens_body >= 0) {
        mg_force_sensor f{};
        f.body = sens_body; f.q[3] = 2.0f; f.flags = MG_SENSOR_FORWARD | MG_SENSOR_CONSTRAINT;
        sens.push_back(f);
    }
    std::vector<float> props((size_t)ND * MG_DOFPROP_N, 0.0f);
    if (fric_dof >= 0) props[(size_t)fric_dof * MG_DOFPROP_N + 9] = 0.25f;
    MgRouteIn in;
    in.attrs = attrs.data(); in.n_attr = (int)attrs.size();
    in.sensors = sens.data(); in.n_sens = (int)sens.size();
    in.crep = crep; in.dof_props = props.data(); in.dof_frc_n = frc ? ND : 0;
    MgRoute R, R2;
    std::string err;
    const int rc = mg_plan_route(L, in, R, err);
    CHECK(rc == MG_OK, "rc %d %s", rc, err.c_str());
    if (rc) return;
    CHECK(mg_plan_route(L, in, R2, err) == MG_OK && R == R2 && R.same_launches(R2), "planning twice differs");

    // ---- what the engine has always done, restated: the owners, the refusals in precedence order
    std::vector<std::vector<unsigned>> own(L.groups.size());
    for (size_t gi = 0; gi < L.groups.size(); ++gi) own[gi].assign((size_t)L.groups[gi].step_count, 0);
    std::string want;
    char buf[512];
    bool attr_free = false, attr_clink = false;
    for (size_t i = 0; i < attrs.size(); ++i) {
        const int b = attrs[i].body;
        const char* why = nullptr;
        switch (L.body_class[b]) {
            case ATTR_FREE: attr_free = true; break;
            case ATTR_ENV_LINK: attr_clink = true; break;
            case ATTR_LINK: own[L.body_grp[b]][L.body_inst[b]] |= RT_ATTR; break;
            case ATTR_ENV_FREE: why = "a free body of a coupled env"; break;
            case ATTR_PILE: why = "a body of a pile env"; break;
            default: why = "not a dynamic body"; break;
        }
        if (why && want.empty()) {
            snprintf(buf, sizeof buf, "attractor %d on rigid body %d: %s cannot carry an attractor in this build", (int)i, b, why);
            want = buf;
        }
    }
    std::string want_sens;
    if (sens_body == B_FREE1) {
        snprintf(buf, sizeof buf, "force sensor %d on rigid body %d: a single-body actor has no joint to measure "
                 "(and the free-body and pile kernels keep no contact moment); force sensors sit on bodies of "
                 "articulations", 0, sens_body);
        want_sens = buf;
    }
    const bool want_class = !want.empty();
    if (want.empty()) want = want_sens;
    const bool fric_env = fric_dof == 11;
    int fric_grp = -1, fric_actor = -1;
    if (fric_dof >= 0 && !fric_env) {
        fric_grp = fric_dof < 6 ? 0 : 1;
        const int inst = fric_grp == 0 ? fric_dof / 2 : (fric_dof - 6) / 2;
        own[fric_grp][inst] |= RT_JFR;
        fric_actor = 2 + fric_dof / 2;   // actors 2..6 are the uncoupled articulations
    }
    if (want.empty() && fric_grp >= 0) {
        bool any_attr = false;
        for (unsigned o : own[fric_grp]) any_attr = any_attr || (o & RT_ATTR);
        if (any_attr) {
            snprintf(buf, sizeof buf, "actor %d: joint friction (DOF friction > 0) together with an attractor on an "
                     "articulation of the same group is not built", fric_actor);
            want = buf;
        }
    }
    if (want.empty() && fric_env) {
        const char* what = crep ? "contact reporting" : sens_body == B_CA + 1 ? "a force sensor" : attr_clink ? "an attractor" : nullptr;
        if (what) {
            snprintf(buf, sizeof buf, "actor %d: joint friction (DOF friction > 0) together with %s on the same "
                     "coupled group is not built", 9, what);   // actor 9: the second coupled articulation
            want = buf;
        }
    }
    CHECK(R.refusal_msg == want, "refusal '%s' want '%s'", R.refusal_msg.c_str(), want.c_str());
    CHECK(R.refusal == (want.empty() ? MG_OK : MG_ERR_UNSUPPORTED), "code %d", R.refusal);
    CHECK(R.sens_refusal == want_sens, "sensor refusal '%s'", R.sens_refusal.c_str());

    // ---- coverage, owners, the split rows
    bool any_owner = false;
    for (auto& g : own)
        for (unsigned o : g) any_owner = any_owner || o;
    CHECK(R.split.empty() == !any_owner, "split table %zu ints, owners %d", R.split.size(), (int)any_owner);
    if (any_owner) CHECK(R.split.size() == L.artic_step.size(), "split size");
    std::vector<std::vector<int>> seen(L.groups.size());
    for (size_t gi = 0; gi < L.groups.size(); ++gi) seen[gi].assign((size_t)L.groups[gi].step_count, 0);
    int n_env[2] = {0, 0}, n_pile = 0, n_free = 0, last_family = -1, last_group = -1;
    bool dropped = false;
    for (const MgLaunch& l : R.launches) {
        CHECK(l.family > last_family || (l.family == last_family && l.group >= last_group), "launch order");
        last_family = l.family; last_group = l.group;
        CHECK(l.count > 0, "empty launch");
        bool built = false;
        unsigned needs = 0;
        const unsigned carried = builds_of(L, l, built, needs);
        const bool ok = built && carried == l.feat;
        dropped = dropped || !ok;
        CHECK(ok || !R.refusal_msg.empty(), "family %d group %d feat 0x%x: carried 0x%x built %d and no refusal", l.family,
              l.group, l.feat, carried, (int)built);
        // an unrefused plan: every buffer a build dereferences exists under the plan's inputs
        // (the sensor tables, the reporting records and the attractor table are allocated with their feature)
        if (R.refusal_msg.empty())
            CHECK((!(needs & MG_NEED_CTORQUE) || R.n_sens > 0) && (!(needs & MG_NEED_CREP) || crep) &&
                      (!(needs & MG_NEED_ATTR) || !attrs.empty()),
                  "family %d group %d feat 0x%x needs 0x%x: a buffer the plan's inputs do not allocate", l.family, l.group, l.feat, needs);
        CHECK(((l.feat & RT_FRC) != 0) == (frc || (l.feat & (RT_SENS | RT_CREP | RT_JFR))) || l.family >= MG_FAM_PILE, "FRC bit 0x%x", l.feat);
        if (l.family == MG_FAM_ARTIC) {
            const MgArticGroup& g = L.groups[l.group];
            unsigned kinds = 0;
            for (unsigned o : own[l.group]) kinds |= o;
            CHECK(l.split == (kinds != 0), "split flag");
            CHECK(l.row0 >= g.step_offset && l.row0 + l.count <= g.step_offset + g.step_count, "rows outside the group");
            const std::vector<int>& rows = l.split ? R.split : L.artic_step;
            int prev = -1;
            for (int r = l.row0; r < l.row0 + l.count; ++r) {
                const int inst = L.body_inst[rows[(size_t)r * MG_ARTIC_I_N]];
                CHECK(L.body_grp[rows[(size_t)r * MG_ARTIC_I_N]] == l.group, "row of another group");
                CHECK(std::memcmp(&rows[(size_t)r * MG_ARTIC_I_N], &L.artic_step[(size_t)(g.step_offset + inst) * MG_ARTIC_I_N],
                                  MG_ARTIC_I_N * sizeof(int)) == 0, "row differs from artic_step's");
                CHECK(inst > prev, "not in stepped order");   // with exactly-once below: a stable permutation
                prev = inst;
                seen[l.group][inst]++;
                const unsigned o = own[l.group][inst];
                CHECK((o & ~l.feat) == 0, "owner 0x%x in a launch with 0x%x", o, l.feat);
                CHECK((o == 0) == !(l.feat & (RT_ATTR | RT_JFR)), "plain instance in an owner launch or the reverse");
            }
            CHECK(!(l.feat & (RT_SENS | RT_CREP)), "articulation launch 0x%x", l.feat);
        } else if (l.family == MG_FAM_ENV) {
            const MgEnvGroup& g = L.env_groups[l.group];
            CHECK(l.row0 == g.offset && l.count == g.count && !l.split, "env rows");
            n_env[l.group]++;
            const bool jfr = fric_env && l.group == 0;
            // every group without friction gets the attractor build as soon as any coupled link owns one
            unsigned feat = (attr_clink && (!jfr || l.group == 0) ? RT_ATTR : 0) | (sens_body == B_CA + 1 && l.group == 0 ? RT_SENS : 0) |
                            (crep ? RT_CREP : 0) | (jfr ? RT_JFR : 0);
            if (frc || (feat & (RT_SENS | RT_CREP | RT_JFR))) feat |= RT_FRC;
            CHECK(l.feat == feat, "env group %d feat 0x%x want 0x%x", l.group, l.feat, feat);
        } else if (l.family == MG_FAM_PILE) {
            n_pile++;
            CHECK(l.count == L.n_pile && l.feat == (crep ? RT_CREP : 0u), "pile launch");
        } else {
            n_free++;
            CHECK(l.count == L.nf_rigid && l.feat == ((attr_free ? RT_ATTR : 0u) | (crep ? RT_CREP : 0u)), "free-body launch 0x%x", l.feat);
        }
    }
    for (size_t gi = 0; gi < seen.size(); ++gi)
        for (size_t k = 0; k < seen[gi].size(); ++k) CHECK(seen[gi][k] == 1, "group %zu instance %zu in %d launches", gi, k, seen[gi][k]);
    CHECK(n_env[0] == 1 && n_env[1] == 1 && n_pile == 1 && n_free == 1, "one launch per coupled group, piles, free bodies");
    // a refusal in these cases and in no other
    CHECK(R.refusal_msg.empty() == !(want_class || !want_sens.empty() || dropped), "refusal '%s' with dropped %d",
          R.refusal_msg.c_str(), (int)dropped);

    const int nfric = fric_dof >= 0 ? 1 : 0;
    CHECK(R.step_writes_rows == (L.step_out_ok && attrs.empty() && !crep && nfric == 0), "step_writes_rows");
    CHECK(R.jfr_ndof == nfric && R.jfr_lanes == (fric_grp >= 0 ? 1 : 0) && R.jfr_envs == (fric_env ? 2 : 0), "stats %d %d %d",
          R.jfr_ndof, R.jfr_lanes, R.jfr_envs);
    CHECK(R.n_attr == (int)attrs.size() && R.crep == crep && R.dof_frc_n == in.dof_frc_n, "echo");
    for (size_t i = 0; i < attrs.size(); ++i) CHECK(R.attr_idx[L.perm[attrs[i].body]] == (int)i, "slot -> record");
    const int ns = want_sens.empty() && sens_body >= 0 ? 1 : 0;
    CHECK(R.n_sens == ns && R.n_sart == ns, "sensor lanes %d", R.n_sens);
    if (ns) {
        const MgArticInfo& ai = L.artic_info[L.body_artic[sens_body]];
        CHECK(R.si[RS_G0] == ai.g0 && R.si[RS_LINK] == 1 && R.si[RS_MASK] == (ai.tmpl == 0 ? 6 : 2) && R.si[RS_OUT] == 0 &&
              R.si[RS_OWNER] == 1 && R.sf[6] == 1.0f, "sensor lane");
        CHECK(R.sart[0] == L.perm[ai.g0] && R.sart[1] == ai.d0 && R.sens_nhb == (ai.tmpl == 0 ? 3 : 2) &&
              R.sens_nsave == MG_STATE_N + 2 * (ai.tmpl == 0 ? 2 : 1), "sensor articulation row");
    }
    if (attrs.empty() && sens_body < 0 && !crep && fric_dof < 0 && !frc) {   // everything off
        CHECK(R.launches.size() == 6 && R.split.empty(), "%zu launches with everything off", R.launches.size());
        for (const MgLaunch& l : R.launches) CHECK(l.feat == 0 && !l.split, "plain launch 0x%x", l.feat);
    }
}

int main() {
    for (int out_ok = 0; out_ok < 2; ++out_ok) {
        const MgLayout L = make_layout(out_ok != 0);
        const int ns = (int)(sizeof kAttrSite / sizeof kAttrSite[0]);
        std::vector<std::vector<int>> attr_sets = {{}};
        for (int i = 0; i < ns; ++i) attr_sets.push_back({kAttrSite[i]});
        for (int i = 0; i < ns; ++i)
            for (int j = 0; j < ns; ++j)
                if (i != j) attr_sets.push_back({kAttrSite[i], kAttrSite[j]});   // both table orders: the first refusal wins
        for (const auto& as : attr_sets)
            for (int sb : kSensSite)
                for (int crep = 0; crep < 2; ++crep)
                    for (int fd : kFricDof)
                        for (int frc = 0; frc < 2; ++frc) run_case(L, as, sb, crep != 0, fd, frc != 0);
    }
    // the tables' validation keeps its codes and texts
    const MgLayout L = make_layout(true);
    MgRoute R;
    std::string err;
    MgRouteIn in;
    mg_attractor two[2] = {attractor(B_FREE1), attractor(B_FREE1)};
    in.attrs = two; in.n_attr = 2;
    CHECK(mg_plan_route(L, in, R, err) == MG_ERR_UNSUPPORTED && err == "attractor 1: body 0 already owns attractor 0 (one attractor per body)",
          "%s", err.c_str());
    two[1].body = NB;
    CHECK(mg_plan_route(L, in, R, err) == MG_ERR_ARG && err == "attractor 1: body 29 out of range", "%s", err.c_str());
    two[1].body = B_FREE2; two[1].damping = -1.0f;
    CHECK(mg_plan_route(L, in, R, err) == MG_ERR_ARG && err == "attractor 1: stiffness and damping must be finite and non-negative",
          "%s", err.c_str());
    in = MgRouteIn();
    mg_force_sensor f{};
    f.body = B_CHAIN0;
    in.sensors = &f; in.n_sens = 1;
    CHECK(mg_plan_route(L, in, R, err) == MG_ERR_ARG && err == "force sensor 0: the local pose must be finite, its rotation not zero",
          "%s", err.c_str());
    in = MgRouteIn();
    std::vector<float> props((size_t)ND * MG_DOFPROP_N, 0.0f);
    props[3 * MG_DOFPROP_N + 9] = -0.5f;
    in.dof_props = props.data();
    CHECK(mg_plan_route(L, in, R, err) == MG_ERR_ARG && err == "DOF 3: friction -0.5 must be finite and non-negative", "%s", err.c_str());
    printf("%ld cases\n%d failures\n", cases, failures);
    return failures ? 1 : 0;
}
