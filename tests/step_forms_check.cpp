// step_forms_check.cpp — which kernel, at which size and form, a step launch runs (the choosers
// of csrc/mg_forms.h), checked on the host alone: every chooser is run over every combination of
// its inputs (every MgRun; block, CU and chain counts exactly at and one past each threshold;
// sizes at and past each limit); every chosen build must be a built one, every built form must
// be chosen by some input, the pointers a build needs must cover every bit of its own form word,
// and the cases DESIGN.md names must come out as documented. The check calls no _form function:
// the choosers are the single statement. Exit status 0 and "0 failures" when all hold.
#include <cstdio>
#include <set>
#include <utility>

#include "mg_forms.h"

static int failures = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            ++failures;                       \
            std::printf("FAIL %s: ", #c);     \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

using Key = std::pair<int, unsigned>;   // integer parameter (0: none), form word

// every built (size, form) of `sizes` x [0, 2^bits) is in `seen`, and nothing else is
template <class Built>
static void check_cover(const char* kernel, const std::set<Key>& seen, std::initializer_list<int> sizes, unsigned bits,
                        Built built) {
    int n_built = 0;
    for (int z : sizes)
        for (unsigned f = 0; f < (1u << bits); ++f)
            if (built(z, f)) {
                ++n_built;
                CHECK(seen.count({z, f}), "%s<%d, %u> is built but no input chooses it", kernel, z, f);
            }
    for (const Key& k : seen) CHECK(built(k.first, k.second), "%s<%d, %u> is chosen but not built", kernel, k.first, k.second);
    std::printf("%s: %d builds, %zu chosen\n", kernel, n_built, seen.size());
}

// The member of the argument block each form bit's code dereferences, per kernel: the check's own
// table, from the kernels. A build must need at least these (the form's own bits, not the routed ones).
struct BitNeed { unsigned bit, need; };
static void check_needs(const MgBuild& b) {
    static const BitNeed rigid1[] = {{RF_ATTR, MG_NEED_ATTR}, {RF_REC, MG_NEED_SLOT_REC}, {RF_CREP, MG_NEED_CREP}, {0, 0}};
    static const BitNeed rigid[] = {{RF_ATTR, MG_NEED_ATTR}, {RF_CREP, MG_NEED_CREP}, {0, 0}};
    static const BitNeed chain[] = {{CF_EXT, MG_NEED_EXT}, {CF_UNI, MG_NEED_UNI}, {CF_FRC, MG_NEED_DOF_FRC}, {0, 0}};
    static const BitNeed lanes[] = {{LF_ATTR, MG_NEED_ATTR}, {LF_FRC, MG_NEED_DOF_FRC}, {0, 0}};
    static const BitNeed env[] = {{EF_ATTR, MG_NEED_ATTR}, {EF_FRC, MG_NEED_DOF_FRC}, {EF_SENS, MG_NEED_CTORQUE},
                                  {EF_CREP, MG_NEED_CREP}, {0, 0}};
    static const BitNeed pile[] = {{PF_CREP, MG_NEED_CREP}, {0, 0}};
    const BitNeed* t = b.kernel == MG_K_RIGID_STEP1 ? rigid1 : b.kernel == MG_K_RIGID_STEP ? rigid
                     : b.kernel == MG_K_ARTIC_CHAIN || b.kernel == MG_K_ARTIC_CHAIN_Q ? chain
                     : b.kernel == MG_K_ARTIC_LANES ? lanes : b.kernel == MG_K_ENV_STEP ? env : pile;
    const unsigned need = mg_build_needs(b);
    for (; t->bit; ++t)
        CHECK(!(b.form & t->bit) || (need & t->need), "kernel %d form %u: bit %u set, pointer 0x%x not needed", b.kernel, b.form,
              t->bit, t->need);
    CHECK(mg_build_fits(b, need, b.kernel) == b.built && (!need || !mg_build_fits(b, 0, b.kernel)) &&
              !mg_build_fits(b, need, MG_K_NONE),
          "kernel %d form %u: mg_build_fits", b.kernel, b.form);
}

static MgRun run_of(int m, int cus) { return MgRun{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0, cus}; }

static void rigid() {
    const size_t fit = MG_TREC_LDS_MAX;
    std::set<Key> seen1, seen2;
    for (int r = 0; r < 8; ++r)
        for (int cus : {1, 256, 304})
            for (int d = 0; d < 2; ++d)   // blocks at the threshold (one resident round) and one past it
                for (size_t lds : {fit, fit + 1})
                    for (int m = 0; m < 16; ++m)
                        for (int more : {0, 1}) {
                            const MgRun run = run_of(r, cus);
                            const bool rec = m & 1, attr = m & 2, crep = m & 4, box = m & 8;
                            const int blocks = cus * 4 * (run.upz ? MG_RIGID1_ROUND_WAVES : 2) + d;
                            const unsigned feat = (attr ? EF_ATTR : 0) | (crep ? EF_CREP : 0);
                            // the last block full, or holding one body
                            for (int nf1 : {blocks * 64, blocks * 64 - 63}) {
                                const MgBuilds b = mg_choose_free(nf1, nf1 + more, lds, rec, box, feat, run);
                                const unsigned f = b.one.form;
                                CHECK(b.built() && b.one.kernel == MG_K_RIGID_STEP1 && b.one.size == 0, "k_rigid_step1 form %u", f);
                                CHECK(b.multi.kernel == (more ? MG_K_RIGID_STEP : MG_K_NONE) && (!more || b.multi.size == 8),
                                      "k_rigid_step only with multi-shape bodies");
                                seen1.insert({0, f});
                                if (more) seen2.insert({0, b.multi.form});
                                CHECK(bool(f & RF_WIDE) == bool(d), "wide exactly past one resident round (form %u)", f);
                                CHECK(bool(f & RF_UPZ) == run.upz, "UPZ follows the run (form %u)", f);
                                CHECK(!(f & RF_REC) || (rec && !crep), "REC without a slot record, or with reporting (form %u)", f);
                                CHECK(mg_rigid_form_public(f) == ((f & RF_WIDE ? 1 : 0) | (f & RF_REC ? 2 : 0) | (f & RF_BOX ? 4 : 0)),
                                      "public bits of form %u", f);
                                CHECK(mg_build_carried(b) == feat, "free bodies carry 0x%x of 0x%x", mg_build_carried(b), feat);
                                check_needs(b.one);
                                if (more) check_needs(b.multi);
                                // ext and step_out change nothing here
                                const MgBuilds b0 = mg_choose_free(nf1, nf1 + more, lds, rec, box, feat, run_of(r & 1, cus));
                                CHECK(b0.one.form == f && b0.multi.form == b.multi.form, "ext / step_out moved a free-body form");
                            }
                        }
    check_cover("k_rigid_step1", seen1, {0}, RF_BITS, [](int, unsigned f) { return k_rigid_step1_built(f); });
    check_cover("k_rigid_step", seen2, {0}, RF_BITS, [](int, unsigned f) { return k_rigid_step_built(f, 8, true); });
    CHECK(!k_rigid_step_built(RF_UPZ, 4, true) && !k_rigid_step_built(RF_UPZ, 8, false), "k_rigid_step: MAXC 8, MULTI only");
    const MgRun up{true, false, false, 256};
    const MgBuilds none = mg_choose_free(0, 0, 0, true, true, 0, up), multi = mg_choose_free(0, 5, 0, true, true, 0, up);
    CHECK(!none.built() && none.one.kernel == MG_K_NONE && none.multi.kernel == MG_K_NONE, "no bodies: no build");
    CHECK(multi.built() && multi.one.kernel == MG_K_NONE && multi.multi.form == RF_UPZ, "multi-shape bodies alone");

    // the documented cases: 64 blocks on 256 CUs, z-up, slot record, box-only, records fit LDS
    auto one = [&](int blocks, unsigned feat) { return mg_choose_free(blocks * 64, blocks * 64, 1024, true, true, feat, up).one; };
    unsigned f = one(64, 0).form;
    CHECK(f == 83 && f == (RF_UPZ | RF_LDS | RF_REC | RF_BOX), "box-only one-round launch: form %u", f);
    CHECK(mg_rigid_form_public(f) == (MG_RIGID_FORM_REC | MG_RIGID_FORM_BOX), "reported %d", mg_rigid_form_public(f));
    CHECK(mg_build_needs(one(64, 0)) == MG_NEED_SLOT_REC, "form 83 needs the slot record alone");
    f = one(64, EF_ATTR).form;
    CHECK(f == (RF_UPZ | RF_ATTR | RF_REC), "with an attractor: form %u", f);
    f = one(64, EF_CREP).form;
    CHECK(f == (RF_UPZ | RF_CREP), "with reporting on: form %u", f);
    CHECK(mg_rigid_form_public(f) == 0, "reporting launch reported %d", mg_rigid_form_public(f));
    CHECK(mg_build_needs(one(64, EF_CREP)) == MG_NEED_CREP, "a reporting launch reads no slot record");
    f = one(4096, 0).form;
    CHECK(f & RF_WIDE, "4096 blocks on 256 CUs: form %u", f);
    CHECK(mg_rigid_form_public(f) == MG_RIGID_FORM_WIDE, "wide launch reported %d", mg_rigid_form_public(f));
    f = one(4096, EF_CREP).form;
    CHECK(f == (RF_UPZ | RF_WIDE | RF_CREP), "a reporting launch keeps the plain WIDE threshold: form %u", f);
    f = mg_choose_free(4096, 4096, 1024, false, true, 0, up).one.form;
    CHECK(!(f & RF_REC), "no slot record: form %u", f);
    static_assert(MG_RIGID_FORM_WIDE == 1 && MG_RIGID_FORM_REC == 2 && MG_RIGID_FORM_BOX == 4, "public values");
}

static void chain() {
    std::set<Key> seenq, seenc;
    const int edge = MG_CHAIN_QUAD_MAX / 4;
    for (int nl = 2; nl <= 4; ++nl)
        for (int na : {1, 4096, edge, edge + 1, 262144})
            for (int r = 0; r < 8; ++r)
                for (int m = 0; m < 32; ++m) {
                    const MgRun run = run_of(r, 256);
                    const bool uni = m & 1, aff = m & 2, out_aff = m & 4, split = m & 8, frc = m & 16;
                    const MgBuild b = mg_choose_artic(nl, nl - 1, true, true, uni, aff, out_aff, split, na, frc ? EF_FRC : 0, run);
                    const bool quad = b.kernel == MG_K_ARTIC_CHAIN_Q;
                    CHECK(b.built && (quad || b.kernel == MG_K_ARTIC_CHAIN) && b.size == nl, "chain of %d links: kernel %d", nl, b.kernel);
                    (quad ? seenq : seenc).insert({nl, b.form});
                    CHECK(quad == (na <= edge), "%d chains: quad %d", na, quad);
                    CHECK(b.aff == (aff && !split) && b.out_aff == (out_aff && !split), "a split launch loads its rows");
                    CHECK(bool(b.form & CF_AFF) == (MG_CHAIN_AFF && !quad && uni && b.aff && (!run.step_out || b.out_aff)),
                          "AFF: UNI, one-lane kernel, rows affine, written rows affine too (form %u)", b.form);
                    CHECK(bool(b.form & CF_FRC) == frc && bool(b.form & CF_EXT) == run.ext && bool(b.form & CF_UNI) == uni, "form %u",
                          b.form);
                    CHECK(mg_build_carried(b) == (frc ? EF_FRC : 0u), "chain carries 0x%x", mg_build_carried(b));
                    check_needs(b);
                    CHECK(mg_choose_artic(nl, nl - 1, true, true, uni, aff, out_aff, split, na, frc ? EF_FRC : 0, run_of(r ^ 1, 1)).form ==
                              b.form, "upz / cus moved a chain form");
                }
    check_cover("k_artic_chain_q", seenq, {2, 3, 4}, CF_BITS, [](int nl, unsigned f) { return k_artic_chain_q_built(nl, f); });
    check_cover("k_artic_chain", seenc, {2, 3, 4}, CF_BITS, [](int nl, unsigned f) { return k_artic_chain_built(nl, f); });
    CHECK(!k_artic_chain_built(1, 0) && !k_artic_chain_built(5, 0), "chains of 2..4 links");
    // the chain condition, written once (mg_choose_artic): chain, 2 to 4 links, no attractor, no friction
    const MgRun plain{true, false, false, 256};
    for (int nl = 1; nl <= 5; ++nl)
        for (int is_chain = 0; is_chain < 2; ++is_chain)
            for (unsigned feat : {0u, (unsigned)EF_FRC, (unsigned)EF_ATTR, (unsigned)(EF_FRC | EF_JFR)}) {
                const MgBuild b = mg_choose_artic(nl, nl - 1, true, is_chain, true, true, true, false, 8, feat, plain);
                const bool want = is_chain && nl >= 2 && nl <= 4 && !(feat & (EF_ATTR | EF_JFR));
                CHECK((b.kernel != MG_K_ARTIC_LANES) == want, "%d links, chain %d, feat 0x%x: kernel %d", nl, is_chain, feat, b.kernel);
            }
    const MgRun out{true, false, true, 256};
    MgBuild c = mg_choose_artic(3, 2, true, true, true, true, true, false, 4096, 0, plain);
    CHECK(c.kernel == MG_K_ARTIC_CHAIN_Q && c.form == CF_UNI, "4096 chains: the quad kernel, form %u", c.form);
    c = mg_choose_artic(3, 2, true, true, true, true, false, false, 16385, 0, plain);
    CHECK(c.kernel == MG_K_ARTIC_CHAIN && c.form == (CF_UNI | CF_AFF), "16385 chains: the one-lane kernel, form %u", c.form);
    CHECK(mg_choose_artic(3, 2, true, true, false, true, false, false, 16385, 0, plain).form == 0, "AFF only if UNI");
    CHECK(mg_choose_artic(3, 2, true, true, true, true, false, false, 16385, 0, out).form == CF_UNI, "written rows not affine: no AFF");
    CHECK(mg_choose_artic(3, 2, true, true, true, true, true, false, 16385, 0, out).form == (CF_UNI | CF_AFF), "written rows affine: AFF");
    CHECK(mg_choose_artic(3, 2, true, true, true, true, true, true, 16385, 0, plain).form == CF_UNI, "a split launch: no AFF");
}

static void env() {
    std::set<Key> seen_e, seen_l;
    int per_obj[4] = {0, 0, 0, 0};
    for (int nl : {0, 1, 4, 5, 16, 17, 32, 33})
        for (int ndof : {0, 4, 5, 16, 17, 32, 33})
            for (int floating = 0; floating < 2; ++floating)
                for (int max_free : {0, 1, 2})
                    for (unsigned m = 0; m < 32; ++m) {
                        const bool attr = m & EF_ATTR, sens = m & EF_SENS, crep = m & EF_CREP, jfr = m & EF_JFR;
                        const int slots = ndof + (floating ? 6 : 0) + 6 * max_free;
                        const MgBuild k = mg_choose_env(nl, ndof, floating, max_free, m, run_of(0, 256));
                        for (int r = 1; r < 8; ++r) {
                            const MgBuild k2 = mg_choose_env(nl, ndof, floating, max_free, m, run_of(r, 1));
                            CHECK(k2.form == k.form && k2.size == k.size && k2.np == k.np && k2.built == k.built, "the run moved k_env_step");
                        }
                        CHECK(k.kernel == MG_K_ENV_STEP, "kernel %d", k.kernel);
                        // more links or slots than the 64-lane build holds: no build
                        CHECK(k.built == (nl <= 32 && slots <= 32), "%d links, %d slots: built %d", nl, slots, (int)k.built);
                        check_needs(k);
                        if (k.built) {
                            seen_e.insert({k.size, k.form});
                            CHECK((k.size == 32) == (nl > 16 || slots > 16), "64 lanes past 16 links or slots");
                            CHECK(k.size >= nl && mg_env_lanes(k.size) >= slots, "%d links, %d slots in a %d-link build", nl, slots, k.size);
                            // the narrow phase follows the env alone
                            CHECK(k.np == (nl > 16 || slots > 16 ? 32 : nl <= 4 && ndof <= 4 && !floating ? 4 : 16), "k_env_np<%d>", k.np);
                            CHECK((k.np == 32) == (k.size == 32) && k.np <= k.size, "k_env_np<%d> before k_env_step<%d>", k.np, k.size);
                            // forced bits: DOF forces with sensors, reporting, friction; a friction group has none of the others
                            const unsigned want = jfr ? EF_FRC | EF_JFR : m | (m & (EF_SENS | EF_CREP) ? EF_FRC : 0);
                            CHECK(k.form == want && mg_build_carried(k) == want, "feat 0x%x: form 0x%x", m, k.form);
                        }
                        if (max_free == 0 && !sens && !crep) {
                            const MgBuild a = mg_choose_artic(nl, ndof, !floating, false, true, true, true, false, 8, m, run_of(0, 256));
                            for (int r = 1; r < 8; ++r)
                                CHECK(mg_choose_artic(nl, ndof, !floating, false, true, true, true, false, 8, m, run_of(r, 1)).form == a.form,
                                      "the run moved k_artic_lanes");
                            CHECK(a.kernel == MG_K_ARTIC_LANES && !a.aff && !a.out_aff, "kernel %d", a.kernel);
                            // a floating base, more links or DOFs than the 64-lane build holds: no build
                            CHECK(a.built == (!floating && nl <= 32 && ndof <= 32), "%d links, %d DOFs, floating %d: built %d", nl, ndof,
                                  floating, (int)a.built);
                            check_needs(a);
                            if (a.built) {
                                seen_l.insert({a.size, a.form});
                                CHECK(a.size >= nl && mg_env_lanes(a.size) >= ndof, "k_artic_lanes size %d", a.size);
                                CHECK(!attr || jfr || a.size >= 16, "attractors: the 16-link build at least");
                            }
                        }
                    }
    check_cover("k_env_step", seen_e, {32, 16, 4}, EF_BITS,
                [](int maxl, unsigned f) { return k_env_step_built(maxl, mg_env_lanes(maxl), f); });
    check_cover("k_artic_lanes", seen_l, {32, 16, 4}, LF_BITS,
                [](int maxl, unsigned f) { return k_artic_lanes_built(maxl, mg_env_lanes(maxl), f); });
    CHECK(!k_env_step_built(16, 64, 0) && !k_env_step_built(8, 16, 0), "sizes: 32 in 64 lanes, 16 or 4 in 16");
    // one object per form: the counts the objects hold
    for (const Key& k : seen_e) per_obj[k_env_step_object(k.second)]++;
    for (const Key& k : seen_l) per_obj[k_artic_lanes_object(k.second)]++;
    CHECK(per_obj[MG_ENV_OBJ_MAIN] == 20 && per_obj[MG_ENV_OBJ_SENS] == 5 && per_obj[MG_ENV_OBJ_CREP] == 10 &&
              per_obj[MG_ENV_OBJ_JFR] == 6,
          "forms per object: %d %d %d %d", per_obj[0], per_obj[1], per_obj[2], per_obj[3]);

    // the documented cases: a Franka-sized group (9 links, 9 DOFs, one free body)
    const MgRun run{true, false, false, 256};
    MgBuild k = mg_choose_env(9, 9, false, 1, EF_FRC | EF_JFR, run);
    CHECK(k.form == (EF_FRC | EF_JFR) && k_env_step_object(k.form) == MG_ENV_OBJ_JFR, "jfr group: form %u", k.form);
    k = mg_choose_env(9, 9, false, 1, EF_SENS | EF_CREP, run);
    CHECK(k.form == (EF_FRC | EF_SENS | EF_CREP) && k_env_step_object(k.form) == MG_ENV_OBJ_CREP, "crep + ctorque: form %u", k.form);
    CHECK(mg_build_needs(k) == (MG_NEED_DOF_FRC | MG_NEED_CTORQUE | MG_NEED_CREP), "crep + ctorque needs 0x%x", mg_build_needs(k));
    k = mg_choose_env(3, 2, false, 1, EF_ATTR, run);
    CHECK(k.size == 16 && k.np == 4 && k.form == EF_ATTR, "a small env with an attractor steps in the 16-link build after k_env_np<4>");
}

static void pile() {
    std::set<Key> seen;
    for (unsigned m = 0; m < 32; ++m)
        for (int r = 0; r < 8; ++r) {
            const MgBuild b = mg_choose_pile(m, run_of(r, 256));
            CHECK(b.built && b.kernel == MG_K_PILE_STEP && b.form == (m & EF_CREP ? PF_CREP : 0u), "pile form %u", b.form);
            CHECK(mg_build_carried(b) == (m & EF_CREP), "a pile carries reporting alone");
            check_needs(b);
            seen.insert({0, b.form});
        }
    check_cover("k_pile_step", seen, {0}, PF_BITS, [](int, unsigned f) { return k_pile_step_built(f); });
}

// the lifting helpers reach exactly the word they are given
static void lift() {
    for (unsigned f = 0; f < 32; ++f) {
        unsigned got = ~0u;
        const bool r = mg_with_form<5>(f, [&](auto c) { got = decltype(c)::value; return got % 3 != 0; });
        CHECK(got == f && r == (f % 3 != 0), "mg_with_form(%u) reached %u", f, got);
    }
    for (int v = 1; v <= 5; ++v) {
        int got = -1;
        const bool r = mg_with_int<2, 3, 4>(v, [&](auto c) { got = decltype(c)::value; return true; });
        CHECK(r == (v >= 2 && v <= 4) && got == (r ? v : -1), "mg_with_int(%d) reached %d", v, got);
    }
}

int main() {
    const float z[3] = {0, 0, 1}, y[3] = {0, 1, 0}, mx[3] = {-1, 0, 0}, x[3] = {1, 0, 0};
    CHECK(mg_step_is_upz(z, y, mx) && !mg_step_is_upz(y, z, mx) && !mg_step_is_upz(z, y, x), "mg_step_is_upz: the +Z basis alone");
    rigid();
    chain();
    env();
    pile();
    lift();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
