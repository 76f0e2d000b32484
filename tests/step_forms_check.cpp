// step_forms_check.cpp — the choice of a step kernel's build (csrc/mg_forms.h),
// checked on the host alone: for every kernel the form function is run over
// every combination of its inputs (block, CU and chain counts exactly at and
// one past each threshold); every chosen form must be a built one, every built
// form must be chosen by some input, and the cases DESIGN.md names must come
// out as documented. Exit status 0 and "0 failures" when all hold.
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

static void rigid() {
    const size_t fit = MG_TREC_LDS_MAX;
    std::set<Key> seen1, seen2;
    for (int upz = 0; upz < 2; ++upz)
        for (int cus : {1, 256, 304})
            for (int d = 0; d < 2; ++d)   // blocks at the threshold (one resident round) and one past it
                for (size_t lds : {fit, fit + 1})
                    for (int m = 0; m < 32; ++m) {
                        const bool rec = m & 1, attr = m & 2, crep = m & 4, ids = m & 8, box = m & 16;
                        const int blocks = cus * 4 * (upz ? MG_RIGID1_ROUND_WAVES : 2) + d;
                        const unsigned f = k_rigid_step1_form(upz, blocks, cus, lds, rec, attr, crep, ids, box);
                        seen1.insert({0, f});
                        CHECK(bool(f & RF_WIDE) == bool(d), "wide exactly past one resident round (form %u)", f);
                        CHECK(!ids || !(f & RF_REC), "free_ids set: no REC (form %u)", f);
                        CHECK(mg_rigid_form_public(f) == ((f & RF_WIDE ? 1 : 0) | (f & RF_REC ? 2 : 0) | (f & RF_BOX ? 4 : 0)),
                              "public bits of form %u", f);
                        seen2.insert({0, k_rigid_step_form(upz, attr, crep)});
                    }
    check_cover("k_rigid_step1", seen1, {0}, RF_BITS, [](int, unsigned f) { return k_rigid_step1_built(f); });
    check_cover("k_rigid_step", seen2, {0}, RF_BITS, [](int, unsigned f) { return k_rigid_step_built(f, 8, true); });
    CHECK(!k_rigid_step_built(RF_UPZ, 4, true) && !k_rigid_step_built(RF_UPZ, 8, false), "k_rigid_step: MAXC 8, MULTI only");

    // the documented cases: 64 blocks on 256 CUs, z-up, slot record, box-only, records fit LDS
    unsigned f = k_rigid_step1_form(true, 64, 256, 1024, true, false, false, false, true);
    CHECK(f == (RF_UPZ | RF_LDS | RF_REC | RF_BOX), "box-only one-round launch: form %u", f);
    CHECK(mg_rigid_form_public(f) == (MG_RIGID_FORM_REC | MG_RIGID_FORM_BOX), "reported %d", mg_rigid_form_public(f));
    f = k_rigid_step1_form(true, 64, 256, 1024, true, true, false, false, true);
    CHECK(f == (RF_UPZ | RF_ATTR | RF_REC), "with an attractor: form %u", f);
    f = k_rigid_step1_form(true, 64, 256, 1024, true, false, true, false, true);
    CHECK(f == (RF_UPZ | RF_CREP), "with reporting on: form %u", f);
    CHECK(mg_rigid_form_public(f) == 0, "reporting launch reported %d", mg_rigid_form_public(f));
    f = k_rigid_step1_form(true, 4096, 256, 1024, true, false, false, false, true);
    CHECK(f & RF_WIDE, "4096 blocks on 256 CUs: form %u", f);
    CHECK(mg_rigid_form_public(f) == MG_RIGID_FORM_WIDE, "wide launch reported %d", mg_rigid_form_public(f));
    f = k_rigid_step1_form(true, 4096, 256, 1024, true, false, true, false, true);
    CHECK(f == (RF_UPZ | RF_WIDE | RF_CREP), "a reporting launch keeps the plain WIDE threshold: form %u", f);
    f = k_rigid_step1_form(true, 64, 256, 1024, true, false, false, true, true);
    CHECK(!(f & RF_REC), "free_ids set: form %u", f);
    static_assert(MG_RIGID_FORM_WIDE == 1 && MG_RIGID_FORM_REC == 2 && MG_RIGID_FORM_BOX == 4, "public values");
}

static void chain() {
    std::set<Key> seenq, seenc;
    const int edge = MG_CHAIN_QUAD_MAX / 4;
    for (int nl = 2; nl <= 4; ++nl)
        for (int na : {1, 4096, edge, edge + 1, 262144})
            for (int m = 0; m < 16; ++m) {
                const bool ext = m & 1, uni = m & 2, aff = m & 4, frc = m & 8;
                const MgChainForm c = mg_chain_form(na, ext, uni, aff, frc);
                (c.quad ? seenq : seenc).insert({nl, c.f});
                CHECK(c.quad == (na <= edge), "%d chains: quad %d", na, c.quad);
                CHECK(!(c.f & CF_AFF) || (!c.quad && uni && aff), "AFF only if UNI, one-lane kernel (form %u)", c.f);
                CHECK(bool(c.f & CF_FRC) == frc && bool(c.f & CF_EXT) == ext && bool(c.f & CF_UNI) == uni, "form %u", c.f);
            }
    check_cover("k_artic_chain_q", seenq, {2, 3, 4}, CF_BITS, [](int nl, unsigned f) { return k_artic_chain_q_built(nl, f); });
    check_cover("k_artic_chain", seenc, {2, 3, 4}, CF_BITS, [](int nl, unsigned f) { return k_artic_chain_built(nl, f); });
    CHECK(!k_artic_chain_built(1, 0) && !k_artic_chain_built(5, 0), "chains of 2..4 links");
    CHECK(mg_chain_form(4096, false, true, true, false).quad, "4096 chains: the quad kernel");
    const MgChainForm c = mg_chain_form(16385, false, true, true, false);
    CHECK(!c.quad && c.f == (CF_UNI | CF_AFF), "16385 chains: the one-lane kernel, form %u", c.f);
    CHECK(mg_chain_form(16385, false, false, true, false).f == 0, "AFF only if UNI");
}

static void env() {
    std::set<Key> seen_e, seen_l;
    int per_obj[4] = {0, 0, 0, 0};
    for (int nl : {0, 1, 4, 5, 16, 17, 32})
        for (int ndof : {0, 4, 5, 16, 17, 32})
            for (int floating = 0; floating < 2; ++floating)
                for (int max_free : {0, 1, 2})
                    for (int m = 0; m < 32; ++m) {
                        const bool attr = m & 1, frc = m & 2, sens = m & 4, crep = m & 8, jfr = m & 16;
                        const int slots = ndof + (floating ? 6 : 0) + 6 * max_free;
                        if (slots > 32) continue;   // refused by the launcher (MG_ENV_SLOTS_WIDE)
                        const MgSizedForm k = k_env_step_form(nl, ndof, floating, slots, attr, frc, sens, crep, jfr);
                        seen_e.insert({k.maxl, k.f});
                        CHECK((k.maxl == 32) == (nl > 16 || slots > 16), "64 lanes past 16 links or slots");
                        CHECK(k.maxl >= nl, "%d links in a %d-link build", nl, k.maxl);
                        if (!floating && max_free == 0 && !sens && !crep) {
                            const MgSizedForm a = k_artic_lanes_form(nl, ndof, attr, frc, jfr);
                            seen_l.insert({a.maxl, a.f});
                            CHECK(a.maxl >= nl && mg_env_lanes(a.maxl) >= ndof, "k_artic_lanes size %d", a.maxl);
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
    MgSizedForm k = k_env_step_form(9, 9, false, 15, false, false, false, false, true);
    CHECK(k.f == (EF_FRC | EF_JFR) && k_env_step_object(k.f) == MG_ENV_OBJ_JFR, "jfr group: form %u", k.f);
    k = k_env_step_form(9, 9, false, 15, false, false, true, true, false);
    CHECK(k.f == (EF_FRC | EF_SENS | EF_CREP) && k_env_step_object(k.f) == MG_ENV_OBJ_CREP, "crep + ctorque: form %u", k.f);
    k = k_env_step_form(3, 2, false, 8, true, false, false, false, false);
    CHECK(k.maxl == 16 && k.f == EF_ATTR, "a small env with an attractor steps in the 16-link build");
}

static void pile() {
    std::set<Key> seen;
    for (int crep = 0; crep < 2; ++crep) seen.insert({0, k_pile_step_form(crep)});
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
    rigid();
    chain();
    env();
    pile();
    lift();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
