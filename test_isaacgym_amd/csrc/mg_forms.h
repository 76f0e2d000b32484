// mg_forms.h — which build of a step kernel a launch gets. Plain C++17: no HIP,
// no device header (tests/step_forms_check.cpp includes it alone). A step kernel's bool template
// parameters are the bits of one form word F; per kernel this header holds the bits,
// <kernel>_built (the single list of the builds that exist: the kernel static_asserts it, the
// launcher instantiates nothing else) and <kernel>_form (a form from plain inputs). The _form
// functions are internals of the choosers at the end of the file: one chooser per kernel family
// states "this launch runs this kernel at this form" (MgBuild). The route refuses by it
// (mg_route.h), the argument builders fill the pointers it needs (migym_capi.cpp), the launchers
// launch it. Nothing else calls a _form function or picks a kernel.
#pragma once
#include <stddef.h>
#include <type_traits>

#include "../../include/migym.h"

// Lifts a run-time word into a template argument: fn(std::integral_constant<unsigned, F>) for
// the F that equals f's low BITS bits; returns fn's result (true: launched, false: no such build)
template <unsigned BITS, unsigned F = 0, class Fn>
inline bool mg_with_form(unsigned f, Fn&& fn) {
    if constexpr (BITS == 0) return fn(std::integral_constant<unsigned, F>{});
    else if ((f >> (BITS - 1)) & 1u) return mg_with_form<BITS - 1, F | (1u << (BITS - 1))>(f, fn);
    else return mg_with_form<BITS - 1, F>(f, fn);
}
// the same for an integer parameter out of a short list; false when v is not in it
template <int... Vs, class Fn>
inline bool mg_with_int(int v, Fn&& fn) {
    bool r = false;
    (void)((v == Vs && ((r = fn(std::integral_constant<int, Vs>{})), true)) || ...);
    return r;
}

// ---- k_rigid_step1 (single-shape free bodies) and k_rigid_step (the others) ----
// UPZ: the +Z ground basis; LDS: template records staged in LDS; WIDE: more waves than one resident
// round; ATTR: a free body owns an attractor; REC: one-round launch that reads the packed slot record;
// CREP: contact reporting; BOX: every shape a plain box (MgRigidArgs::box_only)
enum : unsigned { RF_UPZ = 1, RF_LDS = 2, RF_WIDE = 4, RF_ATTR = 8, RF_REC = 16, RF_CREP = 32, RF_BOX = 64, RF_BITS = 7 };
#ifndef MG_RIGID1_ROUND_WAVES
#define MG_RIGID1_ROUND_WAVES 2
#endif
#ifndef MG_RIGID1_WIDE_WAVES
#define MG_RIGID1_WIDE_WAVES 3
#endif
#ifndef MG_TREC_LDS_MAX
#define MG_TREC_LDS_MAX (48 * 1024)
#endif
constexpr bool k_rigid_step1_built(unsigned f) {
    if (f >> RF_BITS) return false;
    if (f & RF_BOX) return f == (RF_UPZ | RF_LDS | RF_REC | RF_BOX);
    if ((f & RF_CREP) && (f & (RF_LDS | RF_REC))) return false;
    if ((f & RF_ATTR) && (f & RF_LDS)) return false;
    return !((f & RF_WIDE) && (f & RF_REC));   // the slot record: one-round launches only
}
// k_rigid_step<F, MAXC, MULTI>: F of RF_UPZ, RF_ATTR, RF_CREP
constexpr bool k_rigid_step_built(unsigned f, int maxc, bool multi) {
    return !(f & ~(RF_UPZ | RF_ATTR | RF_CREP)) && maxc == 8 && multi;
}
// blocks of 64 bodies, `cus` CUs; lds_bytes: the template records'; the others: is that MgRigidArgs member set
constexpr unsigned k_rigid_step1_form(bool upz, int blocks, int cus, size_t lds_bytes, bool slot_rec, bool attr_idx,
                                      bool crep, bool free_ids, bool box_only) {
    // wide: more waves than one resident round (4 SIMDs x 3 or 2 waves per CU). A reporting launch
    // keeps this threshold of the plain launches on purpose, although its wide build holds two waves
    // per SIMD: which bodies step in which form (and so every value) is the same with reporting on and off.
    const bool wide = blocks > cus * 4 * (upz ? MG_RIGID1_ROUND_WAVES : 2);
    const unsigned f = (upz ? RF_UPZ : 0) | (wide ? RF_WIDE : 0) | (attr_idx ? RF_ATTR : 0);
    // reporting, attractors: template records from global memory; reporting: the slot's indices from their arrays
    if (crep) return f | RF_CREP;
    const bool rec = slot_rec && !free_ids;
    const unsigned r = rec && !wide ? RF_REC : 0;
    if (attr_idx) return f | r;
    const bool fits = lds_bytes <= MG_TREC_LDS_MAX;
    if (upz && !wide && rec && fits && box_only) return RF_UPZ | RF_LDS | RF_REC | RF_BOX;
    return f | r | (fits ? RF_LDS : 0);
}
constexpr unsigned k_rigid_step_form(bool upz, bool attr_idx, bool crep) {
    return (upz ? RF_UPZ : 0) | (attr_idx ? RF_ATTR : 0) | (crep ? RF_CREP : 0);
}
// mg_last_rigid_form's public bits of a k_rigid_step1 form
constexpr int mg_rigid_form_public(unsigned f) {
    return (f & RF_WIDE ? MG_RIGID_FORM_WIDE : 0) | (f & RF_REC ? MG_RIGID_FORM_REC : 0) |
           (f & RF_BOX ? MG_RIGID_FORM_BOX : 0);
}

// ---- k_artic_chain_q (four lanes per chain) and k_artic_chain (one) ----
// EXT: applied wrenches; UNI: the launch's shared constants (MgArticArgs::uni); AFF: rows computed, not
// loaded (k_artic_chain only); FRC: DOF force rows
enum : unsigned { CF_EXT = 1, CF_UNI = 2, CF_AFF = 4, CF_FRC = 8, CF_BITS = 4 };
#ifndef MG_CHAIN_QUAD_MAX
#define MG_CHAIN_QUAD_MAX (64 * 1024)   // four lanes per chain up to this many lanes (one resident round)
#endif
constexpr bool k_artic_chain_built(int nl, unsigned f) {
    return nl >= 2 && nl <= 4 && !(f >> CF_BITS) && (!(f & CF_AFF) || (f & CF_UNI));
}
constexpr bool k_artic_chain_q_built(int nl, unsigned f) { return k_artic_chain_built(nl, f) && !(f & CF_AFF); }
struct MgChainForm { bool quad; unsigned f; };   // quad: k_artic_chain_q
constexpr MgChainForm mg_chain_form(int na, bool ext, bool uni, bool aff, bool dof_frc) {
    const bool quad = (long)na * 4 <= MG_CHAIN_QUAD_MAX;
    return {quad, (ext ? CF_EXT : 0) | (uni ? CF_UNI : 0) | (!quad && uni && aff ? CF_AFF : 0) | (dof_frc ? CF_FRC : 0)};
}

// ---- k_env_step (coupled envs) and k_artic_lanes (uncoupled articulations) ----
// MAXL links in G lanes: 32 in 64 (one env per wavefront), 16 or 4 in 16. ATTR: attractors; FRC: DOF force
// rows; SENS: contact moments (force sensors); CREP: contact reporting; JFR: joint friction
enum : unsigned { EF_ATTR = 1, EF_FRC = 2, EF_SENS = 4, EF_CREP = 8, EF_JFR = 16, EF_BITS = 5 };
enum : unsigned { LF_ATTR = 1, LF_FRC = 2, LF_JFR = 4, LF_BITS = 3 };
constexpr int mg_env_lanes(int maxl) { return maxl > 16 ? 64 : 16; }
constexpr bool mg_env_size_built(int maxl, int g, bool attr) {
    return (maxl == 32 || maxl == 16 || (maxl == 4 && !attr)) && g == mg_env_lanes(maxl);
}
constexpr bool k_env_step_built(int maxl, int g, unsigned f) {
    if ((f >> EF_BITS) || !mg_env_size_built(maxl, g, f & EF_ATTR)) return false;
    if ((f & (EF_SENS | EF_CREP | EF_JFR)) && !(f & EF_FRC)) return false;
    return !(f & EF_JFR) || !(f & (EF_ATTR | EF_SENS | EF_CREP));
}
constexpr bool k_artic_lanes_built(int maxl, int g, unsigned f) {
    if ((f >> LF_BITS) || !mg_env_size_built(maxl, g, f & LF_ATTR)) return false;
    return !(f & LF_JFR) || (f & (LF_ATTR | LF_FRC)) == LF_FRC;
}
// the object that compiles a form: no form is compiled in two
enum MgEnvObject { MG_ENV_OBJ_MAIN, MG_ENV_OBJ_SENS, MG_ENV_OBJ_CREP, MG_ENV_OBJ_JFR };
constexpr MgEnvObject k_env_step_object(unsigned f) {
    return f & EF_JFR ? MG_ENV_OBJ_JFR : f & EF_CREP ? MG_ENV_OBJ_CREP : f & EF_SENS ? MG_ENV_OBJ_SENS : MG_ENV_OBJ_MAIN;
}
constexpr MgEnvObject k_artic_lanes_object(unsigned f) { return f & LF_JFR ? MG_ENV_OBJ_JFR : MG_ENV_OBJ_MAIN; }
struct MgSizedForm { int maxl; unsigned f; };
// 16 lanes up to 16 links and 16 velocity slots, else 64
constexpr bool mg_env_wide(int nl, int slots) { return nl > 16 || slots > 16; }
// slots: DOFs, the floating root's 6, 6 per free body. With attractors the 16-link build steps
// small envs too: it shares only the carry and contact-table records with k_env_np<4>, whose layout
// depends on G alone. SENS, CREP and JFR builds write DOF forces too; a JFR group has none of the others.
constexpr MgSizedForm k_env_step_form(int nl, int ndof, bool floating, int slots, bool attr_idx, bool dof_frc,
                                      bool ctorque, bool crep, bool jfr) {
    const bool small = nl <= 4 && ndof <= 4 && !floating;
    const int maxl = mg_env_wide(nl, slots) ? 32 : small && !attr_idx ? 4 : 16;
    if (jfr) return {maxl, EF_FRC | EF_JFR};
    const unsigned a = attr_idx ? EF_ATTR : 0;
    if (crep) return {maxl, a | EF_FRC | EF_CREP | (ctorque ? EF_SENS : 0)};
    if (ctorque) return {maxl, a | EF_FRC | EF_SENS};
    return {maxl, a | (dof_frc ? EF_FRC : 0)};
}
constexpr MgSizedForm k_artic_lanes_form(int nl, int ndof, bool attr_idx, bool dof_frc, bool jfr) {
    const int plain = mg_env_wide(nl, ndof) ? 32 : nl <= 4 && ndof <= 4 ? 4 : 16;
    if (jfr) return {plain, LF_FRC | LF_JFR};
    if (attr_idx) return {plain == 32 ? 32 : 16, LF_ATTR | (dof_frc ? LF_FRC : 0)};
    return {plain, dof_frc ? LF_FRC : 0};
}

// ---- k_pile_step ----
enum : unsigned { PF_CREP = 1, PF_BITS = 1 };
constexpr bool k_pile_step_built(unsigned f) { return !(f >> PF_BITS); }
constexpr unsigned k_pile_step_form(bool crep) { return crep ? PF_CREP : 0; }

// ---- the choosers: which kernel, at which size and form, a launch runs ----
// what only a simulate knows: the +Z ground basis, an applied wrench is pending, the step writes
// refreshed rows (the fused refresh or the host stage), the device's compute units
struct MgRun { bool upz, ext, step_out; int cus; };
constexpr bool mg_step_is_upz(const float n[3], const float t1[3], const float t2[3]) {
    return n[0] == 0.0f && n[1] == 0.0f && n[2] == 1.0f && t1[0] == 0.0f && t1[1] == 1.0f && t1[2] == 0.0f &&
           t2[0] == -1.0f && t2[1] == 0.0f && t2[2] == 0.0f;
}
// the launches' size limits (mg_internal.h asserts them equal to MG_MAX_LINKS, MG_ENV_SLOTS_WIDE, MG_MAX_CONTACTS)
enum { MG_FORM_MAX_LINKS = 32, MG_FORM_SLOTS_WIDE = 32, MG_FORM_MAX_CONTACTS = 8 };
#ifndef MG_CHAIN_AFF
#define MG_CHAIN_AFF 1
#endif

// the kernel ids (mg_debug_step_builds reports them: include/migym.h MG_KERNEL_*)
enum MgKernel {
    MG_K_NONE = 0, MG_K_RIGID_STEP1 = MG_KERNEL_RIGID_STEP1, MG_K_RIGID_STEP = MG_KERNEL_RIGID_STEP,
    MG_K_ARTIC_CHAIN = MG_KERNEL_ARTIC_CHAIN, MG_K_ARTIC_CHAIN_Q = MG_KERNEL_ARTIC_CHAIN_Q,
    MG_K_ARTIC_LANES = MG_KERNEL_ARTIC_LANES, MG_K_ENV_STEP = MG_KERNEL_ENV_STEP, MG_K_PILE_STEP = MG_KERNEL_PILE_STEP
};
// kernel<size, form>: size is NL (the chains), MAXL in mg_env_lanes(MAXL) lanes (k_env_step,
// k_artic_lanes), MAXC (k_rigid_step), else 0. np: k_env_step's narrow phase k_env_np<4 | 16 | 32>.
// aff, out_aff: MgArticArgs' values of the chains (rows, refreshed rows computed, not loaded).
// kernel MG_K_NONE: the launch has no such part (a free-body half without bodies); built false: no such build.
struct MgBuild {
    int kernel = MG_K_NONE, size = 0;
    unsigned form = 0;
    int np = 0;
    bool aff = false, out_aff = false;
    bool built = false;
};
// the free bodies' two launches: single-shape bodies (k_rigid_step1), then the others (k_rigid_step)
struct MgBuilds {
    MgBuild one, multi;
    constexpr bool built() const { return (one.kernel || multi.kernel) && (!one.kernel || one.built) && (!multi.kernel || multi.built); }
};

// the routed features a build carries (EF_* by value: mg_route.h's RT_*)
constexpr unsigned mg_build_carried(const MgBuild& b) {
    const unsigned f = b.form;
    switch (b.kernel) {
        case MG_K_RIGID_STEP1:
        case MG_K_RIGID_STEP: return (f & RF_ATTR ? EF_ATTR : 0) | (f & RF_CREP ? EF_CREP : 0);
        case MG_K_ARTIC_CHAIN:
        case MG_K_ARTIC_CHAIN_Q: return f & CF_FRC ? EF_FRC : 0;
        case MG_K_ARTIC_LANES: return (f & LF_ATTR ? EF_ATTR : 0) | (f & LF_FRC ? EF_FRC : 0) | (f & LF_JFR ? EF_JFR : 0);
        case MG_K_ENV_STEP: return f;
        case MG_K_PILE_STEP: return f & PF_CREP ? EF_CREP : 0;
        default: return 0;
    }
}
constexpr unsigned mg_build_carried(const MgBuilds& b) {
    return (b.one.kernel ? mg_build_carried(b.one) : ~0u) & (b.multi.kernel ? mg_build_carried(b.multi) : ~0u) &
           (b.one.kernel || b.multi.kernel ? ~0u : 0u);
}

// The optional members of its argument block a build's kernel dereferences unconditionally:
// attr_idx and attr; dof_frc; ctorque; crep, crep_n and crep_body; uni; slot_rec; ext (the chains'
// EXT forms: the other kernels test ext themselves). The builders fill exactly these, the
// launchers launch nothing that lacks one.
enum : unsigned { MG_NEED_ATTR = 1, MG_NEED_DOF_FRC = 2, MG_NEED_CTORQUE = 4, MG_NEED_CREP = 8, MG_NEED_UNI = 16,
                  MG_NEED_SLOT_REC = 32, MG_NEED_EXT = 64 };
constexpr unsigned mg_build_needs(const MgBuild& b) {
    const unsigned f = b.form;
    switch (b.kernel) {
        case MG_K_RIGID_STEP1:
            return (f & RF_ATTR ? MG_NEED_ATTR : 0) | (f & RF_CREP ? MG_NEED_CREP : 0) | (f & RF_REC ? MG_NEED_SLOT_REC : 0);
        case MG_K_RIGID_STEP: return (f & RF_ATTR ? MG_NEED_ATTR : 0) | (f & RF_CREP ? MG_NEED_CREP : 0);
        case MG_K_ARTIC_CHAIN:
        case MG_K_ARTIC_CHAIN_Q:
            return (f & CF_EXT ? MG_NEED_EXT : 0) | (f & CF_UNI ? MG_NEED_UNI : 0) | (f & CF_FRC ? MG_NEED_DOF_FRC : 0);
        case MG_K_ARTIC_LANES: return (f & LF_ATTR ? MG_NEED_ATTR : 0) | (f & LF_FRC ? MG_NEED_DOF_FRC : 0);
        case MG_K_ENV_STEP:
            return (f & EF_ATTR ? MG_NEED_ATTR : 0) | (f & EF_FRC ? MG_NEED_DOF_FRC : 0) | (f & EF_SENS ? MG_NEED_CTORQUE : 0) |
                   (f & EF_CREP ? MG_NEED_CREP : 0);
        case MG_K_PILE_STEP: return f & PF_CREP ? MG_NEED_CREP : 0;
        default: return 0;
    }
}
// a launcher's host check: `b` is a build of `kernel` (or of `kernel2`) and `have`, the MG_NEED_* of the
// block's members that are set, holds all it needs
constexpr bool mg_build_fits(const MgBuild& b, unsigned have, int kernel, int kernel2 = MG_K_NONE) {
    return b.built && (b.kernel == kernel || (kernel2 && b.kernel == kernel2)) && !(mg_build_needs(b) & ~have);
}

// An uncoupled articulation group's launch of `count` instances. A serial chain of 2 to 4 links
// without attractor and joint friction steps in the chain kernels (four lanes per chain up to
// MG_CHAIN_QUAD_MAX lanes), everything else in k_artic_lanes. uni: the group's shared constants
// (chains only). aff, out_aff: the group's rows / refreshed rows are affine; a split launch loads
// them. The computed-row form needs the refreshed rows computed too when the step writes them.
constexpr MgBuild mg_choose_artic(int nl, int ndof, bool fixed_base, bool chain, bool uni_mass, bool aff, bool out_aff,
                                  bool split, int count, unsigned feat, const MgRun& run) {
    MgBuild b;
    const bool attr = feat & EF_ATTR, frc = feat & EF_FRC, jfr = feat & EF_JFR;
    if (!jfr && !attr && chain && nl >= 2 && nl <= 4) {   // serial chain, one DOF per moving link
        b.aff = !split && aff;
        b.out_aff = !split && out_aff;
        const MgChainForm c = mg_chain_form(count, run.ext, uni_mass, MG_CHAIN_AFF && b.aff && (!run.step_out || b.out_aff), frc);
        b.kernel = c.quad ? MG_K_ARTIC_CHAIN_Q : MG_K_ARTIC_CHAIN;
        b.size = nl;
        b.form = c.f;
        b.built = c.quad ? k_artic_chain_q_built(nl, c.f) : k_artic_chain_built(nl, c.f);
        return b;
    }
    const MgSizedForm k = k_artic_lanes_form(nl, ndof, attr, frc, jfr);
    b.kernel = MG_K_ARTIC_LANES;
    b.size = k.maxl;
    b.form = k.f;
    b.built = fixed_base && nl <= MG_FORM_MAX_LINKS && ndof <= MG_FORM_SLOTS_WIDE && k_artic_lanes_built(k.maxl, mg_env_lanes(k.maxl), k.f);
    return b;
}

// A coupled group's launch: nl, ndof, floating of its articulation template (0: none), max_free free
// bodies per env. Velocity slots: DOFs, the floating root's 6, 6 per free body. The narrow phase's
// size follows the env alone (an attractor's 16-link step runs after k_env_np<4>).
constexpr MgBuild mg_choose_env(int nl, int ndof, bool floating, int max_free, unsigned feat, const MgRun&) {
    MgBuild b;
    const int slots = ndof + (floating ? 6 : 0) + 6 * max_free;
    const MgSizedForm k = k_env_step_form(nl, ndof, floating, slots, feat & EF_ATTR, feat & EF_FRC, feat & EF_SENS,
                                          feat & EF_CREP, feat & EF_JFR);
    b.kernel = MG_K_ENV_STEP;
    b.size = k.maxl;
    b.form = k.f;
    b.np = mg_env_wide(nl, slots) ? 32 : nl <= 4 && ndof <= 4 && !floating ? 4 : 16;
    b.built = nl <= MG_FORM_MAX_LINKS && slots <= MG_FORM_SLOTS_WIDE && k_env_step_built(k.maxl, mg_env_lanes(k.maxl), k.f);
    return b;
}

constexpr MgBuild mg_choose_pile(unsigned feat, const MgRun&) {
    MgBuild b;
    b.kernel = MG_K_PILE_STEP;
    b.form = k_pile_step_form(feat & EF_CREP);
    b.built = k_pile_step_built(b.form);
    return b;
}

// The free bodies: nf1 single-shape ones in blocks of 64, then nf - nf1 others. lds_bytes: the
// template records'; slot_rec: the layout holds the packed slot record (a reporting launch reads
// the slot's indices from their arrays instead); box_only: MgLayout::free_flags[0].
constexpr MgBuilds mg_choose_free(int nf1, int nf, size_t lds_bytes, bool slot_rec, bool box_only, unsigned feat,
                                  const MgRun& run) {
    MgBuilds b;
    const bool attr = feat & EF_ATTR, crep = feat & EF_CREP;
    if (nf1 > 0) {
        b.one.kernel = MG_K_RIGID_STEP1;
        b.one.form = k_rigid_step1_form(run.upz, (nf1 + 63) / 64, run.cus, lds_bytes, slot_rec && !crep, attr, crep, false, box_only);
        b.one.built = k_rigid_step1_built(b.one.form);
    }
    if (nf > nf1) {
        b.multi.kernel = MG_K_RIGID_STEP;
        b.multi.size = MG_FORM_MAX_CONTACTS;
        b.multi.form = k_rigid_step_form(run.upz, attr, crep);
        b.multi.built = k_rigid_step_built(b.multi.form, b.multi.size, true);
    }
    return b;
}
