// mg_env.hip — the launchers of the coupled per-env step and of the uncoupled articulations (kernels:
// mg_env_kernels.h), their plain and force-reporting builds (MG_ENV_OBJ_MAIN) and the per-env record sizes.
#include "mg_env_kernels.h"

#ifdef MG_ENV_PHASE_TIMING
extern "C" int mg_debug_env_phase(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_env_phase), sizeof(g_env_phase)) == hipSuccess ? 0 : -1;
}
extern "C" int mg_debug_env_phase_reset(void) {
    unsigned long long z[24] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_env_phase), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

hipError_t mg_launch_artic_lanes(const MgStep& P, const MgArticArgs& A, hipStream_t s) {
    if (A.na <= 0) return hipSuccess;
    if (!A.fixed_base || A.nl > MG_MAX_LINKS || A.ndof > MG_ENV_SLOTS_WIDE) return hipErrorNotSupported;
    // instances that hold a friction DOF or own an attractor (migym_capi.cpp lists them apart) step
    // here, also of a group that steps in k_artic_chain otherwise
    if (A.jfr && (A.attr_idx || !A.dof_frc)) return hipErrorNotSupported;
    if (!A.jfr && !A.attr_idx && A.chain && A.nl >= 2 && A.nl <= 4)   // serial chain, one DOF per moving link
        return mg_launch_artic_chain(P, A, s);
    const MgSizedForm k = k_artic_lanes_form(A.nl, A.ndof, A.attr_idx, A.dof_frc, A.jfr);
    const hipError_t e = k_artic_lanes_object(k.f) == MG_ENV_OBJ_JFR ? mg_launch_artic_lanes_jfr(k.maxl, k.f, s, P, A)
                                                                     : artic_lanes_launch<MG_ENV_OBJ_MAIN>(k.maxl, k.f, s, P, A);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t mg_launch_env_step(const MgStep& P, const MgEnvArgs& A, hipStream_t s) {
    if (A.ne <= 0) return hipSuccess;
    // velocity slots: DOFs, the floating root's 6, 6 per free body (at most MG_ENV_MAXF)
    const int slots = A.ndof + (A.floating ? 6 : 0) + 6 * A.max_free;
    if (A.nl > MG_MAX_LINKS || slots > MG_ENV_SLOTS_WIDE) return hipErrorNotSupported;
    const MgSizedForm k = k_env_step_form(A.nl, A.ndof, A.floating, slots, A.attr_idx, A.dof_frc, A.ctorque, A.crep, A.jfr);
    const MgEnvObject obj = k_env_step_object(k.f);
    // per substep: the narrow phase (one env per wavefront), then the step. The narrow phase's size follows
    // the env alone (an attractor's 16-link step after k_env_np<4>: tests/test_attractor_gpu.py)
    const bool wide = mg_env_wide(A.nl, slots);
    const bool small = A.nl <= 4 && A.ndof <= 4 && !A.floating;
    const int np_blocks = (A.ne + 64 / MG_NP_GN - 1) / (64 / MG_NP_GN);
    MgEnvArgs B = A;
    // k_env_np's LDS copy of the scene's shapes, shape boxes and hulls (B.nhull = -1: too large, read from global memory)
    size_t scene = ((size_t)A.nshape * (MG_SHAPE_STRIDE + MG_OBB_N) + (size_t)A.nhull) * sizeof(float);
#ifndef MG_NP_SCENE_LDS_MAX
#define MG_NP_SCENE_LDS_MAX (24 * 1024)
#endif
    if (scene > MG_NP_SCENE_LDS_MAX || A.nhull < 0) {
        B.nhull = -1;
        scene = 0;
    }
    for (int sub = 0; sub < P.substeps; ++sub) {
        B.sub = sub;
        B.last = sub == P.substeps - 1 ? 1 : 0;
        if (wide) MG_LAUNCH((k_env_np<MG_MAX_LINKS, 64, 64>), dim3(A.ne), dim3(64), scene, s, P, B);
        else if (small) MG_LAUNCH((k_env_np<4, G16, MG_NP_GN>), dim3(np_blocks), dim3(64), scene, s, P, B);
        else MG_LAUNCH((k_env_np<16, G16, MG_NP_GN>), dim3(np_blocks), dim3(64), scene, s, P, B);
        const hipError_t e = obj == MG_ENV_OBJ_JFR    ? mg_launch_env_step_jfr(k.maxl, k.f, s, P, B)
                             : obj == MG_ENV_OBJ_CREP ? mg_launch_env_step_crep(k.maxl, k.f, s, P, B)
                             : obj == MG_ENV_OBJ_SENS ? mg_launch_env_step_sens(k.maxl, k.f, s, P, B)
                                                      : env_step_launch<MG_ENV_OBJ_MAIN>(k.maxl, k.f, s, P, B);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// floats of the per-env carry and contact-table records the launches above
// need (migym_capi.cpp allocates them per coupled env at the widest group's size)
extern "C" int mg_env_carry_floats(void) { return carry_n<64>(); }
extern "C" int mg_env_ctab_floats(void) { return ct_n<MG_ENV_MAXCT_WIDE>(); }
int mg_env_ctab_record_floats(int wide) { return wide ? ct_n<MG_ENV_MAXCT_WIDE>() : ct_n<MG_ENV_MAXCT>(); }
