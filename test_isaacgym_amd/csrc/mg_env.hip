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

hipError_t mg_launch_artic_lanes(const MgStep& P, const MgArticArgs& A, const MgBuild& b, hipStream_t s) {
    if (A.na <= 0) return hipSuccess;
    if (!mg_build_fits(b, mg_args_have(A), MG_K_ARTIC_LANES)) return hipErrorInvalidValue;
    const hipError_t e = k_artic_lanes_object(b.form) == MG_ENV_OBJ_JFR ? mg_launch_artic_lanes_jfr(b, s, P, A)
                                                                        : artic_lanes_launch<MG_ENV_OBJ_MAIN>(b, s, P, A);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t mg_launch_env_step(const MgStep& P, const MgEnvArgs& A, const MgBuild& b, hipStream_t s) {
    if (A.ne <= 0) return hipSuccess;
    if (!mg_build_fits(b, mg_args_have(A), MG_K_ENV_STEP)) return hipErrorInvalidValue;
    const MgEnvObject obj = k_env_step_object(b.form);
    // per substep: the narrow phase (one env per wavefront), then the step
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
        if (b.np == 32) MG_LAUNCH((k_env_np<MG_MAX_LINKS, 64, 64>), dim3(A.ne), dim3(64), scene, s, P, B);
        else if (b.np == 4) MG_LAUNCH((k_env_np<4, G16, MG_NP_GN>), dim3(np_blocks), dim3(64), scene, s, P, B);
        else if (b.np == 16) MG_LAUNCH((k_env_np<16, G16, MG_NP_GN>), dim3(np_blocks), dim3(64), scene, s, P, B);
        else return hipErrorInvalidValue;
        const hipError_t e = obj == MG_ENV_OBJ_JFR    ? mg_launch_env_step_jfr(b, s, P, B)
                             : obj == MG_ENV_OBJ_CREP ? mg_launch_env_step_crep(b, s, P, B)
                             : obj == MG_ENV_OBJ_SENS ? mg_launch_env_step_sens(b, s, P, B)
                                                      : env_step_launch<MG_ENV_OBJ_MAIN>(b, s, P, B);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// floats of the per-env carry and contact-table records the launches above
// need (migym_capi.cpp allocates them per coupled env at the widest group's size)
extern "C" int mg_env_carry_floats(void) { return carry_n<64>(); }
extern "C" int mg_env_ctab_floats(void) { return ct_n<MG_ENV_MAXCT_WIDE>(); }
int mg_env_ctab_record_floats(int wide) { return wide ? ct_n<MG_ENV_MAXCT_WIDE>() : ct_n<MG_ENV_MAXCT>(); }
