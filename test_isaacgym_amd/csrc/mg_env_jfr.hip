// mg_env_jfr.hip — the joint-friction builds (MG_ENV_OBJ_JFR, mg_forms.h): k_env_step for a
// coupled group whose envs hold a friction DOF, k_artic_lanes for the uncoupled instances that do. Friction
// together with attractors, force sensors or contact reporting is refused by mg_simulate.
#include "mg_env_kernels.h"

hipError_t mg_launch_env_step_jfr(const MgBuild& b, hipStream_t s, const MgStep& P, const MgEnvArgs& A) {
    return env_step_launch<MG_ENV_OBJ_JFR>(b, s, P, A);
}
hipError_t mg_launch_artic_lanes_jfr(const MgBuild& b, hipStream_t s, const MgStep& P, const MgArticArgs& A) {
    return artic_lanes_launch<MG_ENV_OBJ_JFR>(b, s, P, A);
}
