// mg_env_sens.hip — k_env_step's contact-moment builds (MG_ENV_OBJ_SENS, mg_forms.h; force sensors,
// DESIGN.md §3.13). An object of their own so that the library builds in parallel.
#include "mg_env_kernels.h"

hipError_t mg_launch_env_step_sens(const MgBuild& b, hipStream_t s, const MgStep& P, const MgEnvArgs& A) {
    return env_step_launch<MG_ENV_OBJ_SENS>(b, s, P, A);
}
