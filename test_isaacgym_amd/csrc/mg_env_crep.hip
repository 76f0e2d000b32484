// mg_env_crep.hip — k_env_step's reporting builds (MG_ENV_OBJ_CREP, mg_forms.h), with or without a
// contact torque row (the rigid contact list).
#include "mg_env_kernels.h"

hipError_t mg_launch_env_step_crep(const MgBuild& b, hipStream_t s, const MgStep& P, const MgEnvArgs& A) {
    return env_step_launch<MG_ENV_OBJ_CREP>(b, s, P, A);
}
