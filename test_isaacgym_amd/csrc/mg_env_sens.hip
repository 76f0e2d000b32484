// mg_env_sens.hip — the contact-moment builds of the coupled per-env step
// (k_env_step<..., SENS>): mg_env.hip compiled a second time
// for these instantiations alone, so that they build beside the others instead
// of lengthening the one translation unit the build already waits for.
#define MG_ENV_SENS_TU 1
#include "mg_env.hip"
