// mg_env_crep.hip — the reporting builds of the coupled per-env step
// (k_env_step<..., CREP>, the rigid contact list): mg_env.hip
// compiled once more for these instantiations alone, beside the others, as
// mg_env_sens.hip does for the contact-moment builds.
#define MG_ENV_CREP_TU 1
#include "mg_env.hip"
