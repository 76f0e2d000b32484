// mg_env_jfr.hip — the joint-friction builds of the coupled per-env step and
// of the uncoupled lanes step (k_env_step<..., JFR>, k_artic_lanes<..., JFR>,
// DESIGN.md §3.15): mg_env.hip compiled once more for these instantiations
// alone, beside the others, as mg_env_sens.hip and mg_env_crep.hip do.
#define MG_ENV_JFR_TU 1
#include "mg_env.hip"
