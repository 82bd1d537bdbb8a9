// capi_knobs.cpp -- the one place that reads the process environment: knobs.hpp's reader over the C library's getenv.  WHICH
// variables exist, their defaults and clamps is knobs.def's; what follows from them is the plans' (dense_plan.hpp, knn_plan.hpp).
// The environment is read when a context is created (skl_ctx_create), when it is asked to look again (skl_ctx_reload_env) and,
// in the A/B build, at every API entry (ctx_bind) -- never on the launch path.
#include "capi_internal.hpp"

#include <cstdlib>

static const char *from_environment(const char *name) { return getenv(name); }

Knobs read_knobs() { return knobs_from(from_environment); }

#ifdef SKL_AB
int ab_forced_log_variant() { return knobs_from(from_environment).force_log_variant; }   // -2: not forced
#endif
