// env.hpp -- the environment knobs of the host code (A/B runs, tests of rare paths).  Callers that read a knob once per process
// keep the value in a static at the call site:  static const int x = env_int("MIRT_...", default);
#pragma once

#include <cstdlib>
#include <cstring>

namespace mirt {

// The variable's value as an integer (atol), or `dflt` when it is not set.
inline long env_int(const char *name, long dflt)
{
    const char *e = getenv(name);
    return e ? atol(e) : dflt;
}

// The variable is set to exactly `value`.
inline bool env_is(const char *name, const char *value)
{
    const char *e = getenv(name);
    return e && !strcmp(e, value);
}

}  // namespace mirt
