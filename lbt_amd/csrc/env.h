// env.h -- the tuning knobs of the environment (host side; experiments: the defaults are the measured choice).
#pragma once
#include <cstdlib>

namespace lbt {

// An integer knob: atoi of the variable, dflt when it is unset. The caller decides whether it is read once
// per process (a function-local static) or at every call. Hidden: not part of the library's exports.
__attribute__((visibility("hidden"))) inline int getenv_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

}  // namespace lbt
