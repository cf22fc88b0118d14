// switches.h -- host-only: the one reader of the TACO_* environment switches declared in switches.def, and the only file in
// csrc/ that reads the environment.  Nothing from HIP is included: a host compiler can compile this header alone (tests/test_switches_host.py).
//   sw_on<SW_X>()    PRESENT / NONZERO / UNLESS0 switches
//   sw_int<SW_X>()   INT switches (the table's default when the variable is unset)
//   sw_text<SW_X>()  TEXT switches (the string, or nullptr)
// Asking a switch for another type than its kind's does not compile.  What a caller does with the value -- range checks,
// sscanf, per-device or per-thread caching -- stays with the caller.
#pragma once
#include <cstdlib>

enum SwKind { SWK_PRESENT, SWK_NONZERO, SWK_UNLESS0, SWK_INT, SWK_TEXT };
enum SwRead { SWR_LIVE, SWR_ONCE };

enum Switch {
#define TACO_SWITCH(name, kind, dflt, read, effect) SW_##name,
#include "switches.def"
#undef TACO_SWITCH
  SW_COUNT
};

struct SwDecl {
  const char* env;
  SwKind kind;
  int dflt;
  SwRead read;
};
constexpr SwDecl kSwitches[SW_COUNT] = {
#define TACO_SWITCH(name, kind, dflt, read, effect) {"TACO_" #name, SWK_##kind, dflt, SWR_##read},
#include "switches.def"
#undef TACO_SWITCH
};

template <Switch S>
inline bool sw_on() {
  constexpr SwDecl d = kSwitches[S];
  static_assert(d.kind == SWK_PRESENT || d.kind == SWK_NONZERO || d.kind == SWK_UNLESS0, "sw_on: the table declares this switch INT or TEXT");
  static_assert(d.read == SWR_LIVE, "sw_on reads at every access");
  const char* e = getenv(d.env);
  if (d.kind == SWK_PRESENT) return e != nullptr;
  if (d.kind == SWK_NONZERO) return e && atoi(e) != 0;
  return !(e && atoi(e) == 0);
}

template <Switch S>
inline int sw_int() {
  constexpr SwDecl d = kSwitches[S];
  static_assert(d.kind == SWK_INT, "sw_int: the table does not declare this switch INT");
  auto read = [] {
    const char* e = getenv(kSwitches[S].env);
    return e ? atoi(e) : kSwitches[S].dflt;
  };
  if constexpr (d.read == SWR_ONCE) {
    static const int v = read();   // (thread-safe: a function-local static, one per switch)
    return v;
  }
  return read();
}

template <Switch S>
inline const char* sw_text() {
  constexpr SwDecl d = kSwitches[S];
  static_assert(d.kind == SWK_TEXT, "sw_text: the table does not declare this switch TEXT");
  static_assert(d.read == SWR_LIVE, "sw_text reads at every access");
  return getenv(d.env);
}
