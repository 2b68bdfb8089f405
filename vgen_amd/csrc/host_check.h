// host_check.h — how an entry point refuses its arguments.  No HIP: common.h hands it to the kernels' translation units,
// the host-only planners (tapgemm_plan.cpp, norm_plan.cpp) include it alone.
#pragma once
#include <stdint.h>

#include "../../include/vgen_hip.h"

void vgen_set_error(const char* fmt, ...);   // cabi.cpp (a stand-alone planner driver brings its own)

#define VGEN_REQUIRE(cond, ...)       \
  do {                                \
    if (!(cond)) {                    \
      vgen_set_error(__VA_ARGS__);    \
      return VGEN_E_BADARG;           \
    }                                 \
  } while (0)

static inline bool vgen_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
