// Host-side helpers for the C ABI (error reporting, argument checks).  Launches go through hftt_launch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

void hftt_set_error(const char* fmt, ...);

#define HFTT_REQUIRE(cond, ...)            \
  do {                                     \
    if (!(cond)) {                         \
      hftt_set_error(__VA_ARGS__);         \
      return 1;                            \
    }                                      \
  } while (0)

static inline int hftt_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// workgroups of `block` threads over `work_items` for a grid-stride kernel: at least one, at most `cap`
static inline int grid_for(long work_items, int block, int cap = 4096) {
  long b = (work_items + block - 1) / block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
