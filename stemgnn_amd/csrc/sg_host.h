// Host-side boilerplate of every launcher: the early return on a HIP error, the 16-byte alignment predicate behind every
// choice of a float4 path, the launch-sizing division and the range check of an int index.  Host code only: nothing here
// reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SG_TRY(e)                                \
  do {                                           \
    hipError_t _e = (e);                         \
    if (_e != hipSuccess) return -(int)_e;       \
  } while (0)

static inline bool sg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 64-bit operands, a grid dimension out (layout.h has the int, host/device one of the tile formulas)
static inline int sg_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// a positive element count or grid size that an int index reaches
static inline bool sg_fits_int(long long v) { return v > 0 && v < (1ll << 31); }
