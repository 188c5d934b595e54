// What mind.hip (images) and mind3d.hip (volumes) state once: the constants, the workgroup's sum, the rounding of a patch
// weight and the checks of an entry point. The kernels themselves stay one file per rank (DESIGN.md 4.7.1 says why).
#pragma once
#include "common.hpp"
#include <math.h>

#define MIND_EPS 1e-8f

// sum over the 256 threads of a workgroup, the four waves in index order; sh holds 4 floats
__device__ __forceinline__ float mind_block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[wv] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// The weight exp(-|q|_2 / sigma^2) of a patch tap at squared distance r2, rounded as the reference rounds it
// (projects/cleargrasp_depth_estimation/modules/old/cyclegan_losses_with_structure.py:126-135): the distance and the
// quotient in fp32, the exponential in double, the result stored as fp32.
static inline float mind_weight(int r2, float sigma) {
  const float sigma2 = (float)((double)sigma * (double)sigma);
  const float d = sqrtf((float)r2);
  const float e = -d / sigma2;
  return (float)exp((double)e);
}

static inline int mind_ceil_div(int n, int d) { return (n + d - 1) / d; }

// The checks every entry point makes after its pointers: the sizes the kernels are built for (region edge S, patch edge P)
// and positive extents
static inline int mind_check_sizes(const char* name, int S, int P, int32_t nl_size, int32_t patch_size, int32_t neighbor_size,
                                   float sigma, bool positive) {
  GS_REQUIRE(nl_size == S && patch_size == P && neighbor_size == 3,
             "%s: only non_local_region_size %d, patch_size %d, neighbor_size 3 are built (got %d, %d, %d)", name, S, P, nl_size,
             patch_size, neighbor_size);
  GS_REQUIRE(sigma > 0.f && positive, "%s: bad argument", name);
  return 0;
}
