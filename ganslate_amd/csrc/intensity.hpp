// Intensity augmentation of a 3-D training patch (ganslate_hip.h states the definition): the per-voxel chain on the
// normalised value n in [0, 1] that gs_patch_augment_clip_minmax (volsample.hip) and gs_patch_zscore_intensity
// (volproc.hip) run just before their last step, and what both entries refuse. A step with neutral parameters is skipped,
// not evaluated, so a neutral descriptor changes no bit.
#pragma once
#include "bspline.hpp"
#include "philox.hpp"

// beta: the bias lattice at this voxel (unused when it.bias == 0); i: the voxel's linear index in the patch; c: its channel
__device__ __forceinline__ float intensity_chain(float n, const GsPatchIntensity& it, double beta, long long i, int c) {
#pragma clang fp contract(off)
  if (it.bias != 0.f) {
    const double pb = (double)it.bias * beta;
    const double md = 1.0 + pb;
    const float m = (float)md;
    n = n * m;
  }
  if (it.contrast != 1.f || it.brightness != 0.f) {
    const float a = n - 0.5f;
    const float b = a * it.contrast;
    const float d = b + 0.5f;
    n = d + it.brightness;
  }
  n = n < 0.f ? 0.f : n;                     // NaN stays NaN, as in clip_minmax
  n = n > 1.f ? 1.f : n;
  if (it.gamma != 1.f) n = powf(n, it.gamma);
  if (it.noise_std > 0.f) {
    unsigned r0, r1;
    philox_r01((unsigned)((unsigned long long)i & 0xffffffffull), (unsigned)((unsigned long long)i >> 32), (unsigned)c, 0u,
               it.key0, it.key1, r0, r1);
    const float s = it.noise_std * normal_from(r0, r1);
    n = n + s;
  }
  n = n < 0.f ? 0.f : n;
  n = n > 1.f ? 1.f : n;
  return n;
}

// What the intensity entries refuse on top of their base entries. *lattice: whether any of the C descriptors reads the
// bias lattice. The lattice checks are check_lattice's (volsample.hip), stated for the one scalar lattice here.
inline int check_intensity(const char* who, const GsPatchIntensity* it, int C, const int32_t* patch, const int32_t* bias_grid,
                           const double* bias_field, bool* lattice) {
  GS_REQUIRE(it, "%s: null intensity", who);
  *lattice = false;
  for (int c = 0; c < C; ++c) {
    const GsPatchIntensity& p = it[c];
    GS_REQUIRE(p.gamma > 0.f && p.gamma - p.gamma == 0.f, "%s: gamma %g of intensity %d must be positive and finite", who, p.gamma, c);
    GS_REQUIRE(p.contrast >= 0.f && p.contrast - p.contrast == 0.f, "%s: contrast %g of intensity %d must be finite and not negative",
               who, p.contrast, c);
    GS_REQUIRE(p.noise_std >= 0.f && p.noise_std - p.noise_std == 0.f,
               "%s: noise_std %g of intensity %d must be finite and not negative", who, p.noise_std, c);
    GS_REQUIRE(p.brightness - p.brightness == 0.f, "%s: brightness %g of intensity %d must be finite", who, p.brightness, c);
    GS_REQUIRE(p.bias > -1.f && p.bias < 1.f, "%s: bias %g of intensity %d must lie inside (-1, 1)", who, p.bias, c);
    if (p.bias != 0.f) *lattice = true;
  }
  GS_REQUIRE(!*lattice || (bias_grid && bias_field), "%s: a non-zero bias needs bias_grid and bias_field", who);
  GS_REQUIRE((bias_grid != nullptr) == (bias_field != nullptr), "%s: bias_grid and bias_field come together", who);
  if (bias_grid) {
    GS_REQUIRE(bias_grid[0] >= 4 && bias_grid[1] >= 4 && bias_grid[2] >= 4,
               "%s: the bias_grid lattice needs at least 4 control points per axis; got %d x %d x %d", who, bias_grid[0],
               bias_grid[1], bias_grid[2]);
    GS_REQUIRE((long long)bias_grid[0] * bias_grid[1] * bias_grid[2] <= GS_ELASTIC_MAX_POINTS,
               "%s: a bias_grid lattice of %d x %d x %d control points exceeds %d", who, bias_grid[0], bias_grid[1], bias_grid[2],
               GS_ELASTIC_MAX_POINTS);
    GS_REQUIRE(patch[0] >= 2 && patch[1] >= 2 && patch[2] >= 2,
               "%s: a patch under a bias_grid lattice needs at least 2 voxels per axis; got %d x %d x %d", who, patch[0], patch[1],
               patch[2]);
    for (int a = 0; a < 3; ++a)
      GS_REQUIRE((long long)(patch[a] - 1) * (bias_grid[a] - 3) <= 0x7fffffffLL,
                 "%s: patch axis %d of %d voxels is too long for %d bias_grid control points", who, a, patch[a], bias_grid[a]);
  }
  return 0;
}
