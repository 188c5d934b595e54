// Uniform cubic B-spline evaluation of a control-point lattice aligned with a patch (ganslate_hip.h states the
// definition): what the elastic gather (volsample.hip) and the bias field of the intensity chain (volsample.hip,
// volproc.hip) share. Float64, one IEEE operation per step, no contraction; D innermost, then H, W outermost.
#pragma once
#include "common.hpp"

// the interval j and the four uniform cubic B-spline weights of output index o on an axis of p voxels over G control
// points: f = (o (G - 3) - j (p - 1)) / (p - 1), one correctly rounded division of two exact integers
__device__ __forceinline__ int bspline_axis(int o, int p, int G, double B[4]) {
#pragma clang fp contract(off)
  const int num = o * (G - 3), den = p - 1;              // the host refused (p - 1) (G - 3) > INT_MAX
  int j = num / den;
  j = j > G - 4 ? G - 4 : j;
  const double f = __ddiv_rn((double)(num - j * den), (double)den);
  const double f2 = f * f;
  const double f3 = f2 * f;
  const double g = 1.0 - f;
  const double gg = g * g;
  const double t1 = 3.0 * f3;
  const double t2 = 6.0 * f2;
  const double t3 = 3.0 * f2;
  const double t4 = 3.0 * f;
  B[0] = __ddiv_rn(gg * g, 6.0);
  B[1] = __ddiv_rn((t1 - t2) + 4.0, 6.0);
  B[2] = __ddiv_rn(((t3 - t1) + t4) + 1.0, 6.0);
  B[3] = __ddiv_rn(f3, 6.0);
  return j;
}

__device__ __forceinline__ double dot4(const double B[4], double a0, double a1, double a2, double a3) {
#pragma clang fp contract(off)
  const double p0 = B[0] * a0;
  const double p1 = B[1] * a1;
  const double p2 = B[2] * a2;
  const double p3 = B[3] * a3;
  const double s1 = p0 + p1;
  const double s2 = s1 + p2;
  return s2 + p3;
}

// R of one lattice column: D innermost (Bz), then H (By). F: one component of the lattice at (j0, j1, column), in LDS or
// in global memory
__device__ __forceinline__ double lattice_R(const double* F, int G1, int G2, const double Bz[4], const double By[4]) {
  double q[4];
  const int sz = G1 * G2;
#pragma unroll
  for (int m = 0; m < 4; ++m) q[m] = dot4(Bz, F[m * G2], F[sz + m * G2], F[2 * sz + m * G2], F[3 * sz + m * G2]);
  return dot4(By, q[0], q[1], q[2], q[3]);
}

// one scalar lattice F[G0][G1][G2] (LDS or global memory) at output voxel o of a patch p: the per-voxel form
__device__ __forceinline__ double lattice_at(const double* F, const int G[3], const int o[3], const int p[3]) {
  double Bz[4], By[4], Bx[4], R[4];
  const int j0 = bspline_axis(o[0], p[0], G[0], Bz);
  const int j1 = bspline_axis(o[1], p[1], G[1], By);
  const int j2 = bspline_axis(o[2], p[2], G[2], Bx);
  const double* at = F + (j0 * G[1] + j1) * G[2] + j2;
#pragma unroll
  for (int n = 0; n < 4; ++n) R[n] = lattice_R(at + n, G[1], G[2], Bz, By);
  return dot4(Bx, R[0], R[1], R[2], R[3]);
}
