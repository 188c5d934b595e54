// What the three elementwise-norm families share (norm.hip: ResNet InstanceNorm + activation + fold; norm_ex.hip: U-Net dual
// activation / slices / dropout; prelu.hip: V-Net InstanceNorm + PReLU + residual): the 8-channel access helpers next to
// unpack_bf8 / add_bf8 / pack_bf8 of common.hpp, the second level of the two-level pixel reductions, and the host-side launch
// arithmetic. The accumulation loops of the reduce kernels are NOT shared: how many pixels each keeps in flight, and whether two
// pixels are added before or after the accumulator, differ on purpose, and their order is part of the result.
#pragma once
#include "internal.hpp"
#include <type_traits>

// eight consecutive floats (per-channel statistics, slopes, sums) as two 16-byte loads
__device__ __forceinline__ void load8(float* f, const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
// channel group c8 of pixel `pix` of a strided bf16 view (cs channels per pixel, the view starts at channel co)
__device__ __forceinline__ void view8(float* f, const unsigned short* t, size_t pix, int cs, int co, int c8) {
  unpack_bf8(f, *reinterpret_cast<const uint4*>(t + pix * cs + co + c8 * 8));
}

// Second level of a two-level reduction workgroup: 256 threads = COLS 8-channel columns x ROWS = 256/COLS pixel rows, grid
// (chunks, N, ceil(C8/COLS)). Every thread hands in its R sums over its pixels, acc = R arrays of 8 floats; COLS*R*8 threads then
// add them over the rows IN ROW ORDER and store them at partial[n][blockIdx.x][r][C8 * 8] of [N][chunks][R][C]. (The sums come as the
// separate arrays the kernels accumulate in: handed over as one [R][8] array the reduce kernels allocated more registers.)
template <int ROWS, int COLS, int W, class... A>
__device__ __forceinline__ void row_fold(float (&red)[ROWS][COLS][W], float* partial, int n, int chunks, int C8,
                                         const A&... acc) {
  constexpr int R = sizeof...(A);
  static_assert(W == R * 8 + 1, "red is [ROWS][COLS][R*8+1]");
  const int tid = threadIdx.x;
  const int col = tid % COLS, row = tid / COLS;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int r = 0;
    ((red[row][col][8 * r++ + k] = acc[k]), ...);
  }
  __syncthreads();
  for (int o = tid; o < COLS * R * 8; o += 256) {
    const int cc = o / (R * 8), k = o - cc * (R * 8);
    const int ch8 = blockIdx.z * COLS + cc;
    if (ch8 < C8) {
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) sum += red[r][cc][k];
      float* out = partial + ((size_t)n * chunks + blockIdx.x) * R * C8 * 8;
      out[(k >> 3) * C8 * 8 + ch8 * 8 + (k & 7)] = sum;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// launch(std::integral_constant<int, COLS>) for the first COLS of the list that C8 reaches (the last one otherwise). The list is
// each launch site's own (norm_ex.hip has no 4 / 2, slice_stats no 32): that is behaviour, kept as it is.
template <int COLS, int... REST, class F>
static inline void norm_by_cols(int C8, F&& launch) {
  if constexpr (sizeof...(REST) == 0) launch(std::integral_constant<int, COLS>{});
  else if (C8 >= COLS) launch(std::integral_constant<int, COLS>{});
  else norm_by_cols<REST...>(C8, launch);
}
// log2(C8) when C8 is a power of two up to 256 (a grid stride of a multiple of 256 elements then keeps a thread on one channel
// group, and the pixel index is a shift), else -1
static inline int norm_c8_shift(int C8) {
  if (C8 <= 0 || C8 > 256 || (C8 & (C8 - 1))) return -1;
  int sh = 0;
  while ((1 << sh) < C8) ++sh;
  return sh;
}
// workgroups of a grid-stride loop of 256 threads over `elems` elements, `per_thread` of them each, at most `cap`
static inline unsigned norm_grid(long long elems, int cap, int per_thread = 1) {
  const long long bx = (elems + 256LL * per_thread - 1) / (256LL * per_thread);
  return (unsigned)(bx > cap ? cap : (bx < 1 ? 1 : bx));
}
