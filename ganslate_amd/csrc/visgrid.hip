// The logged image grid (ganslate/utils/trackers/utils.py process_visuals_for_logging + torchvision.utils.save_image) as
// one kernel: K visuals side by side along the width, the D slices of a volume stacked along the height, [-1, 1] -> bytes,
// gray replicated to RGB, HWC. The reference runs channel repeat, cat, permute, cat, (x + 1) / 2,
// mul(255).add_(0.5).clamp_(0, 255).permute.to(uint8) as separate fp32 passes and copies fp32 to the host.
//   out[s, row, k * W + x, ch] = byte(src_k[s, c0_k + (c_k == 3 ? ch : 0), z, y, x]),  row = z * H + y (all slices) or y
// Streaming: every source element that appears in the image is read once, every output byte written once, no scratch.
// A thread owns one pixel (four along x on the vector path: one float4 load per channel where the source line is 16-byte
// aligned, twelve output bytes as three words where the output is 4-byte aligned); a wave reads and writes a contiguous
// piece of a row. The visual, the sample and the slice come from blockIdx, so the table lookups are wave-uniform. The K
// pointers and channel offsets travel by value in the argument struct: no device allocation, no table upload.
// Nothing an argument holds can make a thread write outside `out`: a thread writes only the pixel(s) its index names,
// behind the bounds check on that index; the host rejects what the grid or the 32-bit row arithmetic cannot take.
#include "common.hpp"

#define VIS_THREADS 256
#define VIS_MAX_SRCS 16          // == GS_VIS_MAX_SRCS (include/ganslate_hip.h)

namespace {

struct VisArgs {
  const float* src[VIS_MAX_SRCS];
  int ctot[VIS_MAX_SRCS], c0[VIS_MAX_SRCS], c[VIS_MAX_SRCS];
  int K, n, D, H, W;
  int slice;                     // -1: all slices stacked; else that slice only
};

struct alignas(4) VisWords { uint32_t a, b, c; };     // four RGB pixels

// The roundings of the separate torch ops: add, halve (exact), multiply, add, clamp, truncate. hipcc contracts a * b + c to
// an fma by default; the pragma switches that off for this body, and the instructions keep their flags when it is inlined.
// fmaxf / fminf return the other operand for a NaN: NaN -> 0, +inf -> 255, -inf -> 0.
__device__ __forceinline__ uint32_t vis_byte(float v) {
#pragma clang fp contract(off)
  float t = v + 1.0f;
  t = t * 0.5f;
  t = t * 255.0f;
  t = t + 0.5f;
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return (uint32_t)(int)t;
}

template <bool VEC>
__global__ __launch_bounds__(VIS_THREADS) void visuals_grid_kernel(VisArgs a, uint8_t* __restrict__ out) {
  constexpr int V = VEC ? 4 : 1;
  const int wq = a.W / V;
  const int idx = blockIdx.x * VIS_THREADS + threadIdx.x;
  if (idx >= a.H * wq) return;
  const int y = idx / wq, x = (idx - y * wq) * V;
  const int s = blockIdx.z / a.K, k = blockIdx.z - s * a.K;
  const int z = a.slice < 0 ? (int)blockIdx.y : a.slice;
  const int row = a.slice < 0 ? z * a.H + y : y, rows = a.slice < 0 ? a.D * a.H : a.H;
  const int nc = a.c[k];
  const int64_t plane = (int64_t)a.H * a.W, cs = (int64_t)a.D * plane;
  const float* p = a.src[k] + ((int64_t)s * a.ctot[k] + a.c0[k]) * cs + (int64_t)z * plane + (int64_t)y * a.W + x;
  uint8_t* o = out + (((int64_t)s * rows + row) * ((int64_t)a.K * a.W) + (int64_t)k * a.W + x) * 3;
  if constexpr (VEC) {
    uint32_t b[3][4];
    const bool al = (reinterpret_cast<uintptr_t>(p) & 15) == 0;      // cs % 4 == 0: the same for every channel
    for (int ch = 0; ch < 3; ++ch) {
      if (ch < nc) {
        const float* q = p + ch * cs;
        float4 v;
        if (al) v = *reinterpret_cast<const float4*>(q);
        else { v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3]; }
        b[ch][0] = vis_byte(v.x); b[ch][1] = vis_byte(v.y); b[ch][2] = vis_byte(v.z); b[ch][3] = vis_byte(v.w);
      } else {
        for (int i = 0; i < 4; ++i) b[ch][i] = b[0][i];
      }
    }
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      VisWords w;                // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, little endian
      w.a = b[0][0] | b[1][0] << 8 | b[2][0] << 16 | b[0][1] << 24;
      w.b = b[1][1] | b[2][1] << 8 | b[0][2] << 16 | b[1][2] << 24;
      w.c = b[2][2] | b[0][3] << 8 | b[1][3] << 16 | b[2][3] << 24;
      *reinterpret_cast<VisWords*>(o) = w;
    } else {
      for (int i = 0; i < 4; ++i)
        for (int ch = 0; ch < 3; ++ch) o[i * 3 + ch] = (uint8_t)b[ch][i];
    }
  } else {
    const uint32_t r = vis_byte(p[0]);
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)(nc == 3 ? vis_byte(p[cs]) : r);
    o[2] = (uint8_t)(nc == 3 ? vis_byte(p[2 * cs]) : r);
  }
}

}  // namespace

extern "C" int gs_visuals_grid_u8(const float* const* src, const int32_t* ctot, const int32_t* c0, const int32_t* c,
                                  int32_t K, int32_t n, int32_t N, int32_t D, int32_t H, int32_t W, int32_t slice,
                                  uint8_t* out, void* stream) {
  GS_REQUIRE(src && ctot && c0 && c && out, "gs_visuals_grid_u8: null argument");
  GS_REQUIRE(K >= 1 && K <= VIS_MAX_SRCS, "gs_visuals_grid_u8: K must lie in [1, %d]; got %d", VIS_MAX_SRCS, K);
  GS_REQUIRE(N >= 1 && n >= 1 && n <= N, "gs_visuals_grid_u8: n must lie in [1, N]; got n %d, N %d", n, N);
  GS_REQUIRE(D >= 1 && H >= 1 && W >= 1, "gs_visuals_grid_u8: D, H, W must be >= 1");
  GS_REQUIRE(slice >= -1 && slice < D, "gs_visuals_grid_u8: slice must be -1 or lie in [0, D); got %d", slice);
  GS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && (int64_t)D * H < ((int64_t)1 << 31) &&
             (int64_t)K * W < ((int64_t)1 << 31), "gs_visuals_grid_u8: H * W, D * H and K * W must be < 2^31");
  GS_REQUIRE(D <= 65535 && (int64_t)n * K <= 65535, "gs_visuals_grid_u8: D and n * K must be <= 65535 (grid)");
  VisArgs a = {};
  for (int k = 0; k < K; ++k) {
    GS_REQUIRE(src[k], "gs_visuals_grid_u8: src[%d] is null", k);
    GS_REQUIRE(c[k] == 1 || c[k] == 3, "gs_visuals_grid_u8: c[%d] must be 1 or 3; got %d", k, c[k]);
    GS_REQUIRE(c0[k] >= 0 && ctot[k] >= 1 && c0[k] <= ctot[k] - c[k],
               "gs_visuals_grid_u8: channels [%d, %d) of visual %d lie outside its %d channels", c0[k], c0[k] + c[k], k,
               ctot[k]);
    a.src[k] = src[k]; a.ctot[k] = ctot[k]; a.c0[k] = c0[k]; a.c[k] = c[k];
  }
  a.K = K; a.n = n; a.D = D; a.H = H; a.W = W; a.slice = slice;
  const bool vec = W % 4 == 0;
  const int per = H * (W / (vec ? 4 : 1));
  const dim3 grid((per + VIS_THREADS - 1) / VIS_THREADS, slice < 0 ? D : 1, n * K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(visuals_grid_kernel<true>, grid, dim3(VIS_THREADS), 0, st, a, out);
  else hipLaunchKernelGGL(visuals_grid_kernel<false>, grid, dim3(VIS_THREADS), 0, st, a, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
