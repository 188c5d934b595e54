// Device-side preparation of multi-modal 2-D samples (data/multimodal_images.py, DeviceMultiModalImagePipeline): what the
// reference's ClearGrasp datasets do per modality on the host (projects/cleargrasp_depth_estimation/datasets/
// train_dataset.py:75-146, val_test_dataset.py:80-167) — the tensor resize transforms.Resize(load_size, BICUBIC), i.e.
// torch's bicubic interpolation without antialiasing (cubic convolution A = -0.75, align_corners = False), clamp to the
// modality's range, min-max to [-1, 1], the noise plane of domain B's RGB, the channel concat — as ONE launch per batch
// tensor [N, C, H, W] on decoded images resident in HBM as stored (uint8 or fp32).
//
// One GsImgStackItem per (sample, modality) in a device array; blockIdx.z is the descriptor, so every descriptor read is
// wave-uniform, blockIdx.y the output row (its four row taps are wave-uniform too), a thread one output pixel of all the
// modality's channels. The kernel computes no source coordinate: the four taps and weights of every output row and column
// come from tables built on the host in float64 and rounded once to fp32, so the result differs from the float64 value
// only by the roundings of the 16-tap sum. Per element, fp32:
//     r = sum_j wy[j] * (sum_i wx[i] * src[iy[j]][ix[i]][c])
//     v = min(max(r, lo), hi);  rescale: v = (v - lo) / (hi - lo), v = 2 v - 1      (clip_minmax's chain, csrc/volsample.hip)
//     noise_std > 0: v = min(max(v + noise_std * z(p), -1), 1)
// z depends on the descriptor's key and the pixel p = y * W + x alone, so the channels of a modality share one plane like
// the reference's `+ torch.normal(0, std, size=(H, W))`: Philox4x32-10 (counter (p, 0, 0, 0), key (key0, key1)) and
// Box-Muller on its first two words with the precise logf / cosf / sqrtf. A descriptor without a source writes c zero
// channels (the dummy channels of a val / test sample). Gather and store, HBM-bound: no LDS, no atomics; the stores of a
// wave are 64 consecutive floats of one output row.
#include <vector>
#include "common.hpp"
#include "philox.hpp"

namespace {
template <typename T>
__device__ __forceinline__ float tap_sum(const T* __restrict__ s, const int4 ix, const float4 wx, long long ps) {
  float r = wx.x * (float)s[ix.x * ps];
  r += wx.y * (float)s[ix.y * ps];
  r += wx.z * (float)s[ix.z * ps];
  r += wx.w * (float)s[ix.w * ps];
  return r;
}

template <typename T>
__device__ __forceinline__ float resample(const T* __restrict__ src, long long row_stride, long long ps, const int4 iy,
                                          const float4 wy, const int4 ix, const float4 wx) {
  float r = wy.x * tap_sum(src + iy.x * row_stride, ix, wx, ps);
  r += wy.y * tap_sum(src + iy.y * row_stride, ix, wx, ps);
  r += wy.z * tap_sum(src + iy.z * row_stride, ix, wx, ps);
  r += wy.w * tap_sum(src + iy.w * row_stride, ix, wx, ps);
  return r;
}

__global__ __launch_bounds__(256) void img_stack_kernel(const GsImgStackItem* __restrict__ items, float* __restrict__ out,
                                                        int C, int H, int W) {
  const GsImgStackItem& it = items[blockIdx.z];
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const long long plane = (long long)H * W;
  float* o = out + ((long long)it.item * C + it.c0) * plane + (long long)y * W + x;
  const int nc = it.c;
  if (it.src == nullptr) {
    for (int c = 0; c < nc; ++c) o[c * plane] = 0.f;
    return;
  }
  const int4 iy = reinterpret_cast<const int4*>(it.idx_y)[y];
  const float4 wy = reinterpret_cast<const float4*>(it.w_y)[y];
  const int4 ix = reinterpret_cast<const int4*>(it.idx_x)[x];
  const float4 wx = reinterpret_cast<const float4*>(it.w_x)[x];
  // HWC: a pixel's channels side by side; else planes of in_h * in_w
  const long long ps = it.hwc ? nc : 1;
  const long long cs = it.hwc ? 1 : (long long)it.in_h * it.in_w;
  const long long row_stride = (long long)it.in_w * ps;
  const float lo = it.lo, hi = it.hi, std = it.noise_std;
  const float span = __fsub_rn(hi, lo);
  float z = 0.f;
  if (std > 0.f) {
    unsigned r0, r1;
    philox_r01((unsigned)(y * W + x), 0u, 0u, 0u, it.key0, it.key1, r0, r1);
    z = normal_from(r0, r1);
  }
  for (int c = 0; c < nc; ++c) {
    float v = it.dtype == GS_IMG_U8
                  ? resample(static_cast<const unsigned char*>(it.src) + c * cs, row_stride, ps, iy, wy, ix, wx)
                  : resample(static_cast<const float*>(it.src) + c * cs, row_stride, ps, iy, wy, ix, wx);
    v = v < lo ? lo : v;                     // NaN stays NaN, like torch.clamp
    v = v > hi ? hi : v;
    if (it.rescale) {
      v = __fdiv_rn(__fsub_rn(v, lo), span);
      v = __fsub_rn(__fmul_rn(2.f, v), 1.f);
    }
    if (std > 0.f) {
      v = v + std * z;
      v = v < -1.f ? -1.f : v;
      v = v > 1.f ? 1.f : v;
    }
    o[c * plane] = v;
  }
}
}  // namespace

extern "C" int gs_img_stack_check(const GsImgStackItem* items, int32_t n, int32_t N, int32_t C, int32_t H, int32_t W) {
  GS_REQUIRE(items && n >= 1 && n <= 65535 && N >= 1 && C >= 1 && H >= 1 && H <= 65535 && W >= 1 &&
                 (int64_t)H * W < ((int64_t)1 << 31) && (int64_t)N * C <= ((int64_t)1 << 24),
             "gs_img_stack_check: bad argument (1 <= n <= 65535, 1 <= H <= 65535, H * W < 2^31, N * C <= 2^24)");
  std::vector<unsigned char> covered((size_t)N * C, 0);
  for (int32_t i = 0; i < n; ++i) {
    const GsImgStackItem& it = items[i];
    GS_REQUIRE(it.item >= 0 && it.item < N, "gs_img_stack_check: descriptor %d: batch item %d outside [0, %d)", i, it.item, N);
    GS_REQUIRE(it.c >= 1 && it.c0 >= 0 && it.c0 <= C - it.c,
               "gs_img_stack_check: descriptor %d: channels [%d, %d+%d) outside [0, %d)", i, it.c0, it.c0, it.c, C);
    if (it.src) {
      GS_REQUIRE(it.idx_y && it.w_y && it.idx_x && it.w_x, "gs_img_stack_check: descriptor %d: null tap table", i);
      GS_REQUIRE(it.in_h > 0 && it.in_w > 0 && (int64_t)it.in_h * it.in_w * it.c < ((int64_t)1 << 31),
                 "gs_img_stack_check: descriptor %d: source size %d x %d x %d (positive, below 2^31 elements)", i, it.in_h,
                 it.in_w, it.c);
      GS_REQUIRE(it.dtype == GS_IMG_U8 || it.dtype == GS_IMG_F32,
                 "gs_img_stack_check: descriptor %d: dtype %d (GS_IMG_U8 / GS_IMG_F32)", i, it.dtype);
      GS_REQUIRE(it.hi > it.lo, "gs_img_stack_check: descriptor %d: clip range [%g, %g] is empty", i, it.lo, it.hi);
      GS_REQUIRE(it.noise_std >= 0.f && it.noise_std < 1e30f, "gs_img_stack_check: descriptor %d: noise_std %g", i,
                 it.noise_std);
    }
    for (int32_t c = it.c0; c < it.c0 + it.c; ++c) {
      unsigned char& seen = covered[(size_t)it.item * C + c];
      GS_REQUIRE(!seen, "gs_img_stack_check: descriptor %d: channel %d of batch item %d is written twice", i, c, it.item);
      seen = 1;
    }
  }
  for (size_t k = 0; k < covered.size(); ++k)
    GS_REQUIRE(covered[k], "gs_img_stack_check: channel %d of batch item %d is written by no descriptor", (int)(k % C),
               (int)(k / C));
  return 0;
}

extern "C" int gs_img_stack(const GsImgStackItem* items, int32_t n, float* out, int32_t N, int32_t C, int32_t H,
                            int32_t W, void* stream) {
  GS_REQUIRE(items && out && n >= 1 && n <= 65535 && N >= 1 && C >= 1 && H >= 1 && H <= 65535 && W >= 1 &&
                 (int64_t)H * W < ((int64_t)1 << 31),
             "gs_img_stack: bad argument (1 <= n <= 65535, 1 <= H <= 65535, H * W < 2^31)");
  const dim3 grid((W + 255) / 256, H, n);
  hipLaunchKernelGGL(img_stack_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), items, out, C, H, W);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
