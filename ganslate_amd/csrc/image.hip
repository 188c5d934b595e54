// Network boundary: NCHW fp32 images (the reference's `visuals`, cyclegan.py:39,84-90) <-> NHWC bf16
// activations with the channel count padded to a multiple of 8, plus the gradients of both conversions
// (tanh' of resnet2d.py:65 and the ReflectionPad2d adjoint of resnet2d.py:24 folded in).
#include "common.hpp"

__global__ __launch_bounds__(256) void image_to_act_kernel(const float* img, unsigned short* act, int C, long long hw,
                                                           int Cp) {
  const int n = blockIdx.y;
  const float* in = img + (size_t)n * C * hw;
  unsigned short* out = act + (size_t)n * hw * Cp;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x)
    store_bf_lanes(out + (size_t)p * Cp, Cp, [&](int c) { return c < C ? in[(size_t)c * hw + p] : 0.f; });
}

__global__ __launch_bounds__(256) void act_to_image_kernel(const unsigned short* act, float* img, int C, long long hw,
                                                           int Cp, int act_kind) {
  const int n = blockIdx.y;
  const unsigned short* in = act + (size_t)n * hw * Cp;
  float* out = img + (size_t)n * C * hw;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x)
    for (int c = 0; c < C; ++c) out[(size_t)c * hw + p] = apply_act(bf2f(in[(size_t)p * Cp + c]), act_kind, 0.f);
}

__global__ __launch_bounds__(256) void act_to_image_bwd_kernel(const float* g_img, const float* out_img,
                                                               unsigned short* g_act, int C, long long hw, int Cp,
                                                               int act_kind) {
  const int n = blockIdx.y;
  const float* gi = g_img + (size_t)n * C * hw;
  const float* oi = out_img ? out_img + (size_t)n * C * hw : nullptr;
  unsigned short* out = g_act + (size_t)n * hw * Cp;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x)
    store_bf_lanes(out + (size_t)p * Cp, Cp, [&](int c) {
      float v = 0.f;
      if (c < C) {
        v = gi[(size_t)c * hw + p];
        if (oi) v *= act_grad_from_out(oi[(size_t)c * hw + p], act_kind, 0.f);
      }
      return v;
    });
}

__global__ __launch_bounds__(256) void image_to_act_bwd_kernel(const unsigned short* g_pad, float* g_img, int C, int D,
                                                               int H, int W, int Cp, int fold, int mode,
                                                               int accumulate) {
  const int n = blockIdx.y;
  const int fd = D > 1 ? fold : 0;
  const int Dp = D + 2 * fd, Hp = H + 2 * fold, Wp = W + 2 * fold;
  const unsigned short* gp = g_pad + (size_t)n * Dp * Hp * Wp * Cp;
  const long long hw = (long long)D * H * W;
  float* out = g_img + (size_t)n * C * hw;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x) {
    const long long zi = p / W;
    const int iw = (int)(p - zi * W);
    const int iz = (int)(zi / H), ih = (int)(zi - (long long)iz * H);
    int ds[8], hs[8], ws[8];
    const int nd = fold_sources(ds, iz, D, fd, mode);
    const int nh = fold_sources(hs, ih, H, fold, mode);
    const int nw = fold_sources(ws, iw, W, fold, mode);
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int e = 0; e < nd; ++e)
        for (int a = 0; a < nh; ++a)
          for (int b = 0; b < nw; ++b) s += bf2f(gp[(((size_t)ds[e] * Hp + hs[a]) * Wp + ws[b]) * Cp + c]);
      if (accumulate) out[(size_t)c * hw + p] += s; else out[(size_t)c * hw + p] = s;
    }
  }
}

static inline dim3 img_grid(long long hw, int N) {
  long long bx = (hw + 255) / 256;
  if (bx > 1024) bx = 1024;
  return dim3((unsigned)bx, N);
}

extern "C" int gs_image_to_act(const float* img, void* act, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                               void* stream) {
  GS_REQUIRE(img && act && N > 0 && C > 0 && Cp >= C && (Cp & 7) == 0, "gs_image_to_act: bad argument");
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(image_to_act_kernel, img_grid(hw, N), dim3(256), 0, static_cast<hipStream_t>(stream), img,
                     static_cast<unsigned short*>(act), C, hw, Cp);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_act_to_image(const void* act, float* img, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                               int32_t act_kind, void* stream) {
  GS_REQUIRE(img && act && N > 0 && C > 0 && Cp >= C, "gs_act_to_image: bad argument");
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(act_to_image_kernel, img_grid(hw, N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(act), img, C, hw, Cp, act_kind);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_act_to_image_backward(const float* g_img, const float* out_img, void* g_act, int32_t N, int32_t C,
                                        int32_t H, int32_t W, int32_t Cp, int32_t act_kind, void* stream) {
  GS_REQUIRE(g_img && g_act && N > 0 && C > 0 && Cp >= C && (Cp & 7) == 0, "gs_act_to_image_backward: bad argument");
  GS_REQUIRE(act_kind == GS_ACT_NONE || out_img, "gs_act_to_image_backward: activation needs the forward output");
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(act_to_image_bwd_kernel, img_grid(hw, N), dim3(256), 0, static_cast<hipStream_t>(stream), g_img,
                     act_kind == GS_ACT_NONE ? nullptr : out_img, static_cast<unsigned short*>(g_act), C, hw, Cp,
                     act_kind);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_image_to_act_backward(const void* g_pad, float* g_img, int32_t N, int32_t C, int32_t D, int32_t H,
                                        int32_t W, int32_t Cp, int32_t fold, int32_t fold_mode, int32_t accumulate,
                                        void* stream) {
  GS_REQUIRE(g_pad && g_img && N > 0 && C > 0 && Cp >= C && D > 0, "gs_image_to_act_backward: bad argument");
  GS_REQUIRE(fold == 0 || fold_mode == GS_BORDER_REFLECT || (fold_mode == GS_BORDER_REPLICATE && fold <= 3),
             "gs_image_to_act_backward: fold must be reflect, or replicate with fold <= 3");
  GS_REQUIRE(fold == 0 || fold_mode != GS_BORDER_REFLECT || (H > fold && W > fold && (D == 1 || D > fold)),
             "gs_image_to_act_backward: a reflect fold needs every folded extent > fold");
  const long long hw = (long long)D * H * W;
  hipLaunchKernelGGL(image_to_act_bwd_kernel, img_grid(hw, N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(g_pad), g_img, C, D, H, W, Cp, fold, fold_mode, accumulate);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- channel sources ------------------------------------------------------------------------------------------------------
// Up to GS_CAT_MAX_SRCS image tensors side by side along the channel axis, each a channel window of a dense [N, C, S] fp32
// tensor: N blocks of channels * S contiguous floats, `stride` floats from one sample to the next, `ptr` at the window's first
// element (c0 * S floats into the tensor). torch.cat([fake_Bt, real_A[:, guide]], dim=1), real_B[:, tB] and the conditional
// discriminator's torch.cat([real_A, fake_B], dim=1) (two whole tensors, pix2pix.py:70,80) -> bf16 activation in one pass, no
// concatenated or sliced tensor in memory. A window base is in general not 16-byte aligned (odd S): every
// source read is a scalar fp32 load, coalesced along the pixels; rounding and the zeroed pad lanes are image_to_act_kernel's.
struct ChanSrcs {
  const float* ptr[GS_CAT_MAX_SRCS];
  long long stride[GS_CAT_MAX_SRCS];
  int ch[GS_CAT_MAX_SRCS];
  int n;
};

__global__ __launch_bounds__(256) void image_cat_to_act_kernel(const ChanSrcs s, unsigned short* act, long long hw, int Cp) {
  const int n = blockIdx.y;
  unsigned short* out = act + (size_t)n * hw * Cp;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x)
    store_bf_lanes(out + (size_t)p * Cp, Cp, [&](int b) {      // b: channel within source j once 0 <= b < ch[j]
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < GS_CAT_MAX_SRCS; ++j) {
        if (j < s.n) {
          if (b >= 0 && b < s.ch[j]) v = s.ptr[j][(size_t)n * s.stride[j] + (size_t)b * hw + p];
          b -= s.ch[j];
        }
      }
      return v;
    });
}

// its gradient: the channels of source j, as a dense [N, ch[j], S] fp32 tensor at grad[j]; a null grad[j] is left alone
struct ChanGrads {
  float* ptr[GS_CAT_MAX_SRCS];
  int ch[GS_CAT_MAX_SRCS];
  int n;
};

__global__ __launch_bounds__(256) void image_cat_to_act_bwd_kernel(const unsigned short* g, const ChanGrads s, long long hw,
                                                                   int Cp) {
  const int n = blockIdx.y;
  const unsigned short* gp = g + (size_t)n * hw * Cp;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x) {
    int off = 0;
#pragma unroll
    for (int j = 0; j < GS_CAT_MAX_SRCS; ++j) {
      if (j < s.n) {
        if (s.ptr[j])
          for (int c = 0; c < s.ch[j]; ++c) s.ptr[j][((size_t)n * s.ch[j] + c) * hw + p] = bf2f(gp[(size_t)p * Cp + off + c]);
        off += s.ch[j];
      }
    }
  }
}

extern "C" int gs_image_cat_to_act(const float* const* src, const int64_t* sample_stride, const int32_t* channels, int32_t K,
                                   void* act, int32_t N, int64_t S, int32_t Cp, void* stream) {
  GS_REQUIRE(src && sample_stride && channels && act && K >= 1 && K <= GS_CAT_MAX_SRCS && N > 0 && N <= 65535 && S > 0 &&
             Cp > 0 && (Cp & 7) == 0, "gs_image_cat_to_act: bad argument");
  ChanSrcs s{};
  long long total = 0;
  for (int j = 0; j < K; ++j) {
    GS_REQUIRE(src[j] && channels[j] > 0 && sample_stride[j] >= (int64_t)channels[j] * S,
               "gs_image_cat_to_act: a source needs a pointer, channels > 0 and a sample stride >= channels * S");
    s.ptr[j] = src[j]; s.stride[j] = sample_stride[j]; s.ch[j] = channels[j];
    total += channels[j];
  }
  GS_REQUIRE(total <= Cp, "gs_image_cat_to_act: the sources hold more channels than the activation");
  s.n = K;
  hipLaunchKernelGGL(image_cat_to_act_kernel, img_grid(S, N), dim3(256), 0, static_cast<hipStream_t>(stream), s,
                     static_cast<unsigned short*>(act), (long long)S, Cp);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_image_cat_to_act_backward(const void* g, float* const* grad, const int32_t* channels, int32_t K, int32_t N,
                                            int64_t S, int32_t Cp, void* stream) {
  GS_REQUIRE(g && grad && channels && K >= 1 && K <= GS_CAT_MAX_SRCS && N > 0 && N <= 65535 && S > 0 && Cp > 0,
             "gs_image_cat_to_act_backward: bad argument");
  ChanGrads s{};
  long long total = 0;
  bool any = false;
  for (int j = 0; j < K; ++j) {
    GS_REQUIRE(channels[j] > 0, "gs_image_cat_to_act_backward: a source needs channels > 0");
    s.ptr[j] = grad[j]; s.ch[j] = channels[j];
    total += channels[j];
    any = any || grad[j];
  }
  GS_REQUIRE(total <= Cp, "gs_image_cat_to_act_backward: the sources hold more channels than the activation gradient");
  GS_REQUIRE(any, "gs_image_cat_to_act_backward: no source asks for a gradient");
  s.n = K;
  hipLaunchKernelGGL(image_cat_to_act_bwd_kernel, img_grid(S, N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(g), s, (long long)S, Cp);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// dst[N, C, S] = zeros with src[N, t, S] at channels [c0, c0 + t): the generated channels next to zeroed guide channels
// (the visuals and infer() of the balanced CycleGAN). One workgroup row per (sample, channel); every element of dst is written
// exactly once, scalar stores (neither plane base need be 16-byte aligned).
__global__ __launch_bounds__(256) void channel_embed_kernel(const float* src, float* dst, int C, int c0, int t, long long hw) {
  const int n = blockIdx.y / C, c = blockIdx.y - n * C;
  float* out = dst + (size_t)blockIdx.y * hw;
  const bool live = c >= c0 && c < c0 + t;
  const float* in = live ? src + ((size_t)n * t + (c - c0)) * hw : nullptr;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long long)gridDim.x * blockDim.x)
    out[p] = live ? in[p] : 0.f;
}

extern "C" int gs_channel_embed(const float* src, float* dst, int32_t N, int32_t C, int32_t c0, int32_t t, int64_t S,
                                void* stream) {
  GS_REQUIRE(src && dst && N > 0 && C > 0 && t > 0 && c0 >= 0 && (int64_t)c0 + t <= C && S > 0 && (int64_t)N * C <= 65535,
             "gs_channel_embed: bad argument (the window [c0, c0 + t) must lie inside C, N * C <= 65535)");
  hipLaunchKernelGGL(channel_embed_kernel, img_grid(S, N * C), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst, C,
                     c0, t, (long long)S);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
