// Loss / metric reductions on the boundary tensors (fp32): wavefront shuffle reduction -> workgroup -> a
// fixed-order final sum by the last-arriving workgroup (deterministic, single launch).
// Replaces nn.MSELoss vs an expanded constant target (ganslate/nn/losses/adversarial_loss.py:28-29,60-62),
// nn.L1Loss (cyclegan_losses.py:64,75,97-101; pix2pix_losses.py:15-19), tensor.mean() of
// utils/metrics/train_metrics.py:27-33 and SSIMLoss (nn/losses/utils/ssim.py:65-99).
#include "internal.hpp"

__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
  return t;
}

// publish this workgroup's partial; the last workgroup to arrive sums all partials in index order
__device__ __forceinline__ void finish_reduction(float partial, float* ws, float scale, float* out) {
  __shared__ int last;
  unsigned* counter = reinterpret_cast<unsigned*>(ws + 1024);
  if (threadIdx.x == 0) {
    __hip_atomic_store(ws + blockIdx.x, partial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == gridDim.x - 1);
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (last) {
    // all 256 threads of the last workgroup: thread t adds partials t, t+256, ... in index order, then a fixed-shape
    // tree over the threads — the same association every run (one thread walking up to 1024 partials cost 90 us)
    __shared__ double tree[256];
    double s = 0.0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256)
      s += (double)__hip_atomic_load(ws + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tree[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out[0] = (float)(tree[0] * (double)scale);
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- pointwise losses --------------------------------------------------------------------------------------------------------
// Every pointwise loss is one term functor: term(i) is element i's summand, grad(i, k) its derivative times k = upstream * gain / n.
// The two kernels below are the only grid-stride walks; a term is handed its indices in ascending order, seek(i, step) first.
struct DenseTerm { __device__ void seek(long long, long long) {} };      // (a term indexed by i alone keeps no cursor)

template <typename F>
__global__ __launch_bounds__(256) void reduce_kernel(F f, long long n, float* ws, float* out) {
  __shared__ float sh[4];
  float s = 0.f;
  const long long step = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  f.seek(i, step);
  for (; i < n; i += step) s += f.term(i);
  s = block_sum(s, sh);
  finish_reduction(s, ws, 1.0f / (float)n, out);
}
template <typename F>
__global__ __launch_bounds__(256) void map_kernel(F f, long long n, float* grad, const float* gscale) {
  const float k = (gscale ? gscale[0] : 1.f) * F::gain / (float)n;
  const long long step = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  f.seek(i, step);
  for (; i < n; i += step) grad[i] = f.grad(i, k);
}

struct MseConstTerm : DenseTerm {
  const float* x; float target;
  static constexpr float gain = 2.f;
  __device__ float term(long long i) const { const float d = x[i] - target; return d * d; }
  __device__ float grad(long long i, float k) const { return k * (x[i] - target); }
};

// The other GAN objectives of AdversarialLoss (adversarial_loss.py:26-34,60-73) as one pointwise function per mode:
//   vanilla       nn.BCEWithLogitsLoss vs the expanded label t: f = max(x,0) - x t + log1p(exp(-|x|)), f' = sigmoid(x) - t
//   wgangp        -mean(x) for real, +mean(x) for fake
//   nonsaturating softplus(-x) for real / softplus(x) for fake, averaged PER SAMPLE (a vector of `rows` losses); the
//                 reference's branch raises NameError (F is never imported, :68-73) — F.softplus' definition (threshold 20)
enum { ADV_LSGAN = 0, ADV_VANILLA = 1, ADV_WGANGP = 2, ADV_NONSAT = 3 };
template <int MODE>
__device__ __forceinline__ float adv_point(float x, float label, float sgn) {
  if constexpr (MODE == ADV_LSGAN) { const float d = x - label; return d * d; }
  if constexpr (MODE == ADV_VANILLA) return fmaxf(x, 0.f) - x * label + log1pf(expf(-fabsf(x)));
  if constexpr (MODE == ADV_WGANGP) return sgn * x;
  const float z = sgn * x;
  return z > 20.f ? z : log1pf(expf(z));
}
template <int MODE>
__device__ __forceinline__ float adv_point_grad(float x, float label, float sgn) {
  if constexpr (MODE == ADV_LSGAN) return 2.f * (x - label);
  if constexpr (MODE == ADV_VANILLA) return 1.f / (1.f + expf(-x)) - label;
  if constexpr (MODE == ADV_WGANGP) return sgn;
  const float z = sgn * x;
  return z > 20.f ? sgn : sgn / (1.f + expf(-z));
}
template <int MODE>
struct AdvTerm : DenseTerm {
  const float* x; float label, sgn;
  static constexpr float gain = 1.f;
  __device__ float term(long long i) const { return adv_point<MODE>(x[i], label, sgn); }
  __device__ float grad(long long i, float k) const { return k * adv_point_grad<MODE>(x[i], label, sgn); }
};
// nonsaturating: one workgroup per sample, fixed-shape sum
__global__ __launch_bounds__(256) void adv_rows_kernel(const float* x, long long per, float sgn, float* loss) {
  __shared__ float sh[4];
  const float* xr = x + (long long)blockIdx.x * per;
  float s = 0.f;
  for (long long i = threadIdx.x; i < per; i += blockDim.x) s += adv_point<ADV_NONSAT>(xr[i], 0.f, sgn);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[blockIdx.x] = s / (float)per;
}
__global__ __launch_bounds__(256) void adv_rows_grad_kernel(const float* x, long long per, float sgn, float* grad,
                                                            const float* gscale) {
  const long long base = (long long)blockIdx.x * per;
  const float k = (gscale ? gscale[blockIdx.x] : 1.f) / (float)per;
  for (long long i = threadIdx.x; i < per; i += blockDim.x)
    grad[base + i] = k * adv_point_grad<ADV_NONSAT>(x[base + i], 0.f, sgn);
}

struct L1Term : DenseTerm {
  const float* a; const float* b;
  static constexpr float gain = 1.f;
  __device__ float term(long long i) const { return fabsf(a[i] - b[i]); }
  __device__ float grad(long long i, float k) const { const float d = a[i] - b[i]; return d > 0.f ? k : (d < 0.f ? -k : 0.f); }
};
struct MeanTerm : DenseTerm {
  const float* x;
  __device__ float term(long long i) const { return x[i]; }
};
// L1 with a strided first operand (a channel window of a real image): sample n of `a` is `per` contiguous floats at
// a + n * stride, b is dense. The flat index i = n * per + r walks the same grid-stride loop as L1Term (same partial sums, same
// final order); the cursor (smp, r) follows it without a division per element. The gradient is the dense operand's: sign(b - a) * k.
struct L1WindowTerm {
  const float* a; long long stride; const float* b; long long per;
  long long smp, r, step;
  static constexpr float gain = 1.f;
  __device__ void seek(long long i, long long step_) { smp = i / per; r = i - smp * per; step = step_; }
  __device__ float diff(long long i) {
    const float d = a[smp * stride + r] - b[i];
    r += step;
    if (r >= per) { const long long q = r / per; smp += q; r -= q * per; }      // (a division only where a sample ends)
    return d;
  }
  __device__ float term(long long i) { return fabsf(diff(i)); }
  __device__ float grad(long long i, float k) { const float d = diff(i); return d > 0.f ? -k : (d < 0.f ? k : 0.f); }
};

static inline unsigned red_blocks(long long n) {
  long long b = (n + 256 * 8 - 1) / (256 * 8);
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (unsigned)b;
}
// this stream's partial-sum workspace, or null with the error set (gs_reduce_workspace's own "more than %d streams" stands)
static float* reduce_workspace(const char* entry, void* stream) {
  float* ws = gs_reduce_workspace(stream);
  if (!ws && !gs_zero_page()) gs_set_error("%s: library not initialised (call gs_init)", entry);
  return ws;
}
// loss = mean of f.term over n elements, then grad = its derivative (either may be null)
template <typename F>
static int pointwise_loss(const char* entry, F f, long long n, float* loss, float* grad, const float* gscale, void* stream) {
  float* ws = reduce_workspace(entry, stream);
  if (!ws) return 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (loss) hipLaunchKernelGGL(reduce_kernel<F>, dim3(red_blocks(n)), dim3(256), 0, st, f, n, ws, loss);
  if (grad) hipLaunchKernelGGL(map_kernel<F>, dim3(red_blocks(n)), dim3(256), 0, st, f, n, grad, gscale);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_mse_const(const float* x, int64_t n, float target, float* loss, float* grad,
                            const float* grad_scale, void* stream) {
  GS_REQUIRE(x && n > 0 && (loss || grad), "gs_mse_const: bad argument");
  return pointwise_loss("gs_mse_const", MseConstTerm{{}, x, target}, n, loss, grad, grad_scale, stream);
}
extern "C" int gs_adv_loss(const float* x, int64_t n, int32_t rows, int32_t mode, int32_t target_is_real, float label,
                           float* loss, float* grad, const float* grad_scale, void* stream) {
  GS_REQUIRE(x && n > 0 && (loss || grad) && mode >= ADV_LSGAN && mode <= ADV_NONSAT, "gs_adv_loss: bad argument");
  const float sgn = target_is_real ? -1.f : 1.f;
  if (mode == ADV_NONSAT) {
    GS_REQUIRE(rows > 0 && n % rows == 0, "gs_adv_loss: nonsaturating needs n divisible by rows (the batch)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (loss) hipLaunchKernelGGL(adv_rows_kernel, dim3(rows), dim3(256), 0, st, x, (long long)(n / rows), sgn, loss);
    if (grad) hipLaunchKernelGGL(adv_rows_grad_kernel, dim3(rows), dim3(256), 0, st, x, (long long)(n / rows), sgn, grad, grad_scale);
    GS_CHECK_HIP(hipGetLastError());
    return 0;
  }
  if (mode == ADV_LSGAN) return pointwise_loss("gs_adv_loss", AdvTerm<ADV_LSGAN>{{}, x, label, sgn}, n, loss, grad, grad_scale, stream);
  if (mode == ADV_VANILLA) return pointwise_loss("gs_adv_loss", AdvTerm<ADV_VANILLA>{{}, x, label, sgn}, n, loss, grad, grad_scale, stream);
  return pointwise_loss("gs_adv_loss", AdvTerm<ADV_WGANGP>{{}, x, label, sgn}, n, loss, grad, grad_scale, stream);
}
extern "C" int gs_l1(const float* a, const float* b, int64_t n, float* loss, float* grad_a, const float* grad_scale,
                     void* stream) {
  GS_REQUIRE(a && b && n > 0 && (loss || grad_a), "gs_l1: bad argument");
  return pointwise_loss("gs_l1", L1Term{{}, a, b}, n, loss, grad_a, grad_scale, stream);
}
extern "C" int gs_l1_window(const float* a, int64_t a_sample_stride, const float* b, int32_t N, int64_t per, float* loss,
                            float* grad_b, const float* grad_scale, void* stream) {
  GS_REQUIRE(a && b && N > 0 && per > 0 && a_sample_stride >= per && (loss || grad_b), "gs_l1_window: bad argument");
  return pointwise_loss("gs_l1_window", L1WindowTerm{a, (long long)a_sample_stride, b, (long long)per, 0, 0, 0},
                        (long long)N * per, loss, grad_b, grad_scale, stream);
}
extern "C" int gs_mean(const float* x, int64_t n, float* out, void* stream) {
  GS_REQUIRE(x && out && n > 0, "gs_mean: bad argument");
  float* ws = reduce_workspace("gs_mean", stream);
  if (!ws) return 2;
  hipLaunchKernelGGL(reduce_kernel<MeanTerm>, dim3(red_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), MeanTerm{{}, x},
                     (long long)n, ws, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- SSIM distance -----------------------------------------------------------------------------------------
// One workgroup = one 16x32 tile of the valid (H-10)x(W-10) output of one plane. Horizontal 11-tap Gaussian of
// the five maps X, Y, XX, YY, XY into LDS, then the vertical pass, S1/S2, sqrt(relu(2-S1-S2)).
#define SSIM_TH 16
#define SSIM_TW 32
__constant__ float c_gauss[11];

// A1 / B1 = S1 and A2 / B2 = S2 rounded as the reference's separate torch ops round them (ssim.py:85-98): every product
// first, then the sums. hipcc contracts a * b + c to an fma by default, which rounds 2 m1 m2 + C1 once but
// m1 m1 + m2 m2 + C1 twice: for identical images (m1 == m2) the two then differ by an ulp, S = 2 - S1 - S2 is +-1.2e-7
// instead of 0 and the backward multiplies by 1 / (2 sqrt(S)). Without contraction 2 m1 m2 and m1 m1 + m2 m2 are the same
// doubling of one rounded product, 2 s12 equals s1sq + s2sq bit for bit, S is exactly 0 and no gradient passes. The forward
// and the gradient maps share this body, so they agree on which pixels have S > 0.
struct SsimTerms { float A1, B1, A2, B2; };
__device__ __forceinline__ SsimTerms ssim_terms(float m1, float m2, float xx, float yy, float xy) {
#pragma clang fp contract(off)
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
  const float s1sq = xx - m11, s2sq = yy - m22, s12 = xy - m12;
  SsimTerms t;
  t.A1 = 2.f * m12 + C1;
  t.B1 = (m11 + m22) + C1;
  t.A2 = 2.f * s12 + C2;
  t.B2 = (s1sq + s2sq) + C2;
  return t;
}

// The window form's forward in double: the balanced recipe's translated channels are often one small plane per sample (a
// 3 x 12 x 11 volume has 6 valid pixels), where nothing averages the per-pixel fp32 error of the cancelling variance terms out
// (measured 6.8e-7 relative on such an input, fp32 in any operation order 5e-9 .. 1.1e-6). Same tiling, same fp32 Gaussian
// weights (the reference's, ssim.py:22-40) widened exactly; the (x + 1) / 2 mapping, the five blurred moments, S and the sums in
// double; one double partial per tile, summed in index order. What is left is the weights' rounding (~1.5e-7) and the final
// rounding of the mean to fp32. The gradient kernels are the dense ones.
// (no contraction, as in ssim_terms: identical images give S = 0 exactly)
__device__ __forceinline__ double ssim_s_double(double m1, double m2, double xx, double yy, double xy) {
#pragma clang fp contract(off)
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
  const double S1 = (2.0 * m12 + C1) / ((m11 + m22) + C1);
  const double S2 = (2.0 * (xy - m12) + C2) / (((xx - m11) + (yy - m22)) + C2);
  return 2.0 - (S1 + S2);
}

// The gradient w.r.t. the second image (the distance is symmetric, swap the arguments for the first):
// L = mean(D), D = sqrt(relu(2 - S1 - S2)) with mu1 = b(X), mu2 = b(Y), e11 = b(XX), e22 = b(YY), e12 = b(XY) (b = the
// separable 11-tap Gaussian, valid region). Per output pixel o, with gD = -dL/(2 D n):
//   G0 = gD * (dS1/dmu2 - mu1 * dS2/ds12 - 2 mu2 * dS2/ds2),  G1 = gD * dS2/ds12,  G2 = gD * dS2/ds2
//   dS1/dmu2 = (2 mu1 B1 - 2 mu2 A1) / B1^2,  dS2/ds12 = 2 / B2,  dS2/ds2 = -A2 / B2^2   (S1 = A1/B1, S2 = A2/B2)
// and dL/dY(p) = 1/2 * ( bT(G0)(p) + X(p) bT(G1)(p) + 2 Y(p) bT(G2)(p) ) with bT the transposed (full) Gaussian; the 1/2 is
// the (y + 1)/2 input mapping (nn/losses/utils/ssim.py:65-99 differentiated; cyclegan_losses.py:78-90 uses it as a loss).
//
// One 16x32 tile of one plane in the arithmetic type T (the fp32 Gaussian weights are widened per use), shared by the forward
// kernels and the gradient maps: which tile of which plane this workgroup is, the (16+10)x(32+10) patch of both images staged
// with the (v + 1) / 2 mapping (zero past the plane), the horizontal 11-tap pass of the five moments X, Y, XX, YY, XY, then per
// valid output pixel the vertical pass and either the distance, summed per thread and returned, or (MAPS) G0, G1, G2.
// x may be a channel window: plane p of sample n at x + n * xstride + p * H * W, xpl planes per sample (dense: xpl = all
// planes, one "sample"). The three tails stay inside this one body, after the vertical pass: with the pass behind a call of its
// own, hipcc pairs its taps differently and contracts other products to fmas, and the gradient maps change in the last bit.
template <typename T> __shared__ T ssim_sx[SSIM_TH + 10][SSIM_TW + 10];
template <typename T> __shared__ T ssim_sy[SSIM_TH + 10][SSIM_TW + 10];
template <typename T> __shared__ T ssim_hz[5][SSIM_TH + 10][SSIM_TW];
template <typename T, bool MAPS>
__device__ __forceinline__ T ssim_tile(const float* x, int xpl, long long xstride, const float* y, int H, int W, int tiles_w,
                                       int tiles_h, const float* grad_scale = nullptr, float inv_cnt = 0.f, float* maps = nullptr,
                                       size_t map_stride = 0) {
  int b = blockIdx.x;
  const int tw = b % tiles_w; b /= tiles_w;
  const int th = b % tiles_h; const int plane = b / tiles_h;
  const int Ho = H - 10, Wo = W - 10;
  const int oh0 = th * SSIM_TH, ow0 = tw * SSIM_TW;
  const float* xp = x + (size_t)(plane / xpl) * xstride + (size_t)(plane % xpl) * H * W;
  const float* yp = y + (size_t)plane * H * W;
  for (int e = threadIdx.x; e < (SSIM_TH + 10) * (SSIM_TW + 10); e += 256) {
    const int r = e / (SSIM_TW + 10), c = e % (SSIM_TW + 10);
    const int ih = oh0 + r, iw = ow0 + c;
    T a = 0, bb = 0;
    if (ih < H && iw < W) { a = ((T)xp[(size_t)ih * W + iw] + (T)1) * (T)0.5; bb = ((T)yp[(size_t)ih * W + iw] + (T)1) * (T)0.5; }
    ssim_sx<T>[r][c] = a; ssim_sy<T>[r][c] = bb;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (SSIM_TH + 10) * SSIM_TW; e += 256) {
    const int r = e / SSIM_TW, c = e % SSIM_TW;
    T m1 = 0, m2 = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const T g = (T)c_gauss[k], a = ssim_sx<T>[r][c + k], bb = ssim_sy<T>[r][c + k];
      m1 += g * a; m2 += g * bb; xx += g * a * a; yy += g * bb * bb; xy += g * a * bb;
    }
    ssim_hz<T>[0][r][c] = m1; ssim_hz<T>[1][r][c] = m2; ssim_hz<T>[2][r][c] = xx; ssim_hz<T>[3][r][c] = yy; ssim_hz<T>[4][r][c] = xy;
  }
  __syncthreads();
  const float up = MAPS ? (grad_scale ? grad_scale[0] : 1.f) * inv_cnt : 0.f;
  float* mp = MAPS ? maps + (size_t)plane * Ho * Wo : nullptr;
  T acc = 0;
  for (int e = threadIdx.x; e < SSIM_TH * SSIM_TW; e += 256) {
    const int r = e / SSIM_TW, c = e % SSIM_TW;
    if (oh0 + r < Ho && ow0 + c < Wo) {
      T m1 = 0, m2 = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const T g = (T)c_gauss[k];
        m1 += g * ssim_hz<T>[0][r + k][c]; m2 += g * ssim_hz<T>[1][r + k][c]; xx += g * ssim_hz<T>[2][r + k][c];
        yy += g * ssim_hz<T>[3][r + k][c]; xy += g * ssim_hz<T>[4][r + k][c];
      }
      if constexpr (std::is_same<T, double>::value) {
        acc += sqrt(fmax(ssim_s_double(m1, m2, xx, yy, xy), 0.0));
      } else {
        const SsimTerms t = ssim_terms(m1, m2, xx, yy, xy);
        const float A1 = t.A1, B1 = t.B1, A2 = t.A2, B2 = t.B2;
        if constexpr (!MAPS) {
          const float S = fmaxf(2.f - (A1 / B1 + A2 / B2), 0.f);
          acc += sqrtf(S);
        } else {
          const float S = 2.f - (A1 / B1 + A2 / B2);
          float g0 = 0.f, g1 = 0.f, g2 = 0.f;
          if (S > 0.f) {
            const float gD = -up / (2.f * sqrtf(S));
            const float dS1 = (2.f * m1 * B1 - 2.f * m2 * A1) / (B1 * B1);
            const float dS2_12 = 2.f / B2, dS2_2 = -A2 / (B2 * B2);
            g0 = gD * (dS1 - m1 * dS2_12 - 2.f * m2 * dS2_2);
            g1 = gD * dS2_12;
            g2 = gD * dS2_2;
          }
          const size_t o = (size_t)(oh0 + r) * Wo + (ow0 + c);
          mp[o] = g0; mp[map_stride + o] = g1; mp[2 * map_stride + o] = g2;
        }
      }
    }
  }
  return acc;
}

__global__ __launch_bounds__(256) void ssim_kernel(const float* x, int xpl, long long xstride, const float* y, int H, int W,
                                                   int tiles_w, int tiles_h, float* partial) {
  __shared__ float sh[4];
  float acc = ssim_tile<float, false>(x, xpl, xstride, y, H, W, tiles_w, tiles_h);
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void ssim_window_kernel(const float* x, int xpl, long long xstride, const float* y, int H,
                                                          int W, int tiles_w, int tiles_h, double* partial) {
  const double acc = ssim_tile<double, false>(x, xpl, xstride, y, H, W, tiles_w, tiles_h);
  // fixed-shape tree over the 256 threads (ssim_sx is free again: every thread is past its last read of it)
  __syncthreads();
  double* tree = &ssim_sx<double>[0][0];
  tree[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) tree[threadIdx.x] += tree[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) partial[blockIdx.x] = tree[0];
}
__global__ __launch_bounds__(256) void ssim_grad_maps_kernel(const float* x, int xpl, long long xstride, const float* y, int H,
                                                             int W, int tiles_w, int tiles_h, const float* grad_scale, float inv_cnt,
                                                             float* maps, size_t map_stride) {
  ssim_tile<float, true>(x, xpl, xstride, y, H, W, tiles_w, tiles_h, grad_scale, inv_cnt, maps, map_stride);
}
static int ssim_init_gauss() {
  static bool init = false;
  if (!init) {
    // fp32 restatement of _fspecial_gauss_1d(11, 1.5) (ssim.py:22-40)
    float g[11], s = 0.f;
    for (int i = 0; i < 11; ++i) { const float c = (float)(i - 5); g[i] = expf(-(c * c) / (2.f * 1.5f * 1.5f)); s += g[i]; }
    for (int i = 0; i < 11; ++i) g[i] /= s;
    GS_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), g, sizeof(g)));
    init = true;
  }
  return 0;
}

// tiles of 16 x 32 covering rows x cols pixels
static inline void ssim_tiles(int rows, int cols, int* th, int* tw) {
  *th = (rows + SSIM_TH - 1) / SSIM_TH;
  *tw = (cols + SSIM_TW - 1) / SSIM_TW;
}
// the arguments of a window entry point: as the dense ones, plus the window's layout
static int ssim_window_check(const char* entry, const float* x, const float* y, const float* out, const float* scratch, int32_t NC,
                             int32_t H, int32_t W, int32_t x_planes, int64_t x_sample_stride) {
  GS_REQUIRE(x && y && out && scratch && NC > 0 && H > 10 && W > 10, "%s: bad argument", entry);
  GS_REQUIRE(x_planes > 0 && NC % x_planes == 0 && x_sample_stride >= (int64_t)x_planes * H * W,
             "%s: NC must be samples * x_planes and the sample stride >= x_planes * H * W", entry);
  return 0;
}

extern "C" int64_t gs_ssim_scratch_floats(int32_t NC, int32_t H, int32_t W) {
  int th, tw;
  ssim_tiles(H - 10, W - 10, &th, &tw);
  return (int64_t)NC * th * tw;
}
// one partial of type P per tile by `kernel`, then their mean over the valid pixels
template <typename P>
static int ssim_forward(void (*kernel)(const float*, int, long long, const float*, int, int, int, int, P*), const float* x, int xpl,
                        long long xstride, const float* y, int32_t NC, int32_t H, int32_t W, float* out, P* partial, void* stream) {
  if (int rc = ssim_init_gauss()) return rc;
  int th, tw;
  ssim_tiles(H - 10, W - 10, &th, &tw);
  const int blocks = NC * th * tw;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, x, xpl, xstride, y, H, W, tw, th, partial);
  double scale = 1.0 / ((double)NC * (H - 10) * (W - 10));
  if (std::is_same<P, float>::value) scale = (double)(float)scale;      // the fp32 path has always rounded its scale to fp32
  hipLaunchKernelGGL((final_sum_kernel<P, 1024>), dim3(1), dim3(256), 0, st, partial, blocks, scale, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int gs_ssim_distance(const float* x, const float* y, int32_t NC, int32_t H, int32_t W, float* out,
                                float* scratch, void* stream) {
  GS_REQUIRE(x && y && out && scratch && NC > 0 && H > 10 && W > 10, "gs_ssim_distance: bad argument");
  return ssim_forward(ssim_kernel, x, NC, 0, y, NC, H, W, out, scratch, stream);
}
extern "C" int gs_ssim_distance_window(const float* x, int64_t x_sample_stride, int32_t x_planes, const float* y, int32_t NC,
                                       int32_t H, int32_t W, float* out, float* scratch, void* stream) {
  if (int rc = ssim_window_check("gs_ssim_distance_window", x, y, out, scratch, NC, H, W, x_planes, x_sample_stride)) return rc;
  GS_REQUIRE(((uintptr_t)scratch & 7) == 0, "gs_ssim_distance_window: scratch must be 8-byte aligned (one double per tile)");
  return ssim_forward(ssim_window_kernel, x, x_planes, (long long)x_sample_stride, y, NC, H, W, out,
                      reinterpret_cast<double*>(scratch), stream);
}

// transposed separable Gaussian of the three maps + combination with X, Y: one workgroup = 16x32 input pixels
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* x, int xpl, long long xstride, const float* y,
                                                       const float* maps, size_t map_stride, int H, int W, int tiles_w,
                                                       int tiles_h, float* grad_y) {
  __shared__ float sm[3][SSIM_TH + 10][SSIM_TW + 10];
  __shared__ float hz[3][SSIM_TH + 10][SSIM_TW];
  int b = blockIdx.x;
  const int tw = b % tiles_w; b /= tiles_w;
  const int th = b % tiles_h; const int plane = b / tiles_h;
  const int Ho = H - 10, Wo = W - 10;
  const int ph0 = th * SSIM_TH, pw0 = tw * SSIM_TW;
  const float* mp = maps + (size_t)plane * Ho * Wo;
  // output-pixel window [ph0 - 10, ph0 + TH) x [pw0 - 10, pw0 + TW), zero outside the valid map
  for (int e = threadIdx.x; e < (SSIM_TH + 10) * (SSIM_TW + 10); e += 256) {
    const int r = e / (SSIM_TW + 10), c = e % (SSIM_TW + 10);
    const int oh = ph0 - 10 + r, ow = pw0 - 10 + c;
    const bool ok = oh >= 0 && oh < Ho && ow >= 0 && ow < Wo;
    const size_t o = ok ? (size_t)oh * Wo + ow : 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) sm[m][r][c] = ok ? mp[m * map_stride + o] : 0.f;
  }
  __syncthreads();
  // horizontal: t[r][c] = sum_k w[k] * G[.., pw - k]  ->  window column (c + 10 - k)
  for (int e = threadIdx.x; e < (SSIM_TH + 10) * SSIM_TW; e += 256) {
    const int r = e / SSIM_TW, c = e % SSIM_TW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float g = c_gauss[k];
      a0 += g * sm[0][r][c + 10 - k]; a1 += g * sm[1][r][c + 10 - k]; a2 += g * sm[2][r][c + 10 - k];
    }
    hz[0][r][c] = a0; hz[1][r][c] = a1; hz[2][r][c] = a2;
  }
  __syncthreads();
  const float* xp = x + (size_t)(plane / xpl) * xstride + (size_t)(plane % xpl) * H * W;
  const float* yp = y + (size_t)plane * H * W;
  float* gp = grad_y + (size_t)plane * H * W;
  for (int e = threadIdx.x; e < SSIM_TH * SSIM_TW; e += 256) {
    const int r = e / SSIM_TW, c = e % SSIM_TW;
    const int ph = ph0 + r, pw = pw0 + c;
    if (ph < H && pw < W) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const float g = c_gauss[k];
        a0 += g * hz[0][r + 10 - k][c]; a1 += g * hz[1][r + 10 - k][c]; a2 += g * hz[2][r + 10 - k][c];
      }
      const size_t i = (size_t)ph * W + pw;
      const float X = (xp[i] + 1.f) * 0.5f, Y = (yp[i] + 1.f) * 0.5f;
      gp[i] = 0.5f * (a0 + X * a1 + 2.f * Y * a2);
    }
  }
}

extern "C" int64_t gs_ssim_backward_scratch_floats(int32_t NC, int32_t H, int32_t W) {
  return 3 * (int64_t)NC * (H - 10) * (W - 10);
}

static int ssim_backward(const float* x, int xpl, long long xstride, const float* y, int32_t NC, int32_t H, int32_t W,
                         const float* grad_scale, float* grad_y, float* scratch, void* stream) {
  if (int rc = ssim_init_gauss()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Ho = H - 10, Wo = W - 10;
  const size_t map_stride = (size_t)NC * Ho * Wo;
  int th, tw, th2, tw2;
  ssim_tiles(Ho, Wo, &th, &tw);
  hipLaunchKernelGGL(ssim_grad_maps_kernel, dim3(NC * th * tw), dim3(256), 0, st, x, xpl, xstride, y, H, W, tw, th, grad_scale,
                     (float)(1.0 / ((double)NC * Ho * Wo)), scratch, map_stride);
  ssim_tiles(H, W, &th2, &tw2);
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3(NC * th2 * tw2), dim3(256), 0, st, x, xpl, xstride, y, scratch, map_stride, H, W, tw2,
                     th2, grad_y);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int gs_ssim_distance_backward(const float* x, const float* y, int32_t NC, int32_t H, int32_t W,
                                         const float* grad_scale, float* grad_y, float* scratch, void* stream) {
  GS_REQUIRE(x && y && grad_y && scratch && NC > 0 && H > 10 && W > 10, "gs_ssim_distance_backward: bad argument");
  return ssim_backward(x, NC, 0, y, NC, H, W, grad_scale, grad_y, scratch, stream);
}
extern "C" int gs_ssim_distance_window_backward(const float* x, int64_t x_sample_stride, int32_t x_planes, const float* y,
                                                int32_t NC, int32_t H, int32_t W, const float* grad_scale, float* grad_y,
                                                float* scratch, void* stream) {
  if (int rc = ssim_window_check("gs_ssim_distance_window_backward", x, y, grad_y, scratch, NC, H, W, x_planes, x_sample_stride))
    return rc;
  return ssim_backward(x, x_planes, x_sample_stride, y, NC, H, W, grad_scale, grad_y, scratch, stream);
}

// ---- scalar algebra of a recipe's loss assembly ----------------------------------------------------------------------------------
// out[r] = c[r] + sum_k m[r][k] * x_k[0] for R <= 8 rows over K <= 16 device scalars (a null x_k counts as 0): the
// "lambda_AB * (alpha * ssim + beta * l1)", "loss_real + loss_fake", "sum of the G losses" lines of the recipes
// (cyclegan_losses.py:21-32,70-90, cyclegan.py:150,182) as ONE launch instead of one torch elementwise kernel per operator;
// the backward of such a combination is the same launch with the transposed matrix over the rows' upstream gradients.
struct ScalarAffineK {
  const float* x[16];
  float m[8][16];
  float c[8];
  float* out;
  int K, R;
};
__global__ __launch_bounds__(64) void scalar_affine_kernel(const ScalarAffineK p) {
  const int r = threadIdx.x;
  if (r >= p.R) return;
  float acc = p.c[r];
  for (int k = 0; k < p.K; ++k)
    if (p.x[k]) acc += p.m[r][k] * p.x[k][0];
  p.out[r] = acc;
}
extern "C" int gs_scalar_affine(const float* const* x, int32_t K, const float* m, const float* c, int32_t R, float* out,
                                void* stream) {
  GS_REQUIRE(x && m && out && K > 0 && K <= 16 && R > 0 && R <= 8, "gs_scalar_affine: bad argument (K <= 16, R <= 8)");
  ScalarAffineK p;
  for (int k = 0; k < 16; ++k) p.x[k] = k < K ? x[k] : nullptr;
  for (int r = 0; r < 8; ++r) {
    p.c[r] = (c && r < R) ? c[r] : 0.f;
    for (int k = 0; k < 16; ++k) p.m[r][k] = (r < R && k < K) ? m[r * K + k] : 0.f;
  }
  p.out = out; p.K = K; p.R = R;
  hipLaunchKernelGGL(scalar_affine_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), p);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// out = a + b over n floats: the join of two gradients of one image (a generated image feeds a discriminator AND the
// other generator, cyclegan.py:131-141 — autograd's own accumulation would be a torch kernel)
__global__ __launch_bounds__(256) void sum2_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                   float4* __restrict__ out, long long n4, const float* as, const float* bs,
                                                   float* os, int tail) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 u = a[i], v = b[i];
    out[i] = float4{u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w};
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) os[threadIdx.x] = as[threadIdx.x] + bs[threadIdx.x];
}
extern "C" int gs_sum2_f32(const float* a, const float* b, float* out, int64_t n, void* stream) {
  GS_REQUIRE(a && b && out && n > 0, "gs_sum2_f32: bad argument");
  GS_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
             "gs_sum2_f32: buffers must be 16-byte aligned");
  const long long n4 = n / 4;
  long long blocks = (n4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(sum2_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(b), reinterpret_cast<float4*>(out), n4,
                     a + n4 * 4, b + n4 * 4, out + n4 * 4, (int)(n - n4 * 4));
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

