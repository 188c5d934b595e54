// MIND structure-consistency loss (Yang et al. 2018), fused from the images to the scalar and from the scalar back to the
// image gradient. Replaces the reference's StructureLoss / MINDDescriptor
// (projects/cleargrasp_depth_estimation/modules/old/cyclegan_losses_with_structure.py:41-92 and :95-182), which run an
// 81-channel depthwise 7x7 convolution over [N, 81, H, W] fp32 maps.
//
// Per plane I (the mean over the channels of an image, zero outside): for the 81 shifts a of the 9x9 non-local region
//   d_a(r) = I(r + a) - I(r)                         (r inside; I(r + a) = 0 outside)
//   D_a(p) = sum_{q in 7x7, p+q inside} g(q) d_a(p+q)^2,   g(q) = exp(-|q|_2 / sigma^2)   (distance, not its square)
//   B_b(p) = sum_{q in 7x7, p+q inside} I(p+q+b) for the 9 shifts b of the 3x3 neighbourhood, V = var_b(B_b) (divisor 8)
//   n_a = exp(-D_a / (V + 1e-8)),  f_a = n_a / sum_c n_c;   output channel i has row offset i % 9 - 4, column offset i / 9 - 4.
//
// One workgroup = one 16 x 16 tile of one plane, one pixel per thread. The plane tile with its halo of 7 (4 for the shift +
// 3 for the patch) sits in LDS (30 x 30 floats); per shift the 22 x 22 tile of masked d_a^2 is written to one of two LDS
// buffers (filled for shift a + 1 while shift a is summed: one barrier per shift) and every thread takes its 49 taps from
// it. The 81 numerators of a pixel stay in registers (the shift loop is unrolled, so every index is a constant) until their
// sum is known: no 81-channel map leaves the workgroup in the forward. No atomics anywhere: the loss is one partial per
// workgroup summed in index order by a second launch, the backward is a gather.
#include "mind_common.hpp"

#define MIND_T 16                    // tile edge
#define MIND_PW 30                   // plane tile: MIND_T + 2 * 7
#define MIND_DW 22                   // squared-difference tile: MIND_T + 2 * 3
#define MIND_DS 48                   // ... its row stride: the four rows of a wave read disjoint banks (0, 48, 32, 16 mod 64)
#define MIND_EW 24                   // backward: tile of E_a, MIND_T + 2 * 4
#define MIND_NS 81

struct MindW { float g[49]; };       // the patch weights, a kernel argument (scalar registers)

__device__ __forceinline__ bool mind_in(int y, int x, int H, int W) {
  return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}
__host__ __device__ constexpr int mind_ai(int a) { return a % 9 - 4; }      // row offset of shift a
__host__ __device__ constexpr int mind_aj(int a) { return a / 9 - 4; }      // column offset

// 30 x 30 tile of the channel mean of one sample with origin (h0 - 7, w0 - 7), zero outside the plane
__device__ __forceinline__ void mind_load_plane(const float* img, int C, int H, int W, int h0, int w0, float* sI) {
  for (int e = threadIdx.x; e < MIND_PW * MIND_PW; e += 256) {
    const int r = e / MIND_PW, c = e - r * MIND_PW;
    const int ih = h0 - 7 + r, iw = w0 - 7 + c;
    float v = 0.f;
    if (mind_in(ih, iw, H, W)) {
      const float* p = img + (size_t)ih * W + iw;
      float s = p[0];
      for (int ch = 1; ch < C; ++ch) s += p[(size_t)ch * H * W];
      v = C > 1 ? s / (float)C : s;
    }
    sI[e] = v;
  }
}

// the nine patch sums of the 3x3 neighbourhood and their unbiased variance at pixel (gy, gx) = tile (py, px)
struct MindV { float B[9]; float mean; float veps; };
__device__ __forceinline__ MindV mind_variance(const float* sI, int py, int px, int gy, int gx, int H, int W) {
  MindV v;
#pragma unroll
  for (int k = 0; k < 9; ++k) v.B[k] = 0.f;
#pragma unroll 1
  for (int qy = -3; qy <= 3; ++qy) {
#pragma unroll
    for (int qx = -3; qx <= 3; ++qx) {
      if (mind_in(gy + qy, gx + qx, H, W)) {
        const float* c = sI + (py + 7 + qy) * MIND_PW + px + 7 + qx;
#pragma unroll
        for (int k = 0; k < 9; ++k) v.B[k] += c[(k % 3 - 1) * MIND_PW + (k / 3 - 1)];
      }
    }
  }
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) m += v.B[k];
  m /= 9.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) { const float d = v.B[k] - m; s += d * d; }
  v.mean = m;
  v.veps = s / 8.f + MIND_EPS;
  return v;
}

// the (up to) two entries of the 22 x 22 tile of masked d_a^2 that a thread fills for every shift
struct MindFill {
  int ci[2], di[2];
  bool in[2];
  __device__ __forceinline__ MindFill(int h0, int w0, int H, int W) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = threadIdx.x + 256 * k;
      const bool ok = e < MIND_DW * MIND_DW;
      const int rr = ok ? e / MIND_DW : 0, rc = ok ? e - rr * MIND_DW : 0;
      in[k] = ok && mind_in(h0 - 3 + rr, w0 - 3 + rc, H, W);
      ci[k] = (rr + 4) * MIND_PW + rc + 4;
      di[k] = ok ? rr * MIND_DS + rc : -1;
    }
  }
  __device__ __forceinline__ void operator()(const float* sI, float* sD, int buf, int off) const {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (di[k] >= 0) {
        const float d = sI[ci[k] + off] - sI[ci[k]];
        sD[buf * (MIND_DW * MIND_DS) + di[k]] = in[k] ? d * d : 0.f;
      }
    }
  }
};
__device__ __forceinline__ float mind_patch_sum(const float* d, const MindW& w) {
  float D = 0.f;
#pragma unroll
  for (int ty = 0; ty < 7; ++ty) {
#pragma unroll
    for (int tx = 0; tx < 7; ++tx) D = fmaf(w.g[ty * 7 + tx], d[ty * MIND_DS + tx], D);
  }
  return D;
}

// f(a, D_a) for a = 0 .. 80 at this thread's pixel, a being a compile-time constant in each call (the forward keeps the 81
// numerators in registers). Every thread of the workgroup must call it (barriers inside); sI must be complete (a barrier
// after mind_load_plane) and is only read.
template <class F>
__device__ __forceinline__ void mind_shifts(const float* sI, float* sD, const MindW& w, int h0, int w0, int H, int W, F&& f) {
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const MindFill fill(h0, w0, H, W);
  fill(sI, sD, 0, mind_ai(0) * MIND_PW + mind_aj(0));
  __syncthreads();
  static_for<0, MIND_NS>([&](auto ic) {
    constexpr int a = decltype(ic)::value;
    if constexpr (a + 1 < MIND_NS) fill(sI, sD, (a + 1) & 1, mind_ai(a + 1) * MIND_PW + mind_aj(a + 1));
    f(ic, mind_patch_sum(sD + (a & 1) * (MIND_DW * MIND_DS) + py * MIND_DS + px, w));
    __syncthreads();
  });
}
// the same as a loop (the backward keeps its per-shift values in its scratch planes)
template <class F>
__device__ __forceinline__ void mind_shifts_loop(const float* sI, float* sD, const MindW& w, int h0, int w0, int H, int W,
                                                 F&& f) {
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const MindFill fill(h0, w0, H, W);
  fill(sI, sD, 0, mind_ai(0) * MIND_PW + mind_aj(0));
  __syncthreads();
#pragma unroll 1
  for (int a = 0; a < MIND_NS; ++a) {
    if (a + 1 < MIND_NS) fill(sI, sD, (a + 1) & 1, mind_ai(a + 1) * MIND_PW + mind_aj(a + 1));
    f(a, mind_patch_sum(sD + (a & 1) * (MIND_DW * MIND_DS) + py * MIND_DS + px, w));
    __syncthreads();
  }
}

// numerators n[81] and their sum Z of one plane at this thread's pixel; leaves the plane in sI
__device__ __forceinline__ MindV mind_numerators(const float* img, int C, int H, int W, int h0, int w0, const MindW& w,
                                                 float* sI, float* sD, float (&n)[MIND_NS], float& Z) {
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  mind_load_plane(img, C, H, W, h0, w0, sI);
  __syncthreads();
  const MindV v = mind_variance(sI, py, px, h0 + py, w0 + px, H, W);
  float z = 0.f;
  mind_shifts(sI, sD, w, h0, w0, H, W, [&](auto ic, float D) {
    constexpr int a = decltype(ic)::value;
    n[a] = expf(-D / v.veps);
    z += n[a];
  });
  Z = z;
  return v;
}

struct MindTile { int n, h0, w0; };
__device__ __forceinline__ MindTile mind_tile(int tiles_w, int tiles_h) {
  int b = blockIdx.x;
  MindTile t;
  t.w0 = (b % tiles_w) * MIND_T; b /= tiles_w;
  t.h0 = (b % tiles_h) * MIND_T;
  t.n = b / tiles_h;
  return t;
}

__global__ __launch_bounds__(256) void mind_descriptor_kernel(const float* x, int C, int H, int W, int tiles_w, int tiles_h,
                                                              const MindW w, float* out) {
  __shared__ float sI[MIND_PW * MIND_PW];
  __shared__ float sD[2 * MIND_DW * MIND_DS];
  const MindTile t = mind_tile(tiles_w, tiles_h);
  const int gy = t.h0 + (threadIdx.x >> 4), gx = t.w0 + (threadIdx.x & 15);
  float n[MIND_NS], Z;
  mind_numerators(x + (size_t)t.n * C * H * W, C, H, W, t.h0, t.w0, w, sI, sD, n, Z);
  if (gy < H && gx < W) {
    float* o = out + (size_t)t.n * MIND_NS * H * W + (size_t)gy * W + gx;
    static_for<0, MIND_NS>([&](auto ic) {
      constexpr int a = decltype(ic)::value;
      o[(size_t)a * H * W] = n[a] / Z;
    });
  }
}

__global__ __launch_bounds__(256) void mind_l1_kernel(const float* x, const float* y, int Cx, int Cy, int H, int W,
                                                      int tiles_w, int tiles_h, const MindW w, float* partial) {
  __shared__ float sI[MIND_PW * MIND_PW];
  __shared__ float sD[2 * MIND_DW * MIND_DS];
  __shared__ float sh[4];
  const MindTile t = mind_tile(tiles_w, tiles_h);
  const int gy = t.h0 + (threadIdx.x >> 4), gx = t.w0 + (threadIdx.x & 15);
  float nx[MIND_NS], ny[MIND_NS], Zx, Zy;
  mind_numerators(x + (size_t)t.n * Cx * H * W, Cx, H, W, t.h0, t.w0, w, sI, sD, nx, Zx);
  mind_numerators(y + (size_t)t.n * Cy * H * W, Cy, H, W, t.h0, t.w0, w, sI, sD, ny, Zy);
  float acc = 0.f;
  static_for<0, MIND_NS>([&](auto ic) {
    constexpr int a = decltype(ic)::value;
    acc += fabsf(nx[a] / Zx - ny[a] / Zy);
  });
  acc = mind_block_sum((gy < H && gx < W) ? acc : 0.f, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---- backward w.r.t. the second image ---------------------------------------------------------------------------------
// With s = grad_scale / (H W 81), sg_a = s sign(f_a^Y - f_a^X), Z = sum n:  dL/dn_a = (sg_a - sum_c sg_c f_c) / Z,
//   GD_a = -n_a / (V + eps) dL/dn_a,   GV = sum_a dL/dn_a n_a D_a / (V + eps)^2,   GB_b = GV 2 (B_b - mean B) / 8.
// First launch: the planes GD (81) and GB (9) per sample. A pixel's n_a^X and D_a^Y wait in scratch planes (each thread
// reads back only what it wrote itself) until Z^X, Z^Y and then sum_c sg_c f_c are known; n_a^X's plane then takes GD_a.
// Per sample: planes 0..80 GD, 81..89 GB, 90..170 D^Y. Second launch (a gather, one thread per pixel r):
//   dL/dI(r) = sum_a 2 [E_a(r - a) d_a(r - a) - E_a(r) d_a(r)] + sum_b F_b(r - b),
// E_a = g * GD_a and F_b = the 7x7 box sum of GB_b, both zero outside the plane; the result goes to every channel as 1/C.
#define MIND_BWD_PLANES 171
__global__ __launch_bounds__(256) void mind_grad_maps_kernel(const float* x, const float* y, int Cx, int Cy, int H, int W,
                                                             int tiles_w, int tiles_h, const MindW w, const float* grad_scale,
                                                             float inv_count, float* maps) {
  __shared__ float sI[MIND_PW * MIND_PW];
  __shared__ float sD[2 * MIND_DW * MIND_DS];
  const MindTile t = mind_tile(tiles_w, tiles_h);
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int gy = t.h0 + py, gx = t.w0 + px;
  const bool valid = gy < H && gx < W;
  const size_t HW = (size_t)H * W;
  float* m = maps + (size_t)t.n * MIND_BWD_PLANES * HW + (size_t)(valid ? gy : 0) * W + (valid ? gx : 0);
  float* mD = m + (size_t)90 * HW;

  mind_load_plane(x + (size_t)t.n * Cx * HW, Cx, H, W, t.h0, t.w0, sI);
  __syncthreads();
  const float vx = mind_variance(sI, py, px, gy, gx, H, W).veps;
  float Zx = 0.f;
  mind_shifts_loop(sI, sD, w, t.h0, t.w0, H, W, [&](int a, float D) {
    const float n = expf(-D / vx);
    Zx += n;
    if (valid) m[(size_t)a * HW] = n;
  });
  mind_load_plane(y + (size_t)t.n * Cy * HW, Cy, H, W, t.h0, t.w0, sI);
  __syncthreads();
  const MindV v = mind_variance(sI, py, px, gy, gx, H, W);
  float Zy = 0.f;
  mind_shifts_loop(sI, sD, w, t.h0, t.w0, H, W, [&](int a, float D) {
    Zy += expf(-D / v.veps);
    if (valid) mD[(size_t)a * HW] = D;
  });
  if (!valid) return;
  const float s = (grad_scale ? grad_scale[0] : 1.f) * inv_count;
  auto sigma_a = [&](float fy, float fx) { const float df = fy - fx; return df > 0.f ? s : (df < 0.f ? -s : 0.f); };
  float S = 0.f;
#pragma unroll 1
  for (int a = 0; a < MIND_NS; ++a) {
    const float fy = expf(-mD[(size_t)a * HW] / v.veps) / Zy;
    S = fmaf(sigma_a(fy, m[(size_t)a * HW] / Zx), fy, S);
  }
  float GV = 0.f;
#pragma unroll 1
  for (int a = 0; a < MIND_NS; ++a) {
    const float D = mD[(size_t)a * HW], ny = expf(-D / v.veps);
    const float dn = (sigma_a(ny / Zy, m[(size_t)a * HW] / Zx) - S) / Zy;
    GV = fmaf(dn * ny, D, GV);
    m[(size_t)a * HW] = -ny / v.veps * dn;
  }
  GV = GV / (v.veps * v.veps);
#pragma unroll
  for (int k = 0; k < 9; ++k) m[(size_t)(MIND_NS + k) * HW] = GV * (2.f * (v.B[k] - v.mean) / 8.f);
}

__global__ __launch_bounds__(256) void mind_gather_kernel(const float* y, int C, int H, int W, int tiles_w, int tiles_h,
                                                          const MindW w, const float* maps, float* grad) {
  __shared__ float sI[MIND_PW * MIND_PW];
  __shared__ float sG[MIND_PW * MIND_PW];
  __shared__ float sE[MIND_EW * MIND_EW];
  const MindTile t = mind_tile(tiles_w, tiles_h);
  const int py = threadIdx.x >> 4, px = threadIdx.x & 15;
  const int gy = t.h0 + py, gx = t.w0 + px;
  const size_t HW = (size_t)H * W;
  const float* mp = maps + (size_t)t.n * MIND_BWD_PLANES * HW;
  mind_load_plane(y + (size_t)t.n * C * HW, C, H, W, t.h0, t.w0, sI);
  float acc = 0.f;
#pragma unroll 1
  for (int a = 0; a < MIND_NS; ++a) {
    const int ai = a % 9 - 4, aj = a / 9 - 4;
    if (ai == 0 && aj == 0) continue;                   // d_a = 0: nothing flows through the zero shift
    mind_load_plane(mp + (size_t)a * HW, 1, H, W, t.h0, t.w0, sG);
    __syncthreads();
    // E_a on the tile and a ring of 4 around it (origin h0 - 4), zero outside the plane
    for (int e = threadIdx.x; e < MIND_EW * MIND_EW; e += 256) {
      const int er = e / MIND_EW, ec = e - er * MIND_EW;
      float E = 0.f;
      if (mind_in(t.h0 - 4 + er, t.w0 - 4 + ec, H, W)) {
        const float* gsrc = sG + er * MIND_PW + ec;
#pragma unroll
        for (int ty = 0; ty < 7; ++ty) {
#pragma unroll
          for (int tx = 0; tx < 7; ++tx) E = fmaf(w.g[ty * 7 + tx], gsrc[ty * MIND_PW + tx], E);
        }
      }
      sE[e] = E;
    }
    __syncthreads();
    const float Ir = sI[(py + 7) * MIND_PW + px + 7];
    const float Ipa = sI[(py + 7 + ai) * MIND_PW + px + 7 + aj];
    const float Ima = sI[(py + 7 - ai) * MIND_PW + px + 7 - aj];
    const float Er = sE[(py + 4) * MIND_EW + px + 4];
    const float Era = sE[(py + 4 - ai) * MIND_EW + px + 4 - aj];
    acc += 2.f * (Era * (Ir - Ima) - Er * (Ipa - Ir));
  }
#pragma unroll 1
  for (int k = 0; k < 9; ++k) {
    const int bi = k % 3 - 1, bj = k / 3 - 1;
    __syncthreads();
    mind_load_plane(mp + (size_t)(MIND_NS + k) * HW, 1, H, W, t.h0, t.w0, sG);
    __syncthreads();
    if (mind_in(gy - bi, gx - bj, H, W)) {
      const float* gsrc = sG + (py + 4 - bi) * MIND_PW + px + 4 - bj;
      float F = 0.f;
#pragma unroll
      for (int ty = 0; ty < 7; ++ty) {
#pragma unroll
        for (int tx = 0; tx < 7; ++tx) F += gsrc[ty * MIND_PW + tx];
      }
      acc += F;
    }
  }
  if (gy < H && gx < W) {
    const float gval = C > 1 ? acc / (float)C : acc;
    float* o = grad + (size_t)t.n * C * HW + (size_t)gy * W + gx;
    for (int ch = 0; ch < C; ++ch) o[(size_t)ch * HW] = gval;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// the reference's weights (mind_weight), by position in the patch
static MindW mind_weights(float sigma) {
  MindW w;
  for (int x = 0; x < 7; ++x)
    for (int y = 0; y < 7; ++y) w.g[x * 7 + y] = mind_weight((x - 3) * (x - 3) + (y - 3) * (y - 3), sigma);
  return w;
}

struct MindGrid { int th, tw; int64_t blocks; };
static MindGrid mind_grid(int N, int H, int W) {
  MindGrid g;
  g.th = mind_ceil_div(H, MIND_T);
  g.tw = mind_ceil_div(W, MIND_T);
  g.blocks = (int64_t)N * g.th * g.tw;
  return g;
}

#define MIND_REQUIRE_SIZES(name)                                                                                        \
  if (int rc = mind_check_sizes(name, 9, 7, nl_size, patch_size, neighbor_size, sigma, N > 0 && H > 0 && W > 0)) return rc; \
  GS_REQUIRE(mind_grid(N, H, W).blocks < (1ll << 31), name ": too many tiles")

extern "C" int64_t gs_mind_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t backward) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  if (backward) return (int64_t)N * MIND_BWD_PLANES * H * W * (int64_t)sizeof(float);
  return mind_grid(N, H, W).blocks * (int64_t)sizeof(float);
}

extern "C" int gs_mind_descriptor(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nl_size,
                                  int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* stream) {
  GS_REQUIRE(x && out && C > 0, "gs_mind_descriptor: bad argument");
  MIND_REQUIRE_SIZES("gs_mind_descriptor");
  const MindGrid g = mind_grid(N, H, W);
  hipLaunchKernelGGL(mind_descriptor_kernel, dim3((unsigned)g.blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, C, H,
                     W, g.tw, g.th, mind_weights(sigma), out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_mind_l1(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t H, int32_t W,
                          int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* scratch,
                          void* stream) {
  GS_REQUIRE(x && y && out && scratch && Cx > 0 && Cy > 0, "gs_mind_l1: bad argument");
  MIND_REQUIRE_SIZES("gs_mind_l1");
  const MindGrid g = mind_grid(N, H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(scratch);
  hipLaunchKernelGGL(mind_l1_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, x, y, Cx, Cy, H, W, g.tw, g.th,
                     mind_weights(sigma), partial);
  hipLaunchKernelGGL((final_sum_kernel<float, 256>), dim3(1), dim3(256), 0, st, (const float*)partial, (int)g.blocks,
                     1.0 / ((double)H * W * MIND_NS), out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_mind_l1_backward(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t H, int32_t W,
                                   int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma,
                                   const float* grad_scale, float* grad_y, void* scratch, void* stream) {
  GS_REQUIRE(x && y && grad_y && scratch && Cx > 0 && Cy > 0, "gs_mind_l1_backward: bad argument");
  MIND_REQUIRE_SIZES("gs_mind_l1_backward");
  const MindGrid g = mind_grid(N, H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* maps = static_cast<float*>(scratch);
  const MindW w = mind_weights(sigma);
  hipLaunchKernelGGL(mind_grad_maps_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, x, y, Cx, Cy, H, W, g.tw, g.th, w,
                     grad_scale, (float)(1.0 / ((double)H * W * MIND_NS)), maps);
  hipLaunchKernelGGL(mind_gather_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, y, Cy, H, W, g.tw, g.th, w,
                     (const float*)maps, grad_y);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
