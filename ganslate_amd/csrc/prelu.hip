// V-Net elementwise family (ganslate/nn/generators/vnet/vnet3d.py:155-267, ganslate/nn/invertible.py:8-48):
// InstanceNorm3d(affine=False) -> [+ residual] -> nn.PReLU(C) (learnable per-channel slope) -> [+ residual] on channel
// slices of NDHWC bf16 tensors, and the autograd backward of that chain including the slope gradient.
//   forward : u = norm(y) (or y);  mode 1: u += res;  v = u > 0 ? u : slope[c]*u;  mode 2: v += res;  out = v
//   backward: gt = g (+ g2);  gu = gt * (u > 0 ? 1 : slope[c]);  dslope[c] += sum gt*min(u,0);
//             dy = rstd*(gu - mean gu - yhat*mean(gu*yhat))  (or gu without norm);  gres = gu (mode 1, optional)
// The residual of mode 1 may be a channel-repeated tensor (InputBlock's x.repeat, vnet3d.py:162-167): channel c reads
// res channel c % res_mod. Uses: InputBlock (norm, mode 1, repeat), down/up convs (norm, no residual), additive
// coupling y1 = x1 + PReLU(IN(conv(x2))) (norm, mode 2), block tails PReLU(core(x) + x) (no norm, mode 1).
// HBM-bound streaming kernels: 16 B per lane, fp32 math, deterministic two-level reductions (atomics only for the
// final per-image accumulation into the parameter-gradient buffer, as in wgrad).
#include "norm_common.hpp"

struct PNormK {
  gs_pnorm_desc d;
  int C8;
  unsigned HW;
  int c8_shift;               // log2(C8) when C8 is a power of two (the element loops' grid strides are multiples of 256), else -1
};

// residual of 8 consecutive channels starting at c8*8 of pixel `pix`
__device__ __forceinline__ void pn_res8(float* f, const gs_pnorm_desc& d, const unsigned short* res, size_t pix,
                                        int c8) {
  if (d.res_mod > 0) {
    const unsigned short* r = res + pix * d.res_cs + d.res_co;
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = bf2f(r[(c8 * 8 + k) % d.res_mod]);
  } else {
    view8(f, res, pix, d.res_cs, d.res_co, c8);
  }
}

// The per-channel numbers of one 8-channel group. A thread whose channel group does not change over its loop (every power-of-two
// channel count: the grid stride is a multiple of C8) loads them ONCE: per 16-byte element the kernels fetched three to six
// 32-byte vectors of statistics / slopes / sums and ran an integer division for the pixel index.
struct PnCh {
  float mu[8], rs[8], sl[8];
};
__device__ __forceinline__ void pn_ch_load(PnCh& c, const gs_pnorm_desc& d, const float* mr, const float* slope, int c8) {
  if (mr) { load8(c.mu, mr + c8 * 8); load8(c.rs, mr + d.C + c8 * 8); }
  if (slope) load8(c.sl, slope + c8 * 8);
}

// pre-activation u of one 8-channel group
__device__ __forceinline__ void pn_preact_c(float* u, float* yh, const PNormK& p, const unsigned short* y, bool has_mr,
                                            const PnCh& c, const unsigned short* res, size_t pix, int c8) {
  const gs_pnorm_desc& d = p.d;
  view8(yh, y, pix, d.y_cs, d.y_co, c8);
  if (has_mr) {
#pragma unroll
    for (int k = 0; k < 8; ++k) yh[k] = (yh[k] - c.mu[k]) * c.rs[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) u[k] = yh[k];
  if (d.res_mode == 1) {
    float r[8];
    pn_res8(r, d, res, pix, c8);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] += r[k];
  }
}

__global__ __launch_bounds__(256) void pnorm_fwd_kernel(const PNormK p, const unsigned short* y, const float* mean_rstd,
                                                        const unsigned short* res, const float* slope,
                                                        unsigned short* out) {
  const gs_pnorm_desc& d = p.d;
  const int n = blockIdx.y;
  const unsigned per_img = p.HW * (unsigned)p.C8;
  const float* mr = mean_rstd ? mean_rstd + (size_t)n * 2 * d.C : nullptr;
  const bool fixed = p.c8_shift >= 0;                  // (uniform) power-of-two channel groups: this thread keeps its group
  PnCh ch;
  if (fixed) pn_ch_load(ch, d, mr, slope, (int)((blockIdx.x * 256u + threadIdx.x) & (unsigned)(p.C8 - 1)));
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < per_img; e += gridDim.x * 256u) {
    const unsigned px = fixed ? e >> p.c8_shift : e / (unsigned)p.C8;
    const int c8 = (int)(e - px * (unsigned)p.C8);
    const size_t pix = (size_t)n * p.HW + px;
    float u[8], yh[8];
    if (!fixed) pn_ch_load(ch, d, mr, slope, c8);
    pn_preact_c(u, yh, p, y, mr != nullptr, ch, res, pix, c8);
    if (slope) {
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = u[k] > 0.f ? u[k] : ch.sl[k] * u[k];
    }
    if (d.res_mode == 2) {
      float r[8];
      pn_res8(r, d, res, pix, c8);
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] += r[k];
    } else if (d.res_mode == 3) {        // inverse of an additive coupling: x = y - F(.)  (memcnn AdditiveCoupling.inverse)
      float r[8];
      pn_res8(r, d, res, pix, c8);
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = r[k] - u[k];
    }
    *reinterpret_cast<uint4*>(out + pix * d.out_cs + d.out_co + c8 * 8) = pack_bf8(u);
  }
}

// gu and the slope-gradient integrand of one 8-channel group
__device__ __forceinline__ void pn_gu_c(float* gu, float* gs, const PNormK& p, const unsigned short* g,
                                        const unsigned short* g2, const float* u, bool has_slope, const PnCh& c, size_t pix,
                                        int c8) {
  const gs_pnorm_desc& d = p.d;
  float a[8], b[8];
  view8(a, g, pix, d.g_cs, d.g_co, c8);
  if (g2) {
    view8(b, g2, pix, d.g2_cs, d.g2_co, c8);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += b[k];
  }
  if (d.res_mode == 3) {                 // out = res - v: the branch sees the negated gradient
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = -a[k];
  }
  if (has_slope) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      gu[k] = u[k] > 0.f ? a[k] : a[k] * c.sl[k];
      gs[k] = u[k] > 0.f ? 0.f : a[k] * u[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) { gu[k] = a[k]; gs[k] = 0.f; }
  }
}

// pass 1: per (n, pixel chunk) partial sums of (gu, gu*yhat, yhat, g*min(u,0)) -> partial [N][chunks][4][C]
template <int COLS>
__global__ __launch_bounds__(256) void pnorm_bwd_reduce_kernel(const PNormK p, const unsigned short* g,
                                                               const unsigned short* g2, const unsigned short* y,
                                                               const float* mean_rstd, const unsigned short* res,
                                                               const float* slope, float* partial, int pix_per_block,
                                                               int chunks) {
  constexpr int ROWS = 256 / COLS;
  __shared__ float red[ROWS][COLS][33];
  const gs_pnorm_desc& d = p.d;
  const int n = blockIdx.y, tid = threadIdx.x;
  const int col = tid % COLS, row = tid / COLS;
  const int c8 = blockIdx.z * COLS + col;
  const unsigned p0 = blockIdx.x * pix_per_block;
  const unsigned p1 = min(p.HW, p0 + pix_per_block);
  const float* mr = mean_rstd ? mean_rstd + (size_t)n * 2 * d.C : nullptr;
  float acc[4][8];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[r][k] = 0.f;
  if (c8 < p.C8) {
    PnCh ch;                                         // (the thread's channel group is fixed: its numbers once)
    pn_ch_load(ch, d, mr, slope, c8);
    for (unsigned px = p0 + row; px < p1; px += ROWS) {
      const size_t pix = (size_t)n * p.HW + px;
      float u[8], yh[8], gu[8], gs[8];
      pn_preact_c(u, yh, p, y, mr != nullptr, ch, res, pix, c8);
      pn_gu_c(gu, gs, p, g, g2, u, slope != nullptr, ch, pix, c8);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        acc[0][k] += gu[k]; acc[1][k] += gu[k] * yh[k]; acc[2][k] += yh[k]; acc[3][k] += gs[k];
      }
    }
  }
  row_fold(red, partial, n, chunks, p.C8, acc[0], acc[1], acc[2], acc[3]);
}

// (pass 2, per (n, c) totals over the chunks -> sums [N][4][C] and the parameter gradients dslope[c] += S4, bias_grad[c] +=
// -rstd*S2*S3/hw, is slot_sum_kernel<4> of norm.hip)

// pass 3: dy (and optionally gres = gu)
__global__ __launch_bounds__(256) void pnorm_bwd_apply_kernel(const PNormK p, const unsigned short* g,
                                                              const unsigned short* g2, const unsigned short* y,
                                                              const float* mean_rstd, const unsigned short* res,
                                                              const float* slope, const float* sums,
                                                              unsigned short* dy, unsigned short* gres) {
  const gs_pnorm_desc& d = p.d;
  const int n = blockIdx.y;
  const unsigned per_img = p.HW * (unsigned)p.C8;
  const float inv_hw = 1.0f / (float)p.HW;
  const float* mr = mean_rstd ? mean_rstd + (size_t)n * 2 * d.C : nullptr;
  const float* sm = sums ? sums + (size_t)n * 4 * d.C : nullptr;
  const bool fixed = p.c8_shift >= 0;                  // (uniform) see pnorm_fwd_kernel
  PnCh ch;
  float s1[8], s2[8];
  auto load_ch = [&](int c8) {
    pn_ch_load(ch, d, mr, slope, c8);
    if (mr) { load8(s1, sm + c8 * 8); load8(s2, sm + d.C + c8 * 8); }
  };
  if (fixed) load_ch((int)((blockIdx.x * 256u + threadIdx.x) & (unsigned)(p.C8 - 1)));
  for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < per_img; e += gridDim.x * 256u) {
    const unsigned px = fixed ? e >> p.c8_shift : e / (unsigned)p.C8;
    const int c8 = (int)(e - px * (unsigned)p.C8);
    const size_t pix = (size_t)n * p.HW + px;
    float u[8], yh[8], gu[8], gs[8], o[8];
    if (!fixed) load_ch(c8);
    pn_preact_c(u, yh, p, y, mr != nullptr, ch, res, pix, c8);
    pn_gu_c(gu, gs, p, g, g2, u, slope != nullptr, ch, pix, c8);
    if (gres) *reinterpret_cast<uint4*>(gres + pix * d.gres_cs + d.gres_co + c8 * 8) = pack_bf8(gu);
    if (mr) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = ch.rs[k] * (gu[k] - s1[k] * inv_hw - yh[k] * s2[k] * inv_hw);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = gu[k];
    }
    *reinterpret_cast<uint4*>(dy + pix * d.dy_cs + d.dy_co + c8 * 8) = pack_bf8(o);
  }
}

static int pn_pix_per_block(long long pixels) {
  // (1024 chunks per image: 2048 made the second pass walk twice the rows for nothing — brats 54.48 -> 54.15 ms, 512: 55.08)
  long long ppb = (pixels + 1023) / 1024;
  return ppb < 64 ? 64 : (int)((ppb + 63) / 64 * 64);
}

static int pn_check(const gs_pnorm_desc* d, const char* who) {
  GS_REQUIRE(d && d->N > 0 && d->pixels > 0 && d->C > 0 && (d->C & 7) == 0, "%s: bad shape", who);
  GS_REQUIRE(d->pixels * (d->C / 8) < (1LL << 31), "%s: image too large", who);
  GS_REQUIRE(d->res_mode >= 0 && d->res_mode <= 3, "%s: res_mode must be 0 .. 3", who);
  GS_REQUIRE((d->y_cs & 7) == 0 && (d->y_co & 7) == 0, "%s: y view must be 8-channel aligned", who);
  GS_REQUIRE(d->res_mode == 0 || d->res_mod > 0 || ((d->res_cs & 7) == 0 && (d->res_co & 7) == 0),
             "%s: residual view must be 8-channel aligned", who);
  return 0;
}

extern "C" int gs_pnorm_forward(const gs_pnorm_desc* d, const void* y, const float* mean_rstd, const void* res,
                                const float* slope, void* out, void* stream) {
  if (int rc = pn_check(d, "gs_pnorm_forward")) return rc;
  GS_REQUIRE(y && out && (d->res_mode == 0 || res), "gs_pnorm_forward: null tensor");
  GS_REQUIRE((d->out_cs & 7) == 0 && (d->out_co & 7) == 0, "gs_pnorm_forward: output view must be 8-channel aligned");
  PNormK k;
  k.d = *d; k.C8 = d->C / 8; k.HW = (unsigned)d->pixels;
  k.c8_shift = norm_c8_shift(k.C8);
  hipLaunchKernelGGL(pnorm_fwd_kernel, dim3(norm_grid((long long)k.HW * k.C8, 2048), d->N), dim3(256), 0,
                     static_cast<hipStream_t>(stream), k, static_cast<const unsigned short*>(y), mean_rstd,
                     static_cast<const unsigned short*>(res), slope, static_cast<unsigned short*>(out));
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t gs_pnorm_backward_scratch_floats(const gs_pnorm_desc* d) {
  const int64_t ppb = pn_pix_per_block(d->pixels);
  const int64_t chunks = (d->pixels + ppb - 1) / ppb;
  return (int64_t)d->N * (chunks + 1) * 4 * d->C;
}

extern "C" int gs_pnorm_backward(const gs_pnorm_desc* d, const void* g, const void* g2, const void* y,
                                 const float* mean_rstd, const void* res, const float* slope, void* dy, void* gres,
                                 float* dslope, float* bias_grad, float* scratch, void* stream) {
  if (int rc = pn_check(d, "gs_pnorm_backward")) return rc;
  GS_REQUIRE(g && y && dy && (d->res_mode != 1 || res), "gs_pnorm_backward: null tensor");
  GS_REQUIRE((d->g_cs & 7) == 0 && (d->g_co & 7) == 0 && (!g2 || ((d->g2_cs & 7) == 0 && (d->g2_co & 7) == 0)) &&
                 (d->dy_cs & 7) == 0 && (d->dy_co & 7) == 0 && (!gres || ((d->gres_cs & 7) == 0 && (d->gres_co & 7) == 0)),
             "gs_pnorm_backward: views must be 8-channel aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  PNormK k;
  k.d = *d; k.C8 = d->C / 8; k.HW = (unsigned)d->pixels;
  k.c8_shift = norm_c8_shift(k.C8);
  const unsigned short* gp = static_cast<const unsigned short*>(g);
  const unsigned short* g2p = static_cast<const unsigned short*>(g2);
  const unsigned short* yp = static_cast<const unsigned short*>(y);
  const unsigned short* rp = static_cast<const unsigned short*>(res);
  float* sums = nullptr;
  if (mean_rstd || (slope && dslope)) {
    GS_REQUIRE(scratch, "gs_pnorm_backward: scratch required (normalisation or slope gradient)");
    const int ppb = pn_pix_per_block(d->pixels);
    const int chunks = (int)((d->pixels + ppb - 1) / ppb);
    sums = scratch + (size_t)d->N * chunks * 4 * d->C;
    // (COLS columns of one pixel are neighbouring 16-B loads: with one column per workgroup a 16- or 32-channel slice was
    // read as every second / fourth 16 bytes of a line by two / four different workgroups)
    norm_by_cols<32, 8, 4, 2, 1>(k.C8, [&](auto cols) {
      constexpr int COLS = decltype(cols)::value;
      hipLaunchKernelGGL((pnorm_bwd_reduce_kernel<COLS>), dim3(chunks, d->N, (k.C8 + COLS - 1) / COLS), dim3(256), 0, st, k, gp,
                         g2p, yp, mean_rstd, rp, slope, scratch, ppb, chunks);
    });
    GS_CHECK_HIP(hipGetLastError());
    // totals, and the slope and bias gradients: per-image totals added in image order (norm.hip), not by atomics. Narrow layers
    // with many chunks take 4 channels per workgroup.
    if (int rc = gs_launch_slot_sum(4, d->C < 128 && chunks > 256, scratch, sums, d->N, chunks, d->C, 1.0f / (float)d->pixels,
                                    mean_rstd, bias_grad, slope ? dslope : nullptr, st)) return rc;
  }
  hipLaunchKernelGGL(pnorm_bwd_apply_kernel, dim3(norm_grid((long long)k.HW * k.C8, 1024), d->N), dim3(256), 0, st, k, gp, g2p,
                     yp, mean_rstd, rp, slope, mean_rstd ? sums : nullptr, static_cast<unsigned short*>(dy),
                     static_cast<unsigned short*>(gres));
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- dst[view] (+)= src[view]: gradient joins of the coupling / skip graph --------------------------------------------
__global__ __launch_bounds__(256) void add_views_kernel(unsigned short* dst, int dcs, int dco, const unsigned short* src,
                                                        int scs, int sco, long long pixels, int C8, int accumulate) {
  const long long total = pixels * C8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long pix = e / C8;
    const int c8 = (int)(e - pix * C8);
    float a[8], b[8];
    unpack_bf8(b, *reinterpret_cast<const uint4*>(src + pix * scs + sco + c8 * 8));
    uint4* o = reinterpret_cast<uint4*>(dst + pix * dcs + dco + c8 * 8);
    if (accumulate) {
      unpack_bf8(a, *o);
#pragma unroll
      for (int k = 0; k < 8; ++k) b[k] += a[k];
    }
    *o = pack_bf8(b);
  }
}

extern "C" int gs_add_views(void* dst, int32_t dst_cs, int32_t dst_co, const void* src, int32_t src_cs, int32_t src_co,
                            int64_t pixels, int32_t C, int32_t accumulate, void* stream) {
  GS_REQUIRE(dst && src && pixels > 0 && C > 0 && ((C | dst_cs | dst_co | src_cs | src_co) & 7) == 0,
             "gs_add_views: bad argument (channel counts / strides / offsets must be multiples of 8)");
  hipLaunchKernelGGL(add_views_kernel, dim3(norm_grid(pixels * (C / 8), 4096)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned short*>(dst), dst_cs, dst_co, static_cast<const unsigned short*>(src), src_cs,
                     src_co, (long long)pixels, C / 8, accumulate);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- adjoint of x.repeat(1, C/Cin, 1, 1, 1) at the image boundary: g_img[n][c0][pix] += sum_{c = c0 mod Cin} g[pix][c] ---
__global__ __launch_bounds__(256) void repeat_bwd_kernel(const unsigned short* g, int cs, int co, float* g_img, int Cin,
                                                         int C, long long pixels) {
  const int n = blockIdx.y;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
    const unsigned short* row = g + ((size_t)n * pixels + p) * cs + co;
    for (int c0 = 0; c0 < Cin; ++c0) {
      float s = 0.f;
      for (int c = c0; c < C; c += Cin) s += bf2f(row[c]);
      g_img[((size_t)n * Cin + c0) * pixels + p] += s;
    }
  }
}

extern "C" int gs_repeat_backward(const void* g, int32_t g_cs, int32_t g_co, float* g_img, int32_t N, int32_t Cin,
                                  int32_t C, int64_t pixels, void* stream) {
  GS_REQUIRE(g && g_img && N > 0 && Cin > 0 && C >= Cin && C % Cin == 0 && pixels > 0, "gs_repeat_backward: bad argument");
  hipLaunchKernelGGL(repeat_bwd_kernel, dim3(norm_grid(pixels, 2048), N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const unsigned short*>(g), g_cs, g_co, g_img, Cin, C, (long long)pixels);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- statistics of a channel slice of an activation tensor -----------------------------------------------------------
// Piresnet3D's coupling function starts with an InstanceNorm of its INPUT half (piresnet3d.py:104-108), a tensor that no
// conv epilogue has seen: per (n, pixel chunk) partial sums [N][slots][2][C] in the layout gs_inorm_finalize reads.
// 256 threads = COLS 8-channel columns x 256/COLS pixel rows, 16-B loads.
template <int COLS>
__global__ __launch_bounds__(256) void slice_stats_kernel(const unsigned short* x, unsigned pixels, int cs, int co, int C8,
                                                          int C, float* partial, int pix_per_block, int slots) {
  constexpr int ROWS = 256 / COLS;
  __shared__ float red[ROWS][COLS][17];
  const int n = blockIdx.y, tid = threadIdx.x;
  const int col = tid % COLS, row = tid / COLS;
  const int c8 = blockIdx.z * COLS + col;
  const unsigned p0 = blockIdx.x * pix_per_block;
  const unsigned p1 = min(pixels, p0 + (unsigned)pix_per_block);
  float a[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = q[k] = 0.f;
  if (c8 < C8) {
    for (unsigned px = p0 + row; px < p1; px += ROWS) {
      float v[8];
      view8(v, x, (size_t)n * pixels + px, cs, co, c8);
#pragma unroll
      for (int k = 0; k < 8; ++k) { a[k] += v[k]; q[k] += v[k] * v[k]; }
    }
  }
  row_fold(red, partial, n, slots, C8, a, q);
}

extern "C" int32_t gs_slice_stats_slots(int64_t pixels) {
  long long ppb = (pixels + 255) / 256;
  if (ppb < 256) ppb = 256;
  return (int32_t)((pixels + ppb - 1) / ppb);
}
extern "C" int gs_slice_stats(const void* x, int32_t N, int64_t pixels, int32_t cs, int32_t co, int32_t C, float* partial,
                              void* stream) {
  GS_REQUIRE(x && partial && N > 0 && pixels > 0 && pixels < (1LL << 31) && C > 0 && (C & 7) == 0 && (cs & 7) == 0 &&
                 (co & 7) == 0,
             "gs_slice_stats: bad argument (C, cs, co multiples of 8)");
  const int slots = gs_slice_stats_slots(pixels);
  const int ppb = (int)((pixels + slots - 1) / slots);
  const int C8 = C / 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned short* xs = static_cast<const unsigned short*>(x);
  norm_by_cols<8, 4, 2, 1>(C8, [&](auto cols) {       // (this kernel's own list: no COLS 32)
    constexpr int COLS = decltype(cols)::value;
    hipLaunchKernelGGL((slice_stats_kernel<COLS>), dim3(slots, N, (C8 + COLS - 1) / COLS), dim3(256), 0, st, xs, (unsigned)pixels,
                       cs, co, C8, C, partial, ppb, slots);
  });
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
