// Validation / test image metrics (ganslate/utils/metrics/val_test_metrics.py:37-166) on the device.
// One call scores N samples of S = P*H*W fp32 elements (P planes of H x W) and writes one fp64 row per sample:
//   [mae, mse, nmse, psnr, ssim, nmi, histogram_chi2]   (columns whose flag is off hold NaN)
// Passes, in stream order (at most four launches):
//   1. moments   : per-workgroup fp64 partials of sum|t-p|, sum (t-p)^2, sum t^2 and min/max of t and p, into a slab;
//                  also zeroes the caller's histogram table
//   2. ssim      : 7x7 uniform-window SSIM (skimage structural_similarity defaults) over the (H-6)x(W-6) interior of every
//                  plane; R = max(t) of the sample is reduced from the moment slab on the device. Window sums in fp64.
//   3. histograms: 100-bin histograms of t and p and their 100x100 joint histogram with numpy's float32 bin edges,
//                  LDS-private uint32 counts, then one integer add per non-empty bin per workgroup
//   4. finalize  : one workgroup per sample reduces the slabs in a fixed order and writes the row
// No float atomics anywhere: the table is bitwise identical from run to run.
// Inputs are expected to be finite. numpy's np.histogram raises ValueError on a non-finite range; here inf / NaN values
// are binned without an error (the bin search settles on some bin) and the other metrics turn inf / NaN.
#include "common.hpp"

#include <math.h>

#define VM_THREADS 256
#define VM_BINS 100
#define VM_HIST_WORDS (2 * VM_BINS + VM_BINS * VM_BINS)
#define VM_MOM 8                // slab row per moments workgroup: sum|d|, sum d^2, sum t^2, min t, max t, min p, max p, -
#define VM_TW 64                // ssim tile: 64 interior columns x 32 interior rows, 4 row groups of 8 per column thread
#define VM_TH 32
#define VM_GROUP_ROWS 8

namespace {

int vm_moment_blocks(int64_t S) {
  const int64_t b = (S + 8191) / 8192;
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
int vm_hist_blocks(int64_t S) {      // 512 at the brats volume: 2 workgroups per CU (each holds 43 KB of LDS)
  const int64_t b = (S + 8191) / 8192;
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
// element range of workgroup b of nb over a sample of S elements: chunks are multiples of 1024 elements, so a 16-byte
// aligned sample base keeps every chunk 16-byte aligned
__device__ __forceinline__ void vm_chunk(int64_t S, int b, int nb, int64_t& b0, int64_t& b1) {
  const int64_t per = ((S + nb - 1) / nb + 1023) / 1024 * 1024;
  b0 = (int64_t)b * per;
  b1 = b0 + per < S ? b0 + per : S;
  if (b0 > S) b0 = S;
}

template <class F>
__device__ __forceinline__ void vm_for_chunk(const float* t, const float* p, int64_t b0, int64_t b1, bool vec, F&& f) {
  int64_t i = b0;
  if (vec) {
    const int64_t n4 = (b1 - b0) / 4;
    const float4* t4 = reinterpret_cast<const float4*>(t + b0);
    const float4* p4 = reinterpret_cast<const float4*>(p + b0);
    for (int64_t k = threadIdx.x; k < n4; k += VM_THREADS) {
      const float4 a = t4[k], b = p4[k];
      f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
    }
    i = b0 + n4 * 4;
  }
  for (int64_t k = i + threadIdx.x; k < b1; k += VM_THREADS) f(t[k], p[k]);
}

// fixed-order workgroup reductions (256 threads): the result is in every thread
__device__ double vm_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = VM_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// fixed-order min / max trees of four values (min, max, min, max) across the workgroup: the result is in every thread
__device__ void vm_block_minmax4(const double v[4], double* sh, double out[4]) {
  for (int q = 0; q < 4; ++q) {
    __syncthreads();
    sh[threadIdx.x] = v[q];
    __syncthreads();
    for (int o = VM_THREADS / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o)
        sh[threadIdx.x] = (q & 1) ? fmax(sh[threadIdx.x], sh[threadIdx.x + o]) : fmin(sh[threadIdx.x], sh[threadIdx.x + o]);
      __syncthreads();
    }
    out[q] = sh[0];
  }
  __syncthreads();
}

// min / max of t and p of sample n from the moment slab (every thread gets them)
__device__ void vm_sample_range(const double* mom, int nb, float* out4, double* sh) {
  double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY}, r4[4];
  for (int b = threadIdx.x; b < nb; b += VM_THREADS) {
    const double* r = mom + (size_t)b * VM_MOM;
    v[0] = fmin(v[0], r[3]); v[1] = fmax(v[1], r[4]); v[2] = fmin(v[2], r[5]); v[3] = fmax(v[3], r[6]);
  }
  vm_block_minmax4(v, sh, r4);
  for (int q = 0; q < 4; ++q) out4[q] = (float)r4[q];
}

// numpy's histogram range and float32 bin edges (numpy/lib/_histograms_impl.py _get_outer_edges / _get_bin_edges and
// numpy/_core/function_base.py linspace, evaluated in float32): explicit roundings, so no contraction changes a bit
__device__ __forceinline__ void vm_outer_edges(float lo, float hi, float& first, float& last) {
  if (lo == hi) { first = __fsub_rn(lo, 0.5f); last = __fadd_rn(hi, 0.5f); }
  else { first = lo; last = hi; }
}
__device__ __forceinline__ float vm_edge(float first, float last, int k) {
  if (k == VM_BINS) return last;
  const float delta = __fsub_rn(last, first);
  const float step = __fdiv_rn(delta, (float)VM_BINS);
  const float y = step == 0.f ? __fmul_rn(__fdiv_rn((float)k, (float)VM_BINS), delta) : __fmul_rn((float)k, step);
  return __fadd_rn(y, first);
}
// the largest i <= 99 with edges[i] <= x (what np.histogram and np.histogramdd both compute for in-range x)
__device__ __forceinline__ int vm_bin(float x, const float* e, float first, float scale) {
  int i = (int)fminf(fmaxf((x - first) * scale, 0.f), (float)(VM_BINS - 1));
  while (i > 0 && x < e[i]) --i;
  while (i < VM_BINS - 1 && x >= e[i + 1]) ++i;
  return i;
}

// ---- pass 1: moments ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VM_THREADS) void vm_moments_kernel(const float* t, const float* p, int64_t S, int nb,
                                                                bool vec, double* mom, unsigned* counts) {
  __shared__ double sh[VM_THREADS];
  const int n = blockIdx.x / nb, b = blockIdx.x % nb;
  if (counts) {
    unsigned* c = counts + (size_t)n * VM_HIST_WORDS;
    for (int i = b * VM_THREADS + threadIdx.x; i < VM_HIST_WORDS; i += nb * VM_THREADS) c[i] = 0u;
  }
  int64_t b0, b1;
  vm_chunk(S, b, nb, b0, b1);
  double sad = 0.0, ssd = 0.0, stt = 0.0;
  float tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY;
  vm_for_chunk(t + (size_t)n * S, p + (size_t)n * S, b0, b1, vec, [&](float a, float c) {
    const double d = (double)a - (double)c;
    sad += fabs(d); ssd += d * d; stt += (double)a * (double)a;
    tmin = fminf(tmin, a); tmax = fmaxf(tmax, a); pmin = fminf(pmin, c); pmax = fmaxf(pmax, c);
  });
  double* r = mom + (size_t)blockIdx.x * VM_MOM;
  sad = vm_block_sum(sad, sh);
  ssd = vm_block_sum(ssd, sh);
  stt = vm_block_sum(stt, sh);
  const double m[4] = {(double)tmin, (double)tmax, (double)pmin, (double)pmax};
  double red[4];
  vm_block_minmax4(m, sh, red);
  if (threadIdx.x == 0) {
    r[0] = sad; r[1] = ssd; r[2] = stt; r[3] = red[0]; r[4] = red[1]; r[5] = red[2]; r[6] = red[3]; r[7] = 0.0;
  }
}

// ---- pass 2: SSIM ---------------------------------------------------------------------------------------------------
// One workgroup = a 32 x 64 tile of the interior of one plane. Thread (column c, row group g) walks 14 input rows with
// a running fp64 sum of the five 7-tap row sums (t, p, tt, pp, tp) and scores 8 interior pixels of its column. Each row
// sum is computed once: the first seven are kept in registers (fully unrolled loop, constant indices) and subtracted
// again when the window leaves them.
__device__ __forceinline__ void vm_row7(const float (*st)[VM_TW + 6], const float (*sp)[VM_TW + 6], int r, int c,
                                       double h[5]) {
  h[0] = h[1] = h[2] = h[3] = h[4] = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double a = st[r][c + k], b = sp[r][c + k];
    h[0] += a; h[1] += b; h[2] += a * a; h[3] += b * b; h[4] += a * b;
  }
}

__global__ __launch_bounds__(VM_THREADS) void vm_ssim_kernel(const float* t, const float* p, int P, int H, int W,
                                                             int tiles_w, int tiles_h, int nb_mom, const double* mom,
                                                             double* partial) {
  __shared__ float st[VM_TH + 6][VM_TW + 6];
  __shared__ float sp[VM_TH + 6][VM_TW + 6];
  __shared__ double sh[VM_THREADS];
  int q = blockIdx.x;
  const int tw = q % tiles_w; q /= tiles_w;
  const int th = q % tiles_h; const int plane = q / tiles_h;
  const int n = plane / P;
  float rg[4];
  vm_sample_range(mom + (size_t)n * nb_mom * VM_MOM, nb_mom, rg, sh);
  const int Ho = H - 6, Wo = W - 6;
  const int y0 = th * VM_TH, x0 = tw * VM_TW;
  const float* tp = t + (size_t)plane * H * W;
  const float* pp = p + (size_t)plane * H * W;
  for (int e = threadIdx.x; e < (VM_TH + 6) * (VM_TW + 6); e += VM_THREADS) {
    const int r = e / (VM_TW + 6), c = e % (VM_TW + 6);
    const int y = y0 + r, x = x0 + c;
    float a = 0.f, b = 0.f;
    if (y < H && x < W) { a = tp[(size_t)y * W + x]; b = pp[(size_t)y * W + x]; }
    st[r][c] = a; sp[r][c] = b;
  }
  __syncthreads();
  const double R = (double)rg[1];
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
  const double inv = 1.0 / 49.0, cov = 49.0 / 48.0;
  const int c = threadIdx.x % VM_TW, g = threadIdx.x / VM_TW;
  double acc = 0.0;
  if (x0 + c < Wo && y0 + g * VM_GROUP_ROWS < Ho) {
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, ring[7][5];
    const int r0 = g * VM_GROUP_ROWS;
#pragma unroll
    for (int r = 0; r < VM_GROUP_ROWS + 6; ++r) {
      double h[5];
      vm_row7(st, sp, r0 + r, c, h);
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] += h[k];
      if (r >= 7) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] -= ring[r - 7][k];
      } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) ring[r][k] = h[k];
      }
      if (r >= 6 && y0 + r0 + r - 6 < Ho) {
        const double ux = v[0] * inv, uy = v[1] * inv, uxx = v[2] * inv, uyy = v[3] * inv, uxy = v[4] * inv;
        const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        acc += (A1 * A2) / (B1 * B2);
      }
    }
  }
  acc = vm_block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---- pass 3: histograms ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VM_THREADS) void vm_hist_kernel(const float* t, const float* p, int64_t S, int nb,
                                                             bool vec, int nb_mom, const double* mom,
                                                             unsigned* counts) {
  __shared__ unsigned h[VM_HIST_WORDS];       // [t bins][p bins][t bin * 100 + p bin]
  __shared__ float et[VM_BINS + 1], ep[VM_BINS + 1];
  __shared__ double sh[VM_THREADS];
  const int n = blockIdx.x / nb, b = blockIdx.x % nb;
  float rg[4];
  vm_sample_range(mom + (size_t)n * nb_mom * VM_MOM, nb_mom, rg, sh);
  float ft, lt, fp, lp;
  vm_outer_edges(rg[0], rg[1], ft, lt);
  vm_outer_edges(rg[2], rg[3], fp, lp);
  for (int i = threadIdx.x; i < VM_HIST_WORDS; i += VM_THREADS) h[i] = 0u;
  if (threadIdx.x <= VM_BINS) { et[threadIdx.x] = vm_edge(ft, lt, threadIdx.x); ep[threadIdx.x] = vm_edge(fp, lp, threadIdx.x); }
  __syncthreads();
  const float scale_t = (float)VM_BINS / (lt - ft), scale_p = (float)VM_BINS / (lp - fp);
  int64_t b0, b1;
  vm_chunk(S, b, nb, b0, b1);
  vm_for_chunk(t + (size_t)n * S, p + (size_t)n * S, b0, b1, vec, [&](float a, float c) {
    const int i = vm_bin(a, et, ft, scale_t), j = vm_bin(c, ep, fp, scale_p);
    atomicAdd(&h[i], 1u);
    atomicAdd(&h[VM_BINS + j], 1u);
    atomicAdd(&h[2 * VM_BINS + i * VM_BINS + j], 1u);
  });
  __syncthreads();
  unsigned* out = counts + (size_t)n * VM_HIST_WORDS;
  for (int i = threadIdx.x; i < VM_HIST_WORDS; i += VM_THREADS)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

// ---- pass 4: finalize -----------------------------------------------------------------------------------------------
__device__ double vm_entr(double x) { return x > 0.0 ? -x * log(x) : 0.0; }

__global__ __launch_bounds__(VM_THREADS) void vm_final_kernel(int64_t S, int P, int H, int W, int nb_mom,
                                                              const double* mom, int ssim_blocks, const double* ssim_part,
                                                              const unsigned* counts, double* table) {
  __shared__ double sh[VM_THREADS];
  __shared__ double rowsum[VM_BINS], colsum[VM_BINS];
  __shared__ float wt[VM_BINS], wp[VM_BINS];
  const int n = blockIdx.x;
  const double* m = mom + (size_t)n * nb_mom * VM_MOM;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb_mom; b += VM_THREADS)
    for (int k = 0; k < 3; ++k) s[k] += m[(size_t)b * VM_MOM + k];
  const double sad = vm_block_sum(s[0], sh), ssd = vm_block_sum(s[1], sh), stt = vm_block_sum(s[2], sh);
  float rg[4];
  vm_sample_range(m, nb_mom, rg, sh);
  const double nan = __builtin_nan("");
  double row[7] = {nan, nan, nan, nan, nan, nan, nan};
  const double mse = ssd / (double)S;
  row[0] = sad / (double)S;
  row[1] = mse;
  row[2] = ssd / stt;
  const double R = (double)rg[1];
  row[3] = 10.0 * log10((R * R) / mse);
  if (ssim_part) {
    const double* sp = ssim_part + (size_t)n * ssim_blocks;
    double a = 0.0;
    for (int b = threadIdx.x; b < ssim_blocks; b += VM_THREADS) a += sp[b];
    a = vm_block_sum(a, sh);
    row[4] = a / ((double)P * (double)(H - 6) * (double)(W - 6));
  }
  if (counts) {
    const unsigned* c = counts + (size_t)n * VM_HIST_WORDS;
    // histogram_chi2: each histogram normalised to sum 1 (the sum is S), 0/0 bins dropped
    double chi = 0.0;
    if (threadIdx.x < VM_BINS) {
      const double g = (double)c[threadIdx.x] / (double)S, q = (double)c[VM_BINS + threadIdx.x] / (double)S;
      if (g + q != 0.0) chi = (q - g) * (q - g) / (q + g);
    }
    row[6] = vm_block_sum(chi, sh);
    // nmi: np.histogramdd([t, p], bins=100, density=True) = ((count / wt[i]) / wp[j]) / S with float32 widths
    float ft, lt, fp, lp;
    vm_outer_edges(rg[0], rg[1], ft, lt);
    vm_outer_edges(rg[2], rg[3], fp, lp);
    if (threadIdx.x < VM_BINS) {
      wt[threadIdx.x] = __fsub_rn(vm_edge(ft, lt, threadIdx.x + 1), vm_edge(ft, lt, threadIdx.x));
      wp[threadIdx.x] = __fsub_rn(vm_edge(fp, lp, threadIdx.x + 1), vm_edge(fp, lp, threadIdx.x));
    }
    __syncthreads();
    const unsigned* cj = c + 2 * VM_BINS;
    auto dens = [&](int i, int j) { return (((double)cj[i * VM_BINS + j] / (double)wt[i]) / (double)wp[j]) / (double)S; };
    if (threadIdx.x < VM_BINS) {
      double a = 0.0;
      for (int j = 0; j < VM_BINS; ++j) a += dens(threadIdx.x, j);
      rowsum[threadIdx.x] = a;
    } else if (threadIdx.x >= 128 && threadIdx.x < 128 + VM_BINS) {
      const int j = threadIdx.x - 128;
      double a = 0.0;
      for (int i = 0; i < VM_BINS; ++i) a += dens(i, j);
      colsum[j] = a;
    }
    __syncthreads();
    double tr = 0.0, tc = 0.0, tj = 0.0;
    if (threadIdx.x < VM_BINS) { tr = rowsum[threadIdx.x]; tc = colsum[threadIdx.x]; }
    for (int e = threadIdx.x; e < VM_BINS * VM_BINS; e += VM_THREADS) tj += dens(e / VM_BINS, e % VM_BINS);
    const double Tr = vm_block_sum(tr, sh), Tc = vm_block_sum(tc, sh), Tj = vm_block_sum(tj, sh);
    double er = 0.0, ec = 0.0, ej = 0.0;
    if (threadIdx.x < VM_BINS) { er = vm_entr(rowsum[threadIdx.x] / Tr); ec = vm_entr(colsum[threadIdx.x] / Tc); }
    for (int e = threadIdx.x; e < VM_BINS * VM_BINS; e += VM_THREADS) ej += vm_entr(dens(e / VM_BINS, e % VM_BINS) / Tj);
    const double H0 = vm_block_sum(ec, sh), H1 = vm_block_sum(er, sh), H01 = vm_block_sum(ej, sh);
    row[5] = (H0 + H1) / H01;
  }
  if (threadIdx.x < 7) table[(size_t)n * 7 + threadIdx.x] = row[threadIdx.x];
}

struct VmPlan {
  int64_t S;
  int nb_mom, nb_hist, tiles_w, tiles_h;
  size_t mom_doubles, ssim_doubles;
};
VmPlan vm_plan(int32_t N, int32_t P, int32_t H, int32_t W) {
  VmPlan q;
  q.S = (int64_t)P * H * W;
  q.nb_mom = vm_moment_blocks(q.S);
  q.nb_hist = vm_hist_blocks(q.S);
  q.tiles_w = W > 6 ? (W - 6 + VM_TW - 1) / VM_TW : 0;
  q.tiles_h = H > 6 ? (H - 6 + VM_TH - 1) / VM_TH : 0;
  q.mom_doubles = (size_t)N * q.nb_mom * VM_MOM;
  q.ssim_doubles = (size_t)N * P * q.tiles_w * q.tiles_h;
  return q;
}

}  // namespace

extern "C" int64_t gs_valmetric_scratch_bytes(int32_t N, int32_t P, int32_t H, int32_t W) {
  if (N <= 0 || P <= 0 || H <= 0 || W <= 0) return 0;
  const VmPlan q = vm_plan(N, P, H, W);
  return (int64_t)((q.mom_doubles + q.ssim_doubles) * sizeof(double));
}

extern "C" int gs_valmetrics(const float* t, const float* p, int32_t N, int32_t P, int32_t H, int32_t W, int32_t flags,
                             double* table, uint32_t* counts, void* scratch, void* stream) {
  GS_REQUIRE(t && p && table && scratch && N > 0 && P > 0 && H > 0 && W > 0 &&
             (flags & ~(GS_VM_SSIM | GS_VM_HIST)) == 0, "gs_valmetrics: bad argument");
  GS_REQUIRE(!(flags & GS_VM_SSIM) || (H >= 7 && W >= 7), "gs_valmetrics: SSIM needs H >= 7 and W >= 7 (7x7 window)");
  GS_REQUIRE(!(flags & GS_VM_HIST) || counts, "gs_valmetrics: histograms need the counts table");
  const VmPlan q = vm_plan(N, P, H, W);
  GS_REQUIRE(q.S < ((int64_t)1 << 32), "gs_valmetrics: a sample must hold fewer than 2^32 elements (uint32 counts)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* mom = static_cast<double*>(scratch);
  double* ssim_part = mom + q.mom_doubles;
  unsigned* cnt = (flags & GS_VM_HIST) ? counts : nullptr;
  const bool vec = ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(p)) & 15) == 0 && q.S % 4 == 0;
  hipLaunchKernelGGL(vm_moments_kernel, dim3(N * q.nb_mom), dim3(VM_THREADS), 0, st, t, p, q.S, q.nb_mom, vec, mom, cnt);
  const int ssim_blocks = P * q.tiles_w * q.tiles_h;
  if (flags & GS_VM_SSIM)
    hipLaunchKernelGGL(vm_ssim_kernel, dim3(N * ssim_blocks), dim3(VM_THREADS), 0, st, t, p, P, H, W, q.tiles_w,
                       q.tiles_h, q.nb_mom, mom, ssim_part);
  if (flags & GS_VM_HIST)
    hipLaunchKernelGGL(vm_hist_kernel, dim3(N * q.nb_hist), dim3(VM_THREADS), 0, st, t, p, q.S, q.nb_hist, vec,
                       q.nb_mom, mom, cnt);
  hipLaunchKernelGGL(vm_final_kernel, dim3(N), dim3(VM_THREADS), 0, st, q.S, P, H, W, q.nb_mom, mom, ssim_blocks,
                     (flags & GS_VM_SSIM) ? ssim_part : nullptr, cnt, table);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
