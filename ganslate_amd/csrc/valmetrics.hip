// Validation / test image metrics (ganslate/utils/metrics/val_test_metrics.py:37-166) on the device.
// One call scores N samples of S = P*H*W fp32 elements (P planes of H x W) and writes one fp64 row per sample:
//   [mae, mse, nmse, psnr, ssim, nmi, histogram_chi2]   (columns whose flag is off hold NaN)
// gs_valmetrics scores whole samples; gs_valmetrics_masked (validator_tester.py:78-98, val_test_metrics.py:19-29,141-149)
// scores every sample inside L <= VM_MAX_LABELS region masks, one row per (sample, label). What the reference's masked
// arrays make of each metric is stated at gs_valmetrics_masked in ganslate_hip.h. tm = t*m and pm = p*m exist nowhere in
// memory: the masks are packed once into one byte per element (bit l = label l) and applied where t and p are loaded.
// Both entry points are one host body (vm_run<MASKED>) and, but for the moments, one kernel body per pass; what the two
// paths do differently is collected in VmPath<MASKED>. Passes, in stream order (plain at most four launches, masked at
// most five, whatever L is):
//   0. pack      : (masked only) L byte masks -> one bit per label
//   1. moments   : per-workgroup fp64 partials into a slab, and zeroes the caller's histogram table. Plain: sum|t-p|,
//                  sum (t-p)^2, sum t^2 and min/max of t and p. Masked (a kernel of its own: it keeps every label in
//                  registers and reads t, p and the bits once): per label sum_m |t-p|, sum_m (t-p)^2, sum_m t^2, n,
//                  Rm = max of t inside the mask, and min / max of tm and pm (the histogram ranges)
//   2. ssim      : 7x7 uniform-window SSIM (skimage structural_similarity defaults) over the (H-6)x(W-6) interior of every
//                  plane, one workgroup per (tile, label), label fastest; the data range R (max t, or Rm) is reduced from
//                  the moment slab on the device. Window sums in fp64.
//   3. histograms: 100-bin histograms of t and p and their 100x100 joint histogram with numpy's float32 bin edges,
//                  LDS-private uint32 counts, then one integer add per non-empty bin per workgroup. One workgroup per
//                  (chunk, label), label fastest: a workgroup's joint table is 40 KB, so L of them would leave one
//                  workgroup per CU at L = 3 and do not fit the CU's 160 KB from L = 4 on; with one label per workgroup
//                  three workgroups share a CU whatever L is, and the L workgroups of a chunk run side by side and share
//                  its lines in L2. Masked-out elements all fall into the bin of 0: they are counted in a register and
//                  added once, not by same-address LDS atomics.
//   4. finalize  : one workgroup per (sample, label) reduces the slabs in a fixed order and writes the row
// No float atomics anywhere, and every reduction has a fixed order (plain: a 256-wide halving tree; masked: xor
// butterflies in each wave, then the four waves in index order): the table is bitwise identical from run to run.
// Inputs are expected to be finite. numpy's np.histogram raises ValueError on a non-finite range; here inf / NaN values
// are binned without an error (the bin search settles on some bin) and the other metrics turn inf / NaN.
#include "common.hpp"

#include <math.h>

#define VM_THREADS 256
#define VM_BINS 100
#define VM_HIST_WORDS (2 * VM_BINS + VM_BINS * VM_BINS)
#define VM_MAX_LABELS GS_VM_MAX_LABELS
#define VM_MOM 8                // plain slab row per moments workgroup: sum|d|, sum d^2, sum t^2, min t, max t, min p, max p, -
#define VMM_MOM 10              // masked slab row per (moments workgroup, label): sum|d|, sum d^2, sum t^2, n, Rm, min tm,
                                // max tm, min pm, max pm, -
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

// f(t[k], p[k], mask byte of k) for k in [b0, b1). MASKED: m holds the packed bits, one byte per element; otherwise m is
// not read and f gets 0
template <bool MASKED, class F>
__device__ __forceinline__ void vm_for_chunk(const float* t, const float* p, const uint8_t* m, int64_t b0, int64_t b1,
                                             bool vec, F&& f) {
  int64_t i = b0;
  if (vec) {
    const int64_t n4 = (b1 - b0) / 4;
    const float4* t4 = reinterpret_cast<const float4*>(t + b0);
    const float4* p4 = reinterpret_cast<const float4*>(p + b0);
    for (int64_t k = threadIdx.x; k < n4; k += VM_THREADS) {
      const float4 a = t4[k], b = p4[k];
      const unsigned w = MASKED ? reinterpret_cast<const unsigned*>(m + b0)[k] : 0u;
      f(a.x, b.x, w & 255u); f(a.y, b.y, (w >> 8) & 255u); f(a.z, b.z, (w >> 16) & 255u); f(a.w, b.w, w >> 24);
    }
    i = b0 + n4 * 4;
  }
  for (int64_t k = i + threadIdx.x; k < b1; k += VM_THREADS) f(t[k], p[k], MASKED ? (unsigned)m[k] : 0u);
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

// workgroup reduction of K values at once; bit k of maxbits / minbits makes v[k] a max / a min, otherwise a sum. Xor
// butterflies inside each wave, then the four waves in index order: the same order every run. Result in every thread.
template <int K>
__device__ __forceinline__ void vmm_block_reduce(double (&v)[K], unsigned minbits, unsigned maxbits, double* sh) {
  auto op = [&](int k, double a, double b) {
    return ((maxbits >> k) & 1) ? fmax(a, b) : ((minbits >> k) & 1) ? fmin(a, b) : a + b;
  };
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] = op(k, v[k], __shfl_xor(v[k], o, 64));
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = op(k, op(k, op(k, sh[k], sh[K + k]), sh[2 * K + k]), sh[3 * K + k]);
  __syncthreads();
}

// What the plain and the masked path do differently after the moments: the slab row, which of its columns the finalize
// sums and which hold the ranges, and the reduction. The plain path is the masked layout at L = 1, label = 0 with its
// own row. Each path keeps its own reduction (here and in the finalize): its order is part of the result's bits.
template <bool MASKED>
struct VmPath {
  static constexpr int MOM = MASKED ? VMM_MOM : VM_MOM;
  static constexpr int SUMS = MASKED ? 4 : 3;       // leading columns the finalize sums (masked: n too, its divisor)

  // the slab rows of sample n, and the row of (moments workgroup b, label) among them
  static __device__ __forceinline__ const double* sample(const double* mom, int n, int nb, int L) {
    return mom + (size_t)n * nb * L * MOM;
  }
  static __device__ __forceinline__ const double* row(const double* mom, int b, int L, int label) {
    return mom + ((size_t)b * L + label) * MOM;
  }

  // rg = {R, min t, max t, min p, max p} of (sample, label) from the sample's slab rows (every thread gets them): the
  // data range of psnr / ssim and the histogram ranges. Plain: R = max t; masked: R = Rm, and t, p stand for tm, pm
  static __device__ void range(const double* mom, int nb, int L, int label, float* rg, double* sh) {
    if constexpr (MASKED) {
      double v[5] = {-INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
      for (int b = threadIdx.x; b < nb; b += VM_THREADS) {
        const double* r = row(mom, b, L, label);
        v[0] = fmax(v[0], r[4]); v[1] = fmin(v[1], r[5]); v[2] = fmax(v[2], r[6]); v[3] = fmin(v[3], r[7]);
        v[4] = fmax(v[4], r[8]);
      }
      vmm_block_reduce<5>(v, 0x0au, 0x15u, sh);
      for (int q = 0; q < 5; ++q) rg[q] = (float)v[q];
    } else {
      double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY}, r4[4];
      for (int b = threadIdx.x; b < nb; b += VM_THREADS) {
        const double* r = row(mom, b, L, label);
        v[0] = fmin(v[0], r[3]); v[1] = fmax(v[1], r[4]); v[2] = fmin(v[2], r[5]); v[3] = fmax(v[3], r[6]);
      }
      vm_block_minmax4(v, sh, r4);
      for (int q = 0; q < 4; ++q) rg[1 + q] = (float)r4[q];
      rg[0] = rg[2];
    }
  }
};

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

// ---- pass 0 (masked): pack ------------------------------------------------------------------------------------------
struct VmMaskPtrs { const uint8_t* m[VM_MAX_LABELS]; };

// bit l of out[i] = (masks[l][i] != 0). words = the number of leading 4-byte groups handled a word at a time (0 when a
// mask is not 4-byte aligned); the bytes after them go one by one.
__global__ __launch_bounds__(VM_THREADS) void vmm_pack_kernel(VmMaskPtrs mk, int L, int64_t words, int64_t total,
                                                              uint8_t* out) {
  const int64_t stride = (int64_t)gridDim.x * VM_THREADS;
  const int64_t i0 = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x;
  for (int64_t i = i0; i < words; i += stride) {
    unsigned r = 0u;
    for (int l = 0; l < L; ++l) {
      const unsigned w = reinterpret_cast<const unsigned*>(mk.m[l])[i];
      r |= (((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u) << l;      // 1 in every non-zero byte
    }
    reinterpret_cast<unsigned*>(out)[i] = r;
  }
  for (int64_t i = words * 4 + i0; i < total; i += stride) {
    unsigned r = 0u;
    for (int l = 0; l < L; ++l) r |= (mk.m[l][i] != 0 ? 1u : 0u) << l;
    out[i] = (uint8_t)r;
  }
}

// ---- pass 1: moments (a kernel per path: 40 VGPRs plain, 162 with up to 8 labels in registers) -----------------------
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
  vm_for_chunk<false>(t + (size_t)n * S, p + (size_t)n * S, nullptr, b0, b1, vec, [&](float a, float c, unsigned) {
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

__global__ __launch_bounds__(VM_THREADS) void vmm_moments_kernel(const float* t, const float* p, const uint8_t* bits,
                                                                 int L, int64_t S, int nb, bool vec, double* mom,
                                                                 unsigned* counts) {
  __shared__ double sh[VM_THREADS];
  const int n = blockIdx.x / nb, b = blockIdx.x % nb;
  if (counts) {
    unsigned* c = counts + (size_t)n * L * VM_HIST_WORDS;
    for (int i = b * VM_THREADS + threadIdx.x; i < L * VM_HIST_WORDS; i += nb * VM_THREADS) c[i] = 0u;
  }
  int64_t b0, b1;
  vm_chunk(S, b, nb, b0, b1);
  double sad[VM_MAX_LABELS], ssd[VM_MAX_LABELS], stt[VM_MAX_LABELS];
  unsigned cnt[VM_MAX_LABELS];
  float rm[VM_MAX_LABELS], tmin[VM_MAX_LABELS], tmax[VM_MAX_LABELS], pmin[VM_MAX_LABELS], pmax[VM_MAX_LABELS];
#pragma unroll
  for (int l = 0; l < VM_MAX_LABELS; ++l) {
    sad[l] = ssd[l] = stt[l] = 0.0; cnt[l] = 0u;
    rm[l] = -INFINITY; tmin[l] = pmin[l] = INFINITY; tmax[l] = pmax[l] = -INFINITY;
  }
  vm_for_chunk<true>(t + (size_t)n * S, p + (size_t)n * S, bits + (size_t)n * S, b0, b1, vec,
                     [&](float a, float c, unsigned w) {
    const double d = (double)a - (double)c;
    const double ad = fabs(d), dd = d * d, aa = (double)a * (double)a;
#pragma unroll
    for (int l = 0; l < VM_MAX_LABELS; ++l) {
      if (l < L) {
        const bool in = (w >> l) & 1u;
        sad[l] += in ? ad : 0.0; ssd[l] += in ? dd : 0.0; stt[l] += in ? aa : 0.0;
        cnt[l] += in ? 1u : 0u;
        rm[l] = in ? fmaxf(rm[l], a) : rm[l];
        const float ta = in ? a : 0.f, pa = in ? c : 0.f;
        tmin[l] = fminf(tmin[l], ta); tmax[l] = fmaxf(tmax[l], ta);
        pmin[l] = fminf(pmin[l], pa); pmax[l] = fmaxf(pmax[l], pa);
      }
    }
  });
#pragma unroll
  for (int l = 0; l < VM_MAX_LABELS; ++l) {
    if (l < L) {
      double v[9] = {sad[l], ssd[l], stt[l], (double)cnt[l], (double)rm[l], (double)tmin[l], (double)tmax[l],
                     (double)pmin[l], (double)pmax[l]};
      vmm_block_reduce<9>(v, 0x0a0u, 0x150u, sh);
      if (threadIdx.x == 0) {
        double* r = mom + ((size_t)blockIdx.x * L + l) * VMM_MOM;
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = v[k];
        r[9] = 0.0;
      }
    }
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

// (A1 A2) / (B1 B2) of one pixel, every product rounded before the sums as numpy rounds them (structural_similarity's
// own statements): contracted to fmas, 2 ux uy + C1 rounds once and ux ux + uy uy + C1 twice, so identical images score
// 1 - 2^-53 on some pixels instead of exactly 1 (csrc/loss.hip, ssim_terms, has the fp32 case, where a root amplifies it)
__device__ __forceinline__ double vm_ssim_pixel(double ux, double uy, double uxx, double uyy, double uxy, double C1,
                                                double C2, double cov) {
#pragma clang fp contract(off)
  const double pxx = ux * ux, pyy = uy * uy, pxy = ux * uy;
  const double vx = cov * (uxx - pxx), vy = cov * (uyy - pyy), vxy = cov * (uxy - pxy);
  const double A1 = 2.0 * pxy + C1, A2 = 2.0 * vxy + C2;
  const double B1 = (pxx + pyy) + C1, B2 = (vx + vy) + C2;
  return (A1 * A2) / (B1 * B2);
}

// stages the (32+6) x (64+6) patch at (y0, x0) of one plane (MASKED: an element whose bit `label` of `bits` is clear is
// staged as 0, so t*m and p*m exist in LDS only) and returns the workgroup's sum of the SSIM map over the tile's interior
// pixels (in every thread)
template <bool MASKED>
__device__ __forceinline__ double vm_ssim_tile(const float* tp, const float* pp, const uint8_t* bits, int label, int H,
                                               int W, int y0, int x0, double R, float (*st)[VM_TW + 6],
                                               float (*sp)[VM_TW + 6], double* sh) {
  const int Ho = H - 6, Wo = W - 6;
  for (int e = threadIdx.x; e < (VM_TH + 6) * (VM_TW + 6); e += VM_THREADS) {
    const int r = e / (VM_TW + 6), c = e % (VM_TW + 6);
    const int y = y0 + r, x = x0 + c;
    float a = 0.f, b = 0.f;
    if (y < H && x < W) {
      a = tp[(size_t)y * W + x]; b = pp[(size_t)y * W + x];
      if (MASKED && !((bits[(size_t)y * W + x] >> label) & 1)) { a = 0.f; b = 0.f; }
    }
    st[r][c] = a; sp[r][c] = b;
  }
  __syncthreads();
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
        acc += vm_ssim_pixel(ux, uy, uxx, uyy, uxy, C1, C2, cov);
      }
    }
  }
  return vm_block_sum(acc, sh);
}

// In the three kernels below `labels` is L of the masked call; the plain instantiations ignore it and `bits`: L = 1,
// label = 0 fold away.
template <bool MASKED>
__global__ __launch_bounds__(VM_THREADS) void vm_ssim_kernel(const float* t, const float* p, const uint8_t* bits,
                                                             int labels, int P, int H, int W, int tiles_w, int tiles_h,
                                                             int nb_mom, const double* mom, double* partial) {
  using Path = VmPath<MASKED>;
  __shared__ float st[VM_TH + 6][VM_TW + 6];
  __shared__ float sp[VM_TH + 6][VM_TW + 6];
  __shared__ double sh[VM_THREADS];
  const int L = MASKED ? labels : 1;
  int q = blockIdx.x;
  const int label = q % L; q /= L;
  const int tw = q % tiles_w; q /= tiles_w;
  const int th = q % tiles_h; const int plane = q / tiles_h;
  const int n = plane / P;
  float rg[5];
  Path::range(Path::sample(mom, n, nb_mom, L), nb_mom, L, label, rg, sh);
  const size_t off = (size_t)plane * H * W;
  const double acc = vm_ssim_tile<MASKED>(t + off, p + off, MASKED ? bits + off : nullptr, label, H, W, th * VM_TH, tw * VM_TW,
                                          (double)rg[0], st, sp, sh);
  // partial[(n, label)][plane of n][tile]: the finalize sums a (sample, label) run in one order whatever L is. At L = 1
  // that index is blockIdx.x.
  if (threadIdx.x == 0) {
    const int per = P * tiles_h * tiles_w;
    partial[MASKED ? ((size_t)n * L + label) * per + ((size_t)(plane - n * P) * tiles_h + th) * tiles_w + tw
                   : (size_t)blockIdx.x] = acc;
  }
}

// ---- pass 3: histograms ---------------------------------------------------------------------------------------------
template <bool MASKED>
__global__ __launch_bounds__(VM_THREADS) void vm_hist_kernel(const float* t, const float* p, const uint8_t* bits,
                                                             int labels, int64_t S, int nb, bool vec, int nb_mom,
                                                             const double* mom, unsigned* counts) {
  using Path = VmPath<MASKED>;
  __shared__ unsigned h[VM_HIST_WORDS];       // [t bins][p bins][t bin * 100 + p bin]
  __shared__ float et[VM_BINS + 1], ep[VM_BINS + 1];
  __shared__ double sh[VM_THREADS];
  const int L = MASKED ? labels : 1;
  std::conditional_t<MASKED, int, unsigned> q = blockIdx.x;       // signed or not on purpose: DESIGN.md 4.11
  const int label = q % L; q /= L;
  const int n = q / nb, b = q % nb;
  float rg[5];
  Path::range(Path::sample(mom, n, nb_mom, L), nb_mom, L, label, rg, sh);
  float ft, lt, fp, lp;
  vm_outer_edges(rg[1], rg[2], ft, lt);
  vm_outer_edges(rg[3], rg[4], fp, lp);
  for (int i = threadIdx.x; i < VM_HIST_WORDS; i += VM_THREADS) h[i] = 0u;
  if (threadIdx.x <= VM_BINS) { et[threadIdx.x] = vm_edge(ft, lt, threadIdx.x); ep[threadIdx.x] = vm_edge(fp, lp, threadIdx.x); }
  __syncthreads();
  const float scale_t = (float)VM_BINS / (lt - ft), scale_p = (float)VM_BINS / (lp - fp);
  int64_t b0, b1;
  vm_chunk(S, b, nb, b0, b1);
  unsigned outside = 0u;
  vm_for_chunk<MASKED>(t + (size_t)n * S, p + (size_t)n * S, MASKED ? bits + (size_t)n * S : nullptr, b0, b1, vec,
                       [&](float a, float c, unsigned w) {
    if (MASKED && !((w >> label) & 1u)) { ++outside; return; }
    const int i = vm_bin(a, et, ft, scale_t), j = vm_bin(c, ep, fp, scale_p);
    atomicAdd(&h[i], 1u);
    atomicAdd(&h[VM_BINS + j], 1u);
    atomicAdd(&h[2 * VM_BINS + i * VM_BINS + j], 1u);
  });
  if (outside) {          // tm = pm = 0 there (0 lies inside both ranges, since a masked-out element took part in them)
    const int i = vm_bin(0.f, et, ft, scale_t), j = vm_bin(0.f, ep, fp, scale_p);
    atomicAdd(&h[i], outside);
    atomicAdd(&h[VM_BINS + j], outside);
    atomicAdd(&h[2 * VM_BINS + i * VM_BINS + j], outside);
  }
  __syncthreads();
  unsigned* out = counts + ((size_t)n * L + label) * VM_HIST_WORDS;
  for (int i = threadIdx.x; i < VM_HIST_WORDS; i += VM_THREADS)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

// ---- pass 4: finalize -----------------------------------------------------------------------------------------------
__device__ double vm_entr(double x) { return x > 0.0 ? -x * log(x) : 0.0; }

// nmi and histogram_chi2 of one count table c ([t bins][p bins][joint]) of S elements whose histogram ranges are
// rg = {min t, max t, min p, max p} (every thread gets both values)
struct VmHistShared {
  double rowsum[VM_BINS], colsum[VM_BINS];
  float wt[VM_BINS], wp[VM_BINS];
};
__device__ __forceinline__ void vm_hist_scores(const unsigned* c, int64_t S, const float* rg, VmHistShared& hs,
                                               double* sh, double& nmi, double& chi2) {
  double* rowsum = hs.rowsum; double* colsum = hs.colsum;
  float* wt = hs.wt; float* wp = hs.wp;
  // histogram_chi2: each histogram normalised to sum 1 (the sum is S), 0/0 bins dropped
  double chi = 0.0;
  if (threadIdx.x < VM_BINS) {
    const double g = (double)c[threadIdx.x] / (double)S, q = (double)c[VM_BINS + threadIdx.x] / (double)S;
    if (g + q != 0.0) chi = (q - g) * (q - g) / (q + g);
  }
  chi2 = vm_block_sum(chi, sh);
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
  nmi = (H0 + H1) / H01;
}

template <bool MASKED>
__global__ __launch_bounds__(VM_THREADS) void vm_final_kernel(int64_t S, int labels, int P, int H, int W, int nb_mom,
                                                              const double* mom, int ssim_blocks, const double* ssim_part,
                                                              const unsigned* counts, double* table) {
  using Path = VmPath<MASKED>;
  __shared__ double sh[VM_THREADS];
  __shared__ VmHistShared hs;
  const int L = MASKED ? labels : 1;
  const int n = blockIdx.x / L, label = blockIdx.x % L;
  const size_t out = MASKED ? (size_t)blockIdx.x : (size_t)n;       // n * L + label: the row of table, counts and partials
  const double* m = Path::sample(mom, n, nb_mom, L);
  double s[Path::SUMS] = {};
  for (int b = threadIdx.x; b < nb_mom; b += VM_THREADS)
    for (int k = 0; k < Path::SUMS; ++k) s[k] += Path::row(m, b, L, label)[k];
  // each path's own reduction, as in Path::range: one pass of butterflies over all columns, or a halving tree per column
  if constexpr (MASKED) vmm_block_reduce<Path::SUMS>(s, 0u, 0u, sh);
  const double sad = MASKED ? s[0] : vm_block_sum(s[0], sh), ssd = MASKED ? s[1] : vm_block_sum(s[1], sh),
               stt = MASKED ? s[2] : vm_block_sum(s[2], sh);
  float rg[5];
  Path::range(m, nb_mom, L, label, rg, sh);
  const double nan = __builtin_nan("");
  double row[7] = {nan, nan, nan, nan, nan, nan, nan};
  // mae and mse average over the elements inside the mask (n: a sum of integers below 2^32, exact), or over all S. The
  // order of the two divisions per path is on purpose: DESIGN.md 4.11
  const double cnt = MASKED ? s[Path::SUMS - 1] : (double)S;
  if constexpr (MASKED) { row[0] = sad / cnt; row[1] = ssd / cnt; } else { row[1] = ssd / cnt; row[0] = sad / cnt; }
  row[2] = ssd / stt;
  const double R = (double)rg[0];
  row[3] = 10.0 * log10((R * R) / (ssd / (double)S));                // skimage averages over all S elements, masked or not
  if (ssim_part) {
    const double* sp = ssim_part + out * ssim_blocks;
    double a = 0.0;
    for (int b = threadIdx.x; b < ssim_blocks; b += VM_THREADS) a += sp[b];
    a = vm_block_sum(a, sh);
    row[4] = a / ((double)P * (double)(H - 6) * (double)(W - 6));
  }
  if (counts) vm_hist_scores(counts + out * VM_HIST_WORDS, S, rg + 1, hs, sh, row[5], row[6]);
  if (threadIdx.x < 7) table[out * 7 + threadIdx.x] = !MASKED || cnt > 0.0 ? row[threadIdx.x] : nan;   // empty mask
}

// ---- host -----------------------------------------------------------------------------------------------------------
// scratch: [moment slab][ssim partials], then for the masked call [packed mask bits, one byte per element]. The plain
// call is L = 1 with its own slab row and no bits.
struct VmPlan {
  int64_t S;
  int nb_mom, nb_hist, tiles_w, tiles_h;
  size_t mom_doubles, ssim_doubles, bit_bytes;
};
VmPlan vm_plan(bool masked, int32_t N, int32_t L, int32_t P, int32_t H, int32_t W) {
  VmPlan q;
  q.S = (int64_t)P * H * W;
  q.nb_mom = vm_moment_blocks(q.S);
  q.nb_hist = vm_hist_blocks(q.S);
  q.tiles_w = W > 6 ? (W - 6 + VM_TW - 1) / VM_TW : 0;
  q.tiles_h = H > 6 ? (H - 6 + VM_TH - 1) / VM_TH : 0;
  q.mom_doubles = (size_t)N * q.nb_mom * L * (masked ? VMM_MOM : VM_MOM);
  q.ssim_doubles = (size_t)N * P * q.tiles_w * q.tiles_h * L;
  q.bit_bytes = masked ? ((size_t)N * q.S + 15) / 16 * 16 : 0;
  return q;
}
int64_t vm_scratch_bytes(const VmPlan& q) {
  return (int64_t)((q.mom_doubles + q.ssim_doubles) * sizeof(double) + q.bit_bytes);
}

// both entry points; `name` is the entry point's, for its refusals. !MASKED: masks is null and L is 1.
template <bool MASKED>
int vm_run(const char* name, const float* t, const float* p, const uint8_t* const* masks, int32_t L, int32_t N,
           int32_t P, int32_t H, int32_t W, int32_t flags, double* table, uint32_t* counts, void* scratch,
           void* stream) {
  GS_REQUIRE(t && p && (masks || !MASKED) && table && scratch && N > 0 && P > 0 && H > 0 && W > 0 &&
             (flags & ~(GS_VM_SSIM | GS_VM_HIST)) == 0, "%s: bad argument", name);
  GS_REQUIRE(L >= 1 && L <= VM_MAX_LABELS, "%s: between 1 and GS_VM_MAX_LABELS masks per call", name);
  GS_REQUIRE(!(flags & GS_VM_SSIM) || (H >= 7 && W >= 7), "%s: SSIM needs H >= 7 and W >= 7 (7x7 window)", name);
  GS_REQUIRE(!(flags & GS_VM_HIST) || counts, "%s: histograms need the counts table", name);
  const VmPlan q = vm_plan(MASKED, N, L, P, H, W);
  GS_REQUIRE(q.S < ((int64_t)1 << 32), "%s: a sample must hold fewer than 2^32 elements (uint32 counts)", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* mom = static_cast<double*>(scratch);
  double* ssim_part = mom + q.mom_doubles;
  uint8_t* bits = MASKED ? reinterpret_cast<uint8_t*>(ssim_part + q.ssim_doubles) : nullptr;
  unsigned* cnt = (flags & GS_VM_HIST) ? counts : nullptr;
  // float4 loads need 16-byte aligned t and p and S % 4 == 0. The bits of sample n start at n * S, so their word loads
  // need S % 4 == 0 too (their base is 8-byte aligned)
  const bool vec = ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(p)) & 15) == 0 && q.S % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(bits) & 3) == 0;
  if constexpr (MASKED) {
    VmMaskPtrs mk = {};
    bool words = true;
    for (int l = 0; l < L; ++l) {
      GS_REQUIRE(masks[l], "%s: null mask", name);
      mk.m[l] = masks[l];
      words = words && (reinterpret_cast<uintptr_t>(masks[l]) & 3) == 0;
    }
    const int64_t total = (int64_t)N * q.S;
    const int64_t nwords = words ? total / 4 : 0;
    const int64_t pack_items = nwords > 0 ? nwords : total;
    const int pack_blocks = (int)((pack_items + 4 * VM_THREADS - 1) / (4 * VM_THREADS) < 2048
                                      ? (pack_items + 4 * VM_THREADS - 1) / (4 * VM_THREADS) : 2048);
    hipLaunchKernelGGL(vmm_pack_kernel, dim3(pack_blocks), dim3(VM_THREADS), 0, st, mk, L, nwords, total, bits);
    hipLaunchKernelGGL(vmm_moments_kernel, dim3(N * q.nb_mom), dim3(VM_THREADS), 0, st, t, p, bits, L, q.S, q.nb_mom,
                       vec, mom, cnt);
  } else {
    hipLaunchKernelGGL(vm_moments_kernel, dim3(N * q.nb_mom), dim3(VM_THREADS), 0, st, t, p, q.S, q.nb_mom, vec, mom,
                       cnt);
  }
  const int ssim_blocks = P * q.tiles_w * q.tiles_h;
  if (flags & GS_VM_SSIM)
    hipLaunchKernelGGL(vm_ssim_kernel<MASKED>, dim3(N * ssim_blocks * L), dim3(VM_THREADS), 0, st, t, p, bits, L, P, H,
                       W, q.tiles_w, q.tiles_h, q.nb_mom, mom, ssim_part);
  if (flags & GS_VM_HIST)
    hipLaunchKernelGGL(vm_hist_kernel<MASKED>, dim3(N * q.nb_hist * L), dim3(VM_THREADS), 0, st, t, p, bits, L, q.S,
                       q.nb_hist, vec, q.nb_mom, mom, cnt);
  hipLaunchKernelGGL(vm_final_kernel<MASKED>, dim3(N * L), dim3(VM_THREADS), 0, st, q.S, L, P, H, W, q.nb_mom, mom,
                     ssim_blocks, (flags & GS_VM_SSIM) ? ssim_part : nullptr, cnt, table);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int64_t gs_valmetric_scratch_bytes(int32_t N, int32_t P, int32_t H, int32_t W) {
  if (N <= 0 || P <= 0 || H <= 0 || W <= 0) return 0;
  return vm_scratch_bytes(vm_plan(false, N, 1, P, H, W));
}

extern "C" int64_t gs_valmetric_masked_scratch_bytes(int32_t N, int32_t L, int32_t P, int32_t H, int32_t W) {
  if (N <= 0 || L <= 0 || L > VM_MAX_LABELS || P <= 0 || H <= 0 || W <= 0) return 0;
  return vm_scratch_bytes(vm_plan(true, N, L, P, H, W));
}

extern "C" int gs_valmetrics(const float* t, const float* p, int32_t N, int32_t P, int32_t H, int32_t W, int32_t flags,
                             double* table, uint32_t* counts, void* scratch, void* stream) {
  return vm_run<false>("gs_valmetrics", t, p, nullptr, 1, N, P, H, W, flags, table, counts, scratch, stream);
}

extern "C" int gs_valmetrics_masked(const float* t, const float* p, const uint8_t* const* masks, int32_t L, int32_t N,
                                    int32_t P, int32_t H, int32_t W, int32_t flags, double* table, uint32_t* counts,
                                    void* scratch, void* stream) {
  return vm_run<true>("gs_valmetrics_masked", t, p, masks, L, N, P, H, W, flags, table, counts, scratch, stream);
}
