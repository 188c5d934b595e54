// Sliding-window (patch-wise) inference around a predictor: gather the windows of a chunk, blend the predictions into an
// accumulator, normalise (ganslate_amd/utils/sliding_window_inferer.py steps 1, 4, 5; monai/inferers/utils.py).
// All tensors are dense fp32 NCDHW; an image is the D == 1 case. The window table is a device int32 [n][4] of
// (batch item, z, y, x) with the starts in PADDED coordinates: the volume padded symmetrically to max(size, roi) per axis.
//   gather     : out[i, c] = window i of the padded input; the padding reads cval and is never materialised
//   accumulate : acc[b, c, window_i] += imap * pred[i, c] for the rows of one chunk, in table order. Output-stationary: one
//                thread owns an accumulator element (four along x on the vector path) and walks the rows in order, so
//                overlapping windows need no atomics and the sum has the host loop's order. One rounded multiply and one
//                rounded add per covering row. Launched over the largest per-sample bounding box of the chunk's windows.
//   finalize   : result[b, c, v] = acc[b, c, v + pad_before] / count(v + pad_before) at the original size. count is no
//                buffer: a thread sums imap over the rows of the whole call that cover its voxel, in table order — the
//                bits of the host's `count[s] += imap` from zero — once for all channels.
// Streaming kernels: every element of the input window, the prediction, the accumulator box and the result moves once.
// Rows are wave-uniform (scalar loads); a row of another sample or another depth range is skipped by a uniform branch.
// Nothing the table holds can make a kernel write out of bounds: gather and finalize write only the element their
// thread index names, accumulate clamps the box it derives from the rows to the accumulator.
#include "common.hpp"

#include <limits.h>

#define SW_THREADS 256

namespace {

struct SwGeom {
  int B, C;
  int D, H, W;        // gather: the input; accumulate: the (padded) accumulator; finalize: the result
  int Dp, Hp, Wp;     // padded size, max(size, roi) per axis (the accumulator's)
  int rd, rh, rw;     // window
  int pz, py, px;     // padding in front of each axis
};

// s + m * p as the host computes it: the product rounded, then the sum rounded. hipcc contracts a * b + c to an fma by
// default, through __fmul_rn / __fadd_rn too (they are plain operators); the pragma switches that off for this body, and
// the instructions keep their flags when it is inlined.
__device__ __forceinline__ float sw_mul_add(float s, float m, float p) {
#pragma clang fp contract(off)
  const float t = m * p;
  return s + t;
}

template <bool VEC>
__global__ __launch_bounds__(SW_THREADS) void sw_gather_kernel(const float* __restrict__ in, SwGeom g,
                                                               const int4* __restrict__ table, float cval,
                                                               float* __restrict__ out) {
  constexpr int V = VEC ? 4 : 1;
  const int rwq = g.rw / V;
  const int idx = blockIdx.x * SW_THREADS + threadIdx.x;
  if (idx >= g.rh * rwq) return;
  const int ly = idx / rwq, lx = (idx - ly * rwq) * V, lz = blockIdx.y;
  const int i = blockIdx.z / g.C, c = blockIdx.z - i * g.C;
  const int4 row = table[i];
  const int z = row.y + lz - g.pz, y = row.z + ly - g.py, x = row.w + lx - g.px;       // in the unpadded input
  const bool line = (unsigned)row.x < (unsigned)g.B && (unsigned)z < (unsigned)g.D && (unsigned)y < (unsigned)g.H;
  const int64_t src = (((int64_t)row.x * g.C + c) * g.D + z) * ((int64_t)g.H * g.W) + (int64_t)y * g.W;
  float* dst = out + (((int64_t)blockIdx.z * g.rd + lz) * g.rh + ly) * (int64_t)g.rw + lx;
  if constexpr (VEC) {
    float4 v = {cval, cval, cval, cval};
    if (line) {
      const float* p = in + src + x;
      if (x >= 0 && x + 3 < g.W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        if ((unsigned)x < (unsigned)g.W) v.x = p[0];
        if ((unsigned)(x + 1) < (unsigned)g.W) v.y = p[1];
        if ((unsigned)(x + 2) < (unsigned)g.W) v.z = p[2];
        if ((unsigned)(x + 3) < (unsigned)g.W) v.w = p[3];
      }
    }
    *reinterpret_cast<float4*>(dst) = v;
  } else {
    *dst = (line && (unsigned)x < (unsigned)g.W) ? in[src + x] : cval;
  }
}

// g.D/H/W == g.Dp/Hp/Wp: the accumulator. bh x bwq (bwq in units of V elements): the host's bound on a sample's box.
template <bool VEC>
__global__ __launch_bounds__(SW_THREADS) void sw_accumulate_kernel(float* __restrict__ acc, SwGeom g,
                                                                   const int4* __restrict__ table, int n,
                                                                   const float* __restrict__ imap,
                                                                   const float* __restrict__ pred, int bh, int bwq) {
  constexpr int V = VEC ? 4 : 1;
  const int b = blockIdx.z / g.C, c = blockIdx.z - b * g.C;
  int z0 = INT_MAX, y0 = INT_MAX, x0 = INT_MAX, z1 = INT_MIN, y1 = INT_MIN, x1 = INT_MIN;
  for (int i = 0; i < n; ++i) {
    const int4 r = table[i];
    if (r.x != b) continue;
    z0 = min(z0, r.y); y0 = min(y0, r.z); x0 = min(x0, r.w);
    z1 = max(z1, r.y); y1 = max(y1, r.z); x1 = max(x1, r.w);
  }
  if (z1 == INT_MIN) return;                 // no window of this sample in the chunk
  z0 = max(z0, 0); y0 = max(y0, 0); x0 = max(x0, 0) & ~(V - 1);
  z1 = min(z1, g.Dp - g.rd) + g.rd; y1 = min(y1, g.Hp - g.rh) + g.rh; x1 = min(x1, g.Wp - g.rw) + g.rw;
  const int idx = blockIdx.x * SW_THREADS + threadIdx.x;
  const int ly = idx / bwq;
  const int z = z0 + blockIdx.y, y = y0 + ly, x = x0 + (idx - ly * bwq) * V;
  if (ly >= bh || z >= z1 || y >= y1 || x + V > x1) return;
  float* a = acc + ((((int64_t)b * g.C + c) * g.Dp + z) * g.Hp + y) * (int64_t)g.Wp + x;
  const int64_t win = (int64_t)g.rd * g.rh * g.rw;
  if constexpr (VEC) {
    float4 s = *reinterpret_cast<const float4*>(a);
    for (int i = 0; i < n; ++i) {
      const int4 r = table[i];
      const int lz = z - r.y;
      if (r.x != b || (unsigned)lz >= (unsigned)g.rd) continue;
      const int wy = y - r.z, wx = x - r.w;
      if ((unsigned)wy < (unsigned)g.rh && wx >= 0 && wx + 4 <= g.rw) {
        const int64_t o = ((int64_t)lz * g.rh + wy) * g.rw + wx;
        const float4 m = *reinterpret_cast<const float4*>(imap + o);
        const float4 p = *reinterpret_cast<const float4*>(pred + ((int64_t)i * g.C + c) * win + o);
        s.x = sw_mul_add(s.x, m.x, p.x); s.y = sw_mul_add(s.y, m.y, p.y);
        s.z = sw_mul_add(s.z, m.z, p.z); s.w = sw_mul_add(s.w, m.w, p.w);
      }
    }
    *reinterpret_cast<float4*>(a) = s;
  } else {
    float s = *a;
    for (int i = 0; i < n; ++i) {
      const int4 r = table[i];
      const int lz = z - r.y;
      if (r.x != b || (unsigned)lz >= (unsigned)g.rd) continue;
      const int wy = y - r.z, wx = x - r.w;
      if ((unsigned)wy < (unsigned)g.rh && (unsigned)wx < (unsigned)g.rw) {
        const int64_t o = ((int64_t)lz * g.rh + wy) * g.rw + wx;
        s = sw_mul_add(s, imap[o], pred[((int64_t)i * g.C + c) * win + o]);
      }
    }
    *a = s;
  }
}

template <bool VEC>
__global__ __launch_bounds__(SW_THREADS) void sw_finalize_kernel(const float* __restrict__ acc, SwGeom g,
                                                                 const int4* __restrict__ table, int n,
                                                                 const float* __restrict__ imap,
                                                                 float* __restrict__ result) {
  constexpr int V = VEC ? 4 : 1;
  const int wq = g.W / V;
  const int idx = blockIdx.x * SW_THREADS + threadIdx.x;
  if (idx >= g.H * wq) return;
  const int y = idx / wq, x = (idx - y * wq) * V, z = blockIdx.y, b = blockIdx.z;
  const int qz = z + g.pz, qy = y + g.py, qx = x + g.px;                               // in the accumulator
  float cnt[V];
#pragma unroll
  for (int k = 0; k < V; ++k) cnt[k] = 0.f;
  for (int i = 0; i < n; ++i) {
    const int4 r = table[i];
    const int lz = qz - r.y;
    if (r.x != b || (unsigned)lz >= (unsigned)g.rd) continue;
    const int wy = qy - r.z;
    if ((unsigned)wy >= (unsigned)g.rh) continue;
    const float* m = imap + ((int64_t)lz * g.rh + wy) * g.rw;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int wx = qx + k - r.w;
      if ((unsigned)wx < (unsigned)g.rw) cnt[k] = __fadd_rn(cnt[k], m[wx]);
    }
  }
  const int64_t a_cs = (int64_t)g.Dp * g.Hp * g.Wp, r_cs = (int64_t)g.D * g.H * g.W;
  const float* a = acc + (int64_t)b * g.C * a_cs + ((int64_t)qz * g.Hp + qy) * g.Wp + qx;
  float* o = result + (int64_t)b * g.C * r_cs + ((int64_t)z * g.H + y) * g.W + x;
  for (int c = 0; c < g.C; ++c, a += a_cs, o += r_cs) {
    if constexpr (VEC) {
      const float4 s = *reinterpret_cast<const float4*>(a);
      float4 q;
      q.x = __fdiv_rn(s.x, cnt[0]); q.y = __fdiv_rn(s.y, cnt[1]);
      q.z = __fdiv_rn(s.z, cnt[2]); q.w = __fdiv_rn(s.w, cnt[3]);
      *reinterpret_cast<float4*>(o) = q;
    } else {
      *o = __fdiv_rn(*a, cnt[0]);
    }
  }
}

bool sw_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// the checks the three entry points share; fills the geometry (padded size = max(size, roi))
static int sw_geometry(const char* who, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, int32_t n,
                       const int32_t* roi, const int32_t* pad_before, SwGeom& g) {
  GS_REQUIRE(B >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: B, C, D, H, W must be >= 1", who);
  GS_REQUIRE(n >= 1, "%s: n must be >= 1", who);
  GS_REQUIRE(roi && roi[0] >= 1 && roi[1] >= 1 && roi[2] >= 1, "%s: roi[k] must be >= 1", who);
  g.B = B; g.C = C; g.D = D; g.H = H; g.W = W;
  g.rd = roi[0]; g.rh = roi[1]; g.rw = roi[2];
  g.Dp = D > g.rd ? D : g.rd; g.Hp = H > g.rh ? H : g.rh; g.Wp = W > g.rw ? W : g.rw;
  g.pz = pad_before ? pad_before[0] : 0; g.py = pad_before ? pad_before[1] : 0; g.px = pad_before ? pad_before[2] : 0;
  GS_REQUIRE(g.pz >= 0 && g.pz <= g.Dp - D && g.py >= 0 && g.py <= g.Hp - H && g.px >= 0 && g.px <= g.Wp - W,
             "%s: pad_before[k] must lie in [0, max(size, roi) - size]", who);
  GS_REQUIRE((int64_t)C * g.Dp * g.Hp * g.Wp < ((int64_t)1 << 31),
             "%s: a padded sample must hold fewer than 2^31 elements", who);
  GS_REQUIRE((int64_t)C * g.rd * g.rh * g.rw < ((int64_t)1 << 31), "%s: a window must hold fewer than 2^31 elements", who);
  return 0;
}

#define SW_GEOMETRY(...)                  \
  do {                                    \
    const int rc_ = sw_geometry(__VA_ARGS__); \
    if (rc_) return rc_;                  \
  } while (0)

extern "C" int gs_sw_gather(const float* in, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, const int32_t* table,
                            int32_t n, const int32_t* roi, const int32_t* pad_before, float cval, float* out,
                            void* stream) {
  GS_REQUIRE(in && table && out && pad_before, "gs_sw_gather: null argument");
  GS_REQUIRE(sw_aligned16(table), "gs_sw_gather: the table must be 16-byte aligned");
  SwGeom g;
  SW_GEOMETRY("gs_sw_gather", B, C, D, H, W, n, roi, pad_before, g);
  GS_REQUIRE(g.rd <= 65535 && (int64_t)n * C <= 65535, "gs_sw_gather: roi[0] and n * C must be <= 65535 (grid)");
  const bool vec = g.rw % 4 == 0 && sw_aligned16(out);
  const int per = g.rh * (g.rw / (vec ? 4 : 1));
  const dim3 grid((per + SW_THREADS - 1) / SW_THREADS, g.rd, n * C);
  const int4* rows = reinterpret_cast<const int4*>(table);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(sw_gather_kernel<true>, grid, dim3(SW_THREADS), 0, st, in, g, rows, cval, out);
  else hipLaunchKernelGGL(sw_gather_kernel<false>, grid, dim3(SW_THREADS), 0, st, in, g, rows, cval, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_sw_accumulate(float* acc, int32_t B, int32_t C, int32_t Dp, int32_t Hp, int32_t Wp,
                                const int32_t* table, const int32_t* table_host, int32_t n, const int32_t* roi,
                                const float* imap, const float* pred, void* stream) {
  GS_REQUIRE(acc && table && table_host && imap && pred, "gs_sw_accumulate: null argument");
  GS_REQUIRE(sw_aligned16(table), "gs_sw_accumulate: the table must be 16-byte aligned");
  SwGeom g;
  SW_GEOMETRY("gs_sw_accumulate", B, C, Dp, Hp, Wp, n, roi, nullptr, g);
  GS_REQUIRE(g.rd <= Dp && g.rh <= Hp && g.rw <= Wp, "gs_sw_accumulate: the accumulator is smaller than the window");
  GS_REQUIRE((int64_t)B * C <= 65535 && Dp <= 65535, "gs_sw_accumulate: B * C and the depth must be <= 65535 (grid)");
  // the largest per-sample bounding box of the chunk's windows sizes the grid; the kernel derives each sample's own box
  // from the device rows
  int bd = 0, bh = 0, bw = 0;
  bool x4 = true;
  for (int b = 0; b < B; ++b) {
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (int i = 0; i < n; ++i) {
      const int32_t* r = table_host + 4 * i;
      GS_REQUIRE(r[0] >= 0 && r[0] < B && r[1] >= 0 && r[1] <= Dp - g.rd && r[2] >= 0 && r[2] <= Hp - g.rh && r[3] >= 0 &&
                 r[3] <= Wp - g.rw, "gs_sw_accumulate: table row %d lies outside the accumulator", i);
      if (r[0] != b) continue;
      for (int k = 0; k < 3; ++k) { lo[k] = r[1 + k] < lo[k] ? r[1 + k] : lo[k]; hi[k] = r[1 + k] > hi[k] ? r[1 + k] : hi[k]; }
      x4 = x4 && r[3] % 4 == 0;
    }
    if (hi[0] == INT_MIN) continue;
    bd = hi[0] - lo[0] + g.rd > bd ? hi[0] - lo[0] + g.rd : bd;
    bh = hi[1] - lo[1] + g.rh > bh ? hi[1] - lo[1] + g.rh : bh;
    bw = hi[2] - lo[2] + g.rw > bw ? hi[2] - lo[2] + g.rw : bw;
  }
  const bool vec = x4 && g.rw % 4 == 0 && Wp % 4 == 0 && sw_aligned16(acc) && sw_aligned16(imap) && sw_aligned16(pred) &&
                   ((int64_t)g.rd * g.rh * g.rw) % 4 == 0;
  const int bwq = vec ? bw / 4 : bw;
  const dim3 grid((bh * bwq + SW_THREADS - 1) / SW_THREADS, bd, B * C);
  const int4* rows = reinterpret_cast<const int4*>(table);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(sw_accumulate_kernel<true>, grid, dim3(SW_THREADS), 0, st, acc, g, rows, n, imap, pred, bh, bwq);
  else hipLaunchKernelGGL(sw_accumulate_kernel<false>, grid, dim3(SW_THREADS), 0, st, acc, g, rows, n, imap, pred, bh, bwq);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_sw_finalize(const float* acc, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W,
                              const int32_t* table, int32_t n, const int32_t* roi, const int32_t* pad_before,
                              const float* imap, float* result, void* stream) {
  GS_REQUIRE(acc && table && imap && result && pad_before, "gs_sw_finalize: null argument");
  GS_REQUIRE(sw_aligned16(table), "gs_sw_finalize: the table must be 16-byte aligned");
  SwGeom g;
  SW_GEOMETRY("gs_sw_finalize", B, C, D, H, W, n, roi, pad_before, g);
  GS_REQUIRE(B <= 65535 && D <= 65535, "gs_sw_finalize: B and the depth must be <= 65535 (grid)");
  const bool vec = W % 4 == 0 && g.Wp % 4 == 0 && g.px % 4 == 0 && sw_aligned16(acc) && sw_aligned16(result) &&
                   ((int64_t)g.Dp * g.Hp * g.Wp) % 4 == 0 && ((int64_t)D * H * W) % 4 == 0;
  const int per = H * (W / (vec ? 4 : 1));
  const dim3 grid((per + SW_THREADS - 1) / SW_THREADS, D, B);
  const int4* rows = reinterpret_cast<const int4*>(table);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(sw_finalize_kernel<true>, grid, dim3(SW_THREADS), 0, st, acc, g, rows, n, imap, result);
  else hipLaunchKernelGGL(sw_finalize_kernel<false>, grid, dim3(SW_THREADS), 0, st, acc, g, rows, n, imap, result);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
