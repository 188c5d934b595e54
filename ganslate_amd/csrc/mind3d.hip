// MIND structure-consistency loss (Yang et al. 2018) for volumes: the scheme of mind.hip moved to three dimensions, fused
// from the volumes to the scalar and from the scalar back to the volume gradient. The reference has no volumetric MIND; the
// definition is this project's own (include/ganslate_hip.h).
//
// Per volume I (the mean over the channels of a [C, D, H, W] sample, zero outside): for the 27 shifts a of the 3x3x3 region
//   d_a(r) = I(r + a) - I(r)                         (r inside; I(r + a) = 0 outside)
//   D_a(p) = sum_{q in 5^3, p+q inside} g(q) d_a(p+q)^2,   g(q) = exp(-|q|_2 / sigma^2)   (distance, not its square)
//   B_b(p) = sum_{q in 5^3, p+q inside} I(p+q+b) for the 27 shifts b of the 3^3 neighbourhood, V = var_b(B_b) (divisor 26)
//   n_a = exp(-D_a / (V + 1e-8)),  f_a = n_a / sum_c n_c;
//   output channel i has depth offset i % 3 - 1, row offset (i / 3) % 3 - 1, column offset i / 9 - 1.
//
// One workgroup = one 4 x 8 x 8 box (depth x rows x columns) of one sample, one voxel per thread, one depth slice per wave.
// The box with its halo of 3 (1 for the shift + 2 for the patch) sits in LDS (10 x 14 x 14 floats); per shift the 8 x 12 x 12
// box of masked d_a^2 is written to one of two LDS buffers (filled for shift a + 1 while shift a is summed: one barrier per
// shift) and every thread takes its 125 taps from it. The 27 numerators of a voxel stay in registers (the shift loop is
// unrolled, so every index is a constant) until their sum is known: no 27-channel volume leaves the workgroup in the
// forward. The 27 neighbourhood sums are box sums over a clipped box, a product of three clipped intervals: they are built
// separably (columns, then rows, then depth), 343 LDS reads per voxel instead of 3375. No atomics anywhere: the loss is one
// partial per workgroup summed in index order by a second launch, the backward is a gather.
#include "mind_common.hpp"

#define M3_BZ 4                      // box: depth
#define M3_BY 8                      // ... rows
#define M3_BX 8                      // ... columns
#define M3_IY 14                     // volume box with halo 3: M3_BY + 6 rows of M3_BX + 6 columns (dense) ...
#define M3_IPS (M3_IY * M3_IY)       // ... its plane stride ...
#define M3_IN ((M3_BZ + 6) * M3_IPS) // ... and its size, 10 planes: 1960 floats
#define M3_DZ 8                      // squared-difference box with halo 2: M3_BZ + 4 planes
#define M3_DY 12                     // ... of M3_BY + 4 rows of M3_BX + 4 columns
#define M3_DRS 24                    // ... row stride: the four rows of a half wave read disjoint banks (0, 24, 16, 8 mod 32)
#define M3_DPS (M3_DY * M3_DRS)      // ... plane stride
#define M3_DN (M3_DZ * M3_DPS)       // ... size of one buffer: 2304 floats
#define M3_EZ 6                      // backward: box of E_a with a ring of 1, M3_BZ + 2 planes
#define M3_EY 10                     // ... of M3_BY + 2 rows of M3_BX + 2 columns
#define M3_NS 27

struct Mind3W { float g[13]; };      // the patch weight by SQUARED distance (0 .. 12), a kernel argument (scalar registers)

__device__ __forceinline__ bool mind3_in(int z, int y, int x, int D, int H, int W) {
  return (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}
__host__ __device__ constexpr int mind3_az(int a) { return a % 3 - 1; }            // depth offset of shift a
__host__ __device__ constexpr int mind3_ay(int a) { return (a / 3) % 3 - 1; }      // row offset
__host__ __device__ constexpr int mind3_ax(int a) { return a / 9 - 1; }            // column offset
__host__ __device__ constexpr int mind3_aoff(int a) { return mind3_az(a) * M3_IPS + mind3_ay(a) * M3_IY + mind3_ax(a); }
__host__ __device__ constexpr int mind3_r2(int tz, int ty, int tx) {
  return (tz - 2) * (tz - 2) + (ty - 2) * (ty - 2) + (tx - 2) * (tx - 2);
}

struct Mind3Pos { int pz, py, px; };
__device__ __forceinline__ Mind3Pos mind3_pos() {
  Mind3Pos p;
  p.px = threadIdx.x & 7;
  p.py = (threadIdx.x >> 3) & 7;
  p.pz = threadIdx.x >> 6;
  return p;
}

// 10 x 14 x 14 box of the channel mean of one sample with origin (z0 - 3, y0 - 3, x0 - 3), zero outside the volume
__device__ __forceinline__ void mind3_load_box(const float* img, int C, int D, int H, int W, int z0, int y0, int x0,
                                               float* sI) {
  const size_t HW = (size_t)H * W, DHW = HW * D;
  for (int e = threadIdx.x; e < M3_IN; e += 256) {
    const int rz = e / M3_IPS, rem = e - rz * M3_IPS, ry = rem / M3_IY, rx = rem - ry * M3_IY;
    const int iz = z0 - 3 + rz, iy = y0 - 3 + ry, ix = x0 - 3 + rx;
    float v = 0.f;
    if (mind3_in(iz, iy, ix, D, H, W)) {
      const float* p = img + (size_t)iz * HW + (size_t)iy * W + ix;
      float s = p[0];
      for (int ch = 1; ch < C; ++ch) s += p[(size_t)ch * DHW];
      v = C > 1 ? s / (float)C : s;
    }
    sI[e] = v;
  }
}

// the 27 patch sums of the 3^3 neighbourhood and their unbiased variance at voxel g = box position p. The clipped patch is
// a product of intervals, so per plane of the box: three column sums per row, folded over the rows into nine sums, folded
// over the planes into the 27.
struct Mind3V { float B[M3_NS]; float mean; float veps; };
__device__ __forceinline__ Mind3V mind3_variance(const float* sI, const Mind3Pos& p, int gz, int gy, int gx, int D, int H,
                                                 int W) {
  Mind3V v;
  bool my[5], mx[5];                 // is tap k - 2 of the patch inside the volume, per axis
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    my[k] = (unsigned)(gy + k - 2) < (unsigned)H;
    mx[k] = (unsigned)(gx + k - 2) < (unsigned)W;
  }
#pragma unroll
  for (int k = 0; k < M3_NS; ++k) v.B[k] = 0.f;
#pragma unroll 1
  for (int lz = 0; lz < 7; ++lz) {                       // plane gz + lz - 3 (a loop: unrolled, its 343 reads fill the registers)
    float P[9];                                          // [by * 3 + bx]: this plane's sums over the clipped rows and columns
#pragma unroll
    for (int k = 0; k < 9; ++k) P[k] = 0.f;
#pragma unroll
    for (int ly = 0; ly < 7; ++ly) {                     // row gy + ly - 3
      const float* r = sI + (p.pz + lz) * M3_IPS + (p.py + ly) * M3_IY + p.px;
      float c[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) c[j] = r[j];           // columns gx - 3 .. gx + 3
#pragma unroll
      for (int bx = 0; bx < 3; ++bx) {
        float sx = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) sx += mx[k] ? c[k + bx] : 0.f;      // tap k - 2, shift bx - 1
#pragma unroll
        for (int by = 0; by < 3; ++by) {
          const int k = ly - by;                         // this row is tap k - 2 of shift by - 1
          if (k >= 0 && k < 5) P[by * 3 + bx] += my[k] ? sx : 0.f;
        }
      }
    }
#pragma unroll
    for (int bz = 0; bz < 3; ++bz) {
      const int qz = lz - bz - 2;                        // this plane is tap qz of shift bz - 1
      const bool on = qz >= -2 && qz <= 2 && (unsigned)(gz + qz) < (unsigned)D;
#pragma unroll
      for (int j = 0; j < 9; ++j) v.B[bz + 3 * (j / 3) + 9 * (j % 3)] += on ? P[j] : 0.f;
    }
  }
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < M3_NS; ++k) m += v.B[k];
  m /= 27.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < M3_NS; ++k) { const float d = v.B[k] - m; s += d * d; }
  v.mean = m;
  v.veps = s / 26.f + MIND_EPS;
  return v;
}

// the (up to) five entries of the 8 x 12 x 12 box of masked d_a^2 that a thread fills for every shift
struct Mind3Fill {
  int ci[5], di[5];
  bool in[5];
  __device__ __forceinline__ Mind3Fill(int z0, int y0, int x0, int D, int H, int W) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int e = threadIdx.x + 256 * k;
      const bool ok = e < M3_DZ * M3_DY * M3_DY;
      const int rz = ok ? e / (M3_DY * M3_DY) : 0, rem = ok ? e - rz * (M3_DY * M3_DY) : 0;
      const int ry = rem / M3_DY, rx = rem - ry * M3_DY;
      in[k] = ok && mind3_in(z0 - 2 + rz, y0 - 2 + ry, x0 - 2 + rx, D, H, W);
      ci[k] = (rz + 1) * M3_IPS + (ry + 1) * M3_IY + rx + 1;
      di[k] = ok ? rz * M3_DPS + ry * M3_DRS + rx : -1;
    }
  }
  __device__ __forceinline__ void operator()(const float* sI, float* sD, int buf, int off) const {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (di[k] >= 0) {
        const float d = sI[ci[k] + off] - sI[ci[k]];
        sD[buf * M3_DN + di[k]] = in[k] ? d * d : 0.f;
      }
    }
  }
};
__device__ __forceinline__ float mind3_patch_sum(const float* d, const Mind3W& w) {
  float D = 0.f;
#pragma unroll
  for (int tz = 0; tz < 5; ++tz) {
#pragma unroll
    for (int ty = 0; ty < 5; ++ty) {
#pragma unroll
      for (int tx = 0; tx < 5; ++tx) D = fmaf(w.g[mind3_r2(tz, ty, tx)], d[tz * M3_DPS + ty * M3_DRS + tx], D);
    }
  }
  return D;
}

// f(a, D_a) for a = 0 .. 26 at this thread's voxel, a being a compile-time constant in each call (the forward keeps the 27
// numerators in registers). Every thread of the workgroup must call it (barriers inside); sI must be complete (a barrier
// after mind3_load_box) and is only read.
template <class F>
__device__ __forceinline__ void mind3_shifts(const float* sI, float* sD, const Mind3W& w, int z0, int y0, int x0, int D,
                                             int H, int W, F&& f) {
  const Mind3Pos p = mind3_pos();
  const Mind3Fill fill(z0, y0, x0, D, H, W);
  fill(sI, sD, 0, mind3_aoff(0));
  __syncthreads();
  static_for<0, M3_NS>([&](auto ic) {
    constexpr int a = decltype(ic)::value;
    if constexpr (a + 1 < M3_NS) fill(sI, sD, (a + 1) & 1, mind3_aoff(a + 1));
    f(ic, mind3_patch_sum(sD + (a & 1) * M3_DN + p.pz * M3_DPS + p.py * M3_DRS + p.px, w));
    __syncthreads();
  });
}
// the same as a loop (the backward keeps its per-shift values in its scratch volumes)
template <class F>
__device__ __forceinline__ void mind3_shifts_loop(const float* sI, float* sD, const Mind3W& w, int z0, int y0, int x0, int D,
                                                  int H, int W, F&& f) {
  const Mind3Pos p = mind3_pos();
  const Mind3Fill fill(z0, y0, x0, D, H, W);
  fill(sI, sD, 0, mind3_aoff(0));
  __syncthreads();
#pragma unroll 1
  for (int a = 0; a < M3_NS; ++a) {
    if (a + 1 < M3_NS) fill(sI, sD, (a + 1) & 1, mind3_aoff(a + 1));
    f(a, mind3_patch_sum(sD + (a & 1) * M3_DN + p.pz * M3_DPS + p.py * M3_DRS + p.px, w));
    __syncthreads();
  }
}

struct Mind3Box { int n, z0, y0, x0; };
__device__ __forceinline__ Mind3Box mind3_box(int bw, int bh, int bd) {
  int b = blockIdx.x;
  Mind3Box t;
  t.x0 = (b % bw) * M3_BX; b /= bw;
  t.y0 = (b % bh) * M3_BY; b /= bh;
  t.z0 = (b % bd) * M3_BZ;
  t.n = b / bd;
  return t;
}

// numerators n[27] and their sum Z of one sample at this thread's voxel; leaves the volume box in sI
__device__ __forceinline__ Mind3V mind3_numerators(const float* img, int C, int D, int H, int W, const Mind3Box& t,
                                                   const Mind3W& w, float* sI, float* sD, float (&n)[M3_NS], float& Z) {
  const Mind3Pos p = mind3_pos();
  mind3_load_box(img, C, D, H, W, t.z0, t.y0, t.x0, sI);
  __syncthreads();
  const Mind3V v = mind3_variance(sI, p, t.z0 + p.pz, t.y0 + p.py, t.x0 + p.px, D, H, W);
  float z = 0.f;
  mind3_shifts(sI, sD, w, t.z0, t.y0, t.x0, D, H, W, [&](auto ic, float Da) {
    constexpr int a = decltype(ic)::value;
    n[a] = expf(-Da / v.veps);
    z += n[a];
  });
  Z = z;
  return v;
}

__global__ __launch_bounds__(256) void mind3d_descriptor_kernel(const float* x, int C, int D, int H, int W, int bw, int bh,
                                                                int bd, const Mind3W w, float* out) {
  __shared__ float sI[M3_IN];
  __shared__ float sD[2 * M3_DN];
  const Mind3Box t = mind3_box(bw, bh, bd);
  const Mind3Pos p = mind3_pos();
  const int gz = t.z0 + p.pz, gy = t.y0 + p.py, gx = t.x0 + p.px;
  const size_t DHW = (size_t)D * H * W;
  float n[M3_NS], Z;
  mind3_numerators(x + (size_t)t.n * C * DHW, C, D, H, W, t, w, sI, sD, n, Z);
  if (gz < D && gy < H && gx < W) {
    float* o = out + (size_t)t.n * M3_NS * DHW + ((size_t)gz * H + gy) * W + gx;
    static_for<0, M3_NS>([&](auto ic) {
      constexpr int a = decltype(ic)::value;
      o[(size_t)a * DHW] = n[a] / Z;
    });
  }
}

__global__ __launch_bounds__(256) void mind3d_l1_kernel(const float* x, const float* y, int Cx, int Cy, int D, int H, int W,
                                                        int bw, int bh, int bd, const Mind3W w, float* partial) {
  __shared__ float sI[M3_IN];
  __shared__ float sD[2 * M3_DN];
  __shared__ float sh[4];
  const Mind3Box t = mind3_box(bw, bh, bd);
  const Mind3Pos p = mind3_pos();
  const int gz = t.z0 + p.pz, gy = t.y0 + p.py, gx = t.x0 + p.px;
  const size_t DHW = (size_t)D * H * W;
  float nx[M3_NS], ny[M3_NS], Zx, Zy;
  mind3_numerators(x + (size_t)t.n * Cx * DHW, Cx, D, H, W, t, w, sI, sD, nx, Zx);
  mind3_numerators(y + (size_t)t.n * Cy * DHW, Cy, D, H, W, t, w, sI, sD, ny, Zy);
  float acc = 0.f;
  static_for<0, M3_NS>([&](auto ic) {
    constexpr int a = decltype(ic)::value;
    acc += fabsf(nx[a] / Zx - ny[a] / Zy);
  });
  acc = mind_block_sum((gz < D && gy < H && gx < W) ? acc : 0.f, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---- backward w.r.t. the second volume --------------------------------------------------------------------------------
// With s = grad_scale / (D H W 27), sg_a = s sign(f_a^Y - f_a^X), Z = sum n:  dL/dn_a = (sg_a - sum_c sg_c f_c) / Z,
//   GD_a = -n_a / (V + eps) dL/dn_a,   GV = sum_a dL/dn_a n_a D_a / (V + eps)^2,   GB_b = GV 2 (B_b - mean B) / 26
// (re-centred: see the end of the first kernel).
// First launch: the volumes GD (27) and GB (27) per sample. A voxel's n_a^X and D_a^Y wait in scratch volumes (each thread
// reads back only what it wrote itself) until Z^X, Z^Y and then sum_c sg_c f_c are known; n_a^X's volume then takes GD_a.
// Per sample: volumes 0..26 GD, 27..53 GB, 54..80 D^Y. Second launch (a gather, one thread per voxel r):
//   dL/dI(r) = sum_a 2 [E_a(r - a) d_a(r - a) - E_a(r) d_a(r)] + sum_b F_b(r - b),
// E_a = g * GD_a and F_b = the 5^3 box sum of GB_b, both zero outside the volume; the result goes to every channel as 1/C.
#define M3_BWD_VOLS 81
__global__ __launch_bounds__(256) void mind3d_grad_maps_kernel(const float* x, const float* y, int Cx, int Cy, int D, int H,
                                                               int W, int bw, int bh, int bd, const Mind3W w,
                                                               const float* grad_scale, float inv_count, float* maps) {
  __shared__ float sI[M3_IN];
  __shared__ float sD[2 * M3_DN];
  const Mind3Box t = mind3_box(bw, bh, bd);
  const Mind3Pos p = mind3_pos();
  const int gz = t.z0 + p.pz, gy = t.y0 + p.py, gx = t.x0 + p.px;
  const bool valid = gz < D && gy < H && gx < W;
  const size_t DHW = (size_t)D * H * W;
  float* m = maps + (size_t)t.n * M3_BWD_VOLS * DHW + (valid ? ((size_t)gz * H + gy) * W + gx : 0);
  float* mD = m + (size_t)54 * DHW;

  mind3_load_box(x + (size_t)t.n * Cx * DHW, Cx, D, H, W, t.z0, t.y0, t.x0, sI);
  __syncthreads();
  const float vx = mind3_variance(sI, p, gz, gy, gx, D, H, W).veps;
  float Zx = 0.f;
  mind3_shifts_loop(sI, sD, w, t.z0, t.y0, t.x0, D, H, W, [&](int a, float Da) {
    const float n = expf(-Da / vx);
    Zx += n;
    if (valid) m[(size_t)a * DHW] = n;
  });
  mind3_load_box(y + (size_t)t.n * Cy * DHW, Cy, D, H, W, t.z0, t.y0, t.x0, sI);
  __syncthreads();
  const Mind3V v = mind3_variance(sI, p, gz, gy, gx, D, H, W);
  float Zy = 0.f;
  mind3_shifts_loop(sI, sD, w, t.z0, t.y0, t.x0, D, H, W, [&](int a, float Da) {
    Zy += expf(-Da / v.veps);
    if (valid) mD[(size_t)a * DHW] = Da;
  });
  if (!valid) return;
  const float s = (grad_scale ? grad_scale[0] : 1.f) * inv_count;
  auto sigma_a = [&](float fy, float fx) { const float df = fy - fx; return df > 0.f ? s : (df < 0.f ? -s : 0.f); };
  float S = 0.f;
#pragma unroll 1
  for (int a = 0; a < M3_NS; ++a) {
    const float fy = expf(-mD[(size_t)a * DHW] / v.veps) / Zy;
    S = fmaf(sigma_a(fy, m[(size_t)a * DHW] / Zx), fy, S);
  }
  float GV = 0.f;
#pragma unroll 1
  for (int a = 0; a < M3_NS; ++a) {
    const float Da = mD[(size_t)a * DHW], ny = expf(-Da / v.veps);
    const float dn = (sigma_a(ny / Zy, m[(size_t)a * DHW] / Zx) - S) / Zy;
    GV = fmaf(dn * ny, Da, GV);
    m[(size_t)a * DHW] = -ny / v.veps * dn;
  }
  GV = GV / (v.veps * v.veps);
  // The rounded mean leaves sum_b (B_b - mean) = 27 (true mean - mean) != 0, a share common to all 27 GB_b of the voxel. The
  // gather adds the GB_b of 125 voxels with all but cancelling signs, where a common share does not cancel: it is taken
  // out (the derivative of the mean as it was computed), so that sum_b GB_b = 0 to rounding.
  float rest = 0.f;
#pragma unroll
  for (int k = 0; k < M3_NS; ++k) rest += v.B[k] - v.mean;
  rest /= 27.f;
#pragma unroll
  for (int k = 0; k < M3_NS; ++k) m[(size_t)(M3_NS + k) * DHW] = GV * (2.f * ((v.B[k] - v.mean) - rest) / 26.f);
}

__global__ __launch_bounds__(256) void mind3d_gather_kernel(const float* y, int C, int D, int H, int W, int bw, int bh,
                                                            int bd, const Mind3W w, const float* maps, float* grad) {
  __shared__ float sI[M3_IN];
  __shared__ float sG[M3_IN];
  __shared__ float sE[M3_EZ * M3_EY * M3_EY];
  const Mind3Box t = mind3_box(bw, bh, bd);
  const Mind3Pos p = mind3_pos();
  const int gz = t.z0 + p.pz, gy = t.y0 + p.py, gx = t.x0 + p.px;
  const size_t DHW = (size_t)D * H * W;
  const float* mp = maps + (size_t)t.n * M3_BWD_VOLS * DHW;
  mind3_load_box(y + (size_t)t.n * C * DHW, C, D, H, W, t.z0, t.y0, t.x0, sI);
  float acc = 0.f;
#pragma unroll 1
  for (int a = 0; a < M3_NS; ++a) {
    const int az = mind3_az(a), ay = mind3_ay(a), ax = mind3_ax(a);
    if (az == 0 && ay == 0 && ax == 0) continue;        // d_a = 0: nothing flows through the zero shift
    mind3_load_box(mp + (size_t)a * DHW, 1, D, H, W, t.z0, t.y0, t.x0, sG);
    __syncthreads();
    // E_a on the box and a ring of 1 around it (origin - 1), zero outside the volume
    for (int e = threadIdx.x; e < M3_EZ * M3_EY * M3_EY; e += 256) {
      const int ez = e / (M3_EY * M3_EY), rem = e - ez * (M3_EY * M3_EY), ey = rem / M3_EY, ex = rem - ey * M3_EY;
      float E = 0.f;
      if (mind3_in(t.z0 - 1 + ez, t.y0 - 1 + ey, t.x0 - 1 + ex, D, H, W)) {
        const float* gsrc = sG + ez * M3_IPS + ey * M3_IY + ex;
#pragma unroll
        for (int tz = 0; tz < 5; ++tz) {
#pragma unroll
          for (int ty = 0; ty < 5; ++ty) {
#pragma unroll
            for (int tx = 0; tx < 5; ++tx) E = fmaf(w.g[mind3_r2(tz, ty, tx)], gsrc[tz * M3_IPS + ty * M3_IY + tx], E);
          }
        }
      }
      sE[e] = E;
    }
    __syncthreads();
    const int ic = (p.pz + 3) * M3_IPS + (p.py + 3) * M3_IY + p.px + 3, io = az * M3_IPS + ay * M3_IY + ax;
    const float Ir = sI[ic], Ipa = sI[ic + io], Ima = sI[ic - io];
    const float Er = sE[(p.pz + 1) * (M3_EY * M3_EY) + (p.py + 1) * M3_EY + p.px + 1];
    const float Era = sE[(p.pz + 1 - az) * (M3_EY * M3_EY) + (p.py + 1 - ay) * M3_EY + p.px + 1 - ax];
    acc += 2.f * (Era * (Ir - Ima) - Er * (Ipa - Ir));
  }
#pragma unroll 1
  for (int k = 0; k < M3_NS; ++k) {
    const int bz = mind3_az(k), by = mind3_ay(k), bx = mind3_ax(k);
    __syncthreads();
    mind3_load_box(mp + (size_t)(M3_NS + k) * DHW, 1, D, H, W, t.z0, t.y0, t.x0, sG);
    __syncthreads();
    if (mind3_in(gz - bz, gy - by, gx - bx, D, H, W)) {
      const float* gsrc = sG + (p.pz + 1 - bz) * M3_IPS + (p.py + 1 - by) * M3_IY + p.px + 1 - bx;
      float F = 0.f;
#pragma unroll
      for (int tz = 0; tz < 5; ++tz) {
#pragma unroll
        for (int ty = 0; ty < 5; ++ty) {
#pragma unroll
          for (int tx = 0; tx < 5; ++tx) F += gsrc[tz * M3_IPS + ty * M3_IY + tx];
        }
      }
      acc += F;
    }
  }
  if (gz < D && gy < H && gx < W) {
    const float gval = C > 1 ? acc / (float)C : acc;
    float* o = grad + (size_t)t.n * C * DHW + ((size_t)gz * H + gy) * W + gx;
    for (int ch = 0; ch < C; ++ch) o[(size_t)ch * DHW] = gval;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// the weights (mind_weight) by squared distance: that of a tap of the 5^3 patch is an integer in 0 .. 12
static Mind3W mind3_weights(float sigma) {
  Mind3W w;
  for (int r2 = 0; r2 < 13; ++r2) w.g[r2] = mind_weight(r2, sigma);
  return w;
}

struct Mind3Grid { int bd, bh, bw; int64_t blocks; };
static Mind3Grid mind3_grid(int N, int D, int H, int W) {
  Mind3Grid g;
  g.bd = mind_ceil_div(D, M3_BZ);
  g.bh = mind_ceil_div(H, M3_BY);
  g.bw = mind_ceil_div(W, M3_BX);
  g.blocks = (int64_t)N * g.bd * g.bh * g.bw;
  return g;
}

#define MIND3_REQUIRE_SIZES(name)                                                                                       \
  if (int rc = mind_check_sizes(name, 3, 5, nl_size, patch_size, neighbor_size, sigma, N > 0 && D > 0 && H > 0 && W > 0))   \
    return rc;                                                                                                          \
  GS_REQUIRE((int64_t)D * H * W < (1ll << 31), name ": a sample of 2^31 or more voxels");                               \
  GS_REQUIRE(mind3_grid(N, D, H, W).blocks < (1ll << 31), name ": too many boxes")

extern "C" int64_t gs_mind3d_scratch_bytes(int32_t N, int32_t D, int32_t H, int32_t W, int32_t backward) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  if (backward) return (int64_t)N * M3_BWD_VOLS * D * H * W * (int64_t)sizeof(float);
  return mind3_grid(N, D, H, W).blocks * (int64_t)sizeof(float);
}

extern "C" int gs_mind3d_descriptor(const float* x, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t nl_size,
                                    int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* stream) {
  GS_REQUIRE(x && out && C > 0, "gs_mind3d_descriptor: bad argument");
  MIND3_REQUIRE_SIZES("gs_mind3d_descriptor");
  const Mind3Grid g = mind3_grid(N, D, H, W);
  hipLaunchKernelGGL(mind3d_descriptor_kernel, dim3((unsigned)g.blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     C, D, H, W, g.bw, g.bh, g.bd, mind3_weights(sigma), out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_mind3d_l1(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t D, int32_t H,
                            int32_t W, int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma, float* out,
                            void* scratch, void* stream) {
  GS_REQUIRE(x && y && out && scratch && Cx > 0 && Cy > 0, "gs_mind3d_l1: bad argument");
  MIND3_REQUIRE_SIZES("gs_mind3d_l1");
  const Mind3Grid g = mind3_grid(N, D, H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(scratch);
  hipLaunchKernelGGL(mind3d_l1_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, x, y, Cx, Cy, D, H, W, g.bw, g.bh, g.bd,
                     mind3_weights(sigma), partial);
  hipLaunchKernelGGL((final_sum_kernel<float, 256>), dim3(1), dim3(256), 0, st, (const float*)partial, (int)g.blocks,
                     1.0 / ((double)D * H * W * M3_NS), out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int gs_mind3d_l1_backward(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t D, int32_t H,
                                     int32_t W, int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma,
                                     const float* grad_scale, float* grad_y, void* scratch, void* stream) {
  GS_REQUIRE(x && y && grad_y && scratch && Cx > 0 && Cy > 0, "gs_mind3d_l1_backward: bad argument");
  MIND3_REQUIRE_SIZES("gs_mind3d_l1_backward");
  const Mind3Grid g = mind3_grid(N, D, H, W);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* maps = static_cast<float*>(scratch);
  const Mind3W w = mind3_weights(sigma);
  hipLaunchKernelGGL(mind3d_grad_maps_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, x, y, Cx, Cy, D, H, W, g.bw, g.bh,
                     g.bd, w, grad_scale, (float)(1.0 / ((double)D * H * W * M3_NS)), maps);
  hipLaunchKernelGGL(mind3d_gather_kernel, dim3((unsigned)g.blocks), dim3(256), 0, st, y, Cy, D, H, W, g.bw, g.bh, g.bd, w,
                     (const float*)maps, grad_y);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
