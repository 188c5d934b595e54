// Device-side sampling of multi-modal training patches (data/multimodal_volumes.py, data/device_volumes.py): the
// HX4-PET dataset of the reference (projects/maastro_hx4_pet_translation/datasets/train_dataset.py with
// datasets/utils/patch_samplers.py and basic.py) draws the patch centre ("focal point") inside a body mask — uniformly or
// weighted by a PET volume — by building a float64 probability map of the whole volume per sample. Here the volumes and
// masks are RESIDENT in HBM and the draw is a masked prefix sum over the valid zone's box; the uniform u comes from the
// host's np.random stream, everything else stays on the device.
//
// gs_voxel_draw — the selection rule (ganslate_hip.h states it in full): over the zone box in C order,
//   mask-only:  the k-th non-zero voxel, k = min(floor(u * count), count - 1)         (int64, exact)
//   weighted:   the first voxel whose inclusive float64 prefix sum exceeds u * total;  fallback: the last positive one
// restricted to the stochastic-focal box around A's point when that intersection is not empty (flag 0), else
// unrestricted (flag 1). Three launches, no atomics, no host round trip:
//   1. NR workgroups, each owning a contiguous C-order range of the box; every thread sums one contiguous run of its range
//      in index order, thread 0 adds the 256 run sums in index order -> per-range partials for both sets
//   2. one thread scans the NR partials in index order: picks the set, the owning range and the residual target
//   3. the owning range repeats pass 1's sums (bitwise the same numbers), thread 0 finds the owning run, and that run's
//      thread rescans it and stores the voxel
// Every sum has one fixed order, so a draw is bitwise reproducible; pass 3 re-derives exactly the partial pass 2 compared
// against, so the owning run always exists. HBM-bound and small: 1 B (mask) or 1 + 4 B (mask + fp32 weight) per voxel of a
// box of a few MB, read once plus one range. The lanes of a wave read adjacent short runs, i.e. one contiguous span per
// wave; that and in-order scans are all this kernel needs — it is not tuned further.
//
// gs_patch_clip_minmax — crop + per-modality normalisation of all C modalities of one sample in one launch:
//   v = mask ? (float)x : outside;  v = v / divisor;  v = min(max(v, lo), hi);  v = (v - lo) / (hi - lo);  v = 2 * v - 1
// one IEEE fp32 operation per step (no contraction), the focal point read from device memory, the start clamped into the
// volume so that no point can make the kernel read outside it.
//
// gs_patch_affine_clip_minmax / gs_patch_affine — the same crop through a 3 x 3 matrix (random flips, rotation, zoom: data/
// utils/patch_affine.py): per output voxel float64 source coordinates round the patch centre, the eight corners masked and
// bounds-checked one by one, three rounded-step fp32 lerps (W, H, D), then the same chain (or none, for the raw gather that
// feeds gs_patch_zscore). One thread per voxel, the modalities looped inside it; no contraction anywhere in the definition.
// gs_patch_elastic_clip_minmax / gs_patch_elastic — the same kernel with a free-form deformation (a lattice of control-point
// displacements, cubic B-splines) added to the patch offset in front of the matrix: a compile-time variant of that kernel.
// gs_patch_augment_clip_minmax — either of the two with the intensity chain of intensity.hpp (bias field, contrast,
// brightness, gamma, noise) between the min-max step and 2 n - 1: one more compile-time variant.
//
// gs_volume_prepare — a whole case for the val / test engines (data/multimodal_valtest.py): the same mask step and the same
// per-voxel chain (one device function, clip_minmax), with centred padding up to a target shape in between; the pad value is
// the minimum of the masked volume over the case, NaN-propagating like np.min, each mask padded with its own minimum. Two
// launches: 256 partial minima per volume / mask, then the apply pass, whose workgroups fold the partials in one fixed tree.
//
// ModTable — the per-modality columns (volume pointer, dtype, outside, divisor, lo, hi) that every kernel argument struct
// of these entries begins with. One host function, fill_table, checks the caller's arrays and fills it; check_patch_fits and
// patch_start (the start clamp, device side) are the other rules the entries share.
#include <limits>
#include "common.hpp"
#include "intensity.hpp"

namespace {
constexpr int NR = 256;      // ranges = workgroups of pass 1
constexpr int NT = 256;      // threads per workgroup = runs per range

struct DrawK {
  const uint8_t* mask;
  const void* weight;
  int D, H, W;
  int z0, y0, x0, bd, bh, bw;      // the valid zone's box
  long long n, L, S;               // voxels of the box, voxels per range, voxels per run
  double u;
  const int32_t* focal_a;          // device: the point drawn in A (nullptr: no focal box)
  int da[3], region[3];            // A's dims; focal region size in voxels of this volume
};

template <typename V>
struct Sel {
  int range, set;
  V resid;
};

template <typename T>
using Vt = typename std::conditional<std::is_void<T>::value, long long, double>::type;

template <typename V>
__device__ __forceinline__ V never() {
  if constexpr (std::is_same<V, double>::value) return std::numeric_limits<double>::infinity();
  else return std::numeric_limits<long long>::max();
}

// the reference's _sample_focal_point_B / _apply_stochastic_focal_method in float64, one rounding per operation
__device__ __forceinline__ void focal_box(const DrawK& k, int lo[3], int hi[3]) {
  const int size[3] = {k.D, k.H, k.W};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = 0;
    hi[a] = size[a];
    if (k.focal_a) {
      const double rel = __ddiv_rn((double)k.focal_a[a], (double)k.da[a]);
      const double f = __dmul_rn(rel, (double)size[a]);
      const double half = __ddiv_rn((double)k.region[a], 2.0);
      const int mn = (int)__dsub_rn(f, half), mx = (int)__dadd_rn(f, half);
      lo[a] = mn > 0 ? mn : 0;
      hi[a] = mx < size[a] ? mx : size[a];
    }
  }
}

template <typename T>
__device__ __forceinline__ Vt<T> weight_at(const DrawK& k, long long off) {
  using V = Vt<T>;
  if (!k.mask[off]) return V(0);
  if constexpr (std::is_void<T>::value) {
    return V(1);
  } else {
    const double w = (double)static_cast<const T*>(k.weight)[off];
    return w > 0.0 ? w : 0.0;      // negative (and NaN) weights count as 0
  }
}

// the run of thread t of range r: [b, e) in box C order
__device__ __forceinline__ void run_bounds(const DrawK& k, int r, int t, long long& b, long long& e) {
  const long long rb = (long long)r * k.L;
  long long re = rb + k.L;
  if (re > k.n) re = k.n;
  b = rb + (long long)t * k.S;
  e = b + k.S;
  if (e > re) e = re;
}

// f(z, y, x, weight) in index order over [b, e), volume coordinates; f returns false to stop
template <typename T, typename F>
__device__ __forceinline__ void walk_run(const DrawK& k, long long b, long long e, F&& f) {
  if (b >= e) return;
  int x = (int)(b % k.bw);
  const long long row = b / k.bw;
  int y = (int)(row % k.bh), z = (int)(row / k.bh);
  for (long long i = b; i < e; ++i) {
    const long long off = ((long long)(k.z0 + z) * k.H + (k.y0 + y)) * k.W + (k.x0 + x);
    if (!f(k.z0 + z, k.y0 + y, k.x0 + x, weight_at<T>(k, off))) return;
    if (++x == k.bw) {
      x = 0;
      if (++y == k.bh) { y = 0; ++z; }
    }
  }
}

__device__ __forceinline__ bool inside(const int lo[3], const int hi[3], int z, int y, int x) {
  return z >= lo[0] && z < hi[0] && y >= lo[1] && y < hi[1] && x >= lo[2] && x < hi[2];
}

// partial[2 r] = sum over (focal box ∩ range r), partial[2 r + 1] = sum over range r
template <typename T>
__global__ __launch_bounds__(NT) void draw_partials_kernel(const DrawK k, Vt<T>* partial) {
  using V = Vt<T>;
  __shared__ V sf[NT], sz[NT];
  int lo[3], hi[3];
  focal_box(k, lo, hi);
  long long b, e;
  run_bounds(k, blockIdx.x, threadIdx.x, b, e);
  V af = 0, az = 0;
  walk_run<T>(k, b, e, [&](int z, int y, int x, V w) {
    az += w;
    if (inside(lo, hi, z, y, x)) af += w;
    return true;
  });
  sf[threadIdx.x] = af;
  sz[threadIdx.x] = az;
  __syncthreads();
  if (threadIdx.x == 0) {
    V a = 0, c = 0;
    for (int i = 0; i < NT; ++i) { a += sf[i]; c += sz[i]; }
    partial[2 * blockIdx.x] = a;
    partial[2 * blockIdx.x + 1] = c;
  }
}

// first index whose entry exceeds what is left of the target, scanning in index order; none: the last positive entry,
// with a residual nothing exceeds (the rescans then end at their last positive voxel)
template <typename V, typename G>
__device__ __forceinline__ int owner_of(int count, V target, V& resid, G&& get) {
  V before = 0;
  int lastpos = -1;
  for (int i = 0; i < count; ++i) {
    const V p = get(i);
    if (p > 0) lastpos = i;
    const V rs = target - before;
    if (p > rs) { resid = rs; return i; }
    before += p;
  }
  resid = never<V>();
  return lastpos;
}

template <typename T>
__global__ void draw_select_kernel(const DrawK k, const Vt<T>* partial, Sel<Vt<T>>* sel, int32_t* out) {
  using V = Vt<T>;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  V tf = 0, tz = 0;
  for (int r = 0; r < NR; ++r) { tf += partial[2 * r]; tz += partial[2 * r + 1]; }
  const bool focal = k.focal_a != nullptr;
  const int set = (focal && tf > 0) ? 0 : 1;
  const int flag = (focal && !(tf > 0)) ? 1 : 0;
  const V total = set == 0 ? tf : tz;
  out[3] = flag;
  if (!(total > 0)) {                      // empty zone ∩ body, or no positive weight in it
    out[0] = out[1] = out[2] = -1;
    sel->range = -1;
    return;
  }
  V target;
  if constexpr (std::is_void<T>::value) {
    long long kk = (long long)floor(__dmul_rn(k.u, (double)total));
    if (kk > total - 1) kk = total - 1;
    if (kk < 0) kk = 0;
    target = kk;                           // the k-th non-zero voxel is the first with inclusive count > k
  } else {
    target = __dmul_rn(k.u, total);
  }
  V resid;
  sel->range = owner_of<V>(NR, target, resid, [&](int r) { return partial[2 * r + set]; });
  sel->set = set;
  sel->resid = resid;
}

template <typename T>
__global__ __launch_bounds__(NT) void draw_locate_kernel(const DrawK k, const Sel<Vt<T>>* sel, int32_t* out) {
  using V = Vt<T>;
  __shared__ V s[NT];
  __shared__ int own_run;
  __shared__ V own_resid;
  const int r = sel->range;
  if (r < 0) return;
  const bool all = sel->set != 0;
  int lo[3], hi[3];
  focal_box(k, lo, hi);
  long long b, e;
  run_bounds(k, r, threadIdx.x, b, e);
  V a = 0;
  walk_run<T>(k, b, e, [&](int z, int y, int x, V w) {
    if (all || inside(lo, hi, z, y, x)) a += w;
    return true;
  });
  s[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    V resid;
    own_run = owner_of<V>(NT, sel->resid, resid, [&](int i) { return s[i]; });
    own_resid = resid;
  }
  __syncthreads();
  if ((int)threadIdx.x != own_run) return;
  const V resid = own_resid;
  V acc = 0;
  int pz = -1, py = -1, px = -1;
  walk_run<T>(k, b, e, [&](int z, int y, int x, V w) {
    if (!(w > 0) || !(all || inside(lo, hi, z, y, x))) return true;
    pz = z; py = y; px = x;
    acc += w;
    return !(acc > resid);
  });
  out[0] = pz;
  out[1] = py;
  out[2] = px;
}

template <typename T>
int launch_draw(const DrawK& k, int32_t* out, void* ws, hipStream_t st) {
  using V = Vt<T>;
  V* partial = static_cast<V*>(ws);
  Sel<V>* sel = reinterpret_cast<Sel<V>*>(partial + 2 * NR);
  hipLaunchKernelGGL((draw_partials_kernel<T>), dim3(NR), dim3(NT), 0, st, k, partial);
  hipLaunchKernelGGL((draw_select_kernel<T>), dim3(1), dim3(64), 0, st, k, partial, sel, out);
  hipLaunchKernelGGL((draw_locate_kernel<T>), dim3(1), dim3(NT), 0, st, k, sel, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// the valid zone [floor(p / 2), size - ceil(p / 2)) of one axis
inline int zone_lo(int p) { return p / 2; }
inline int zone_hi(int size, int p) { return size - (p + 1) / 2; }

long long range_len(int D, int H, int W, const int32_t* p) {
  const long long bd = zone_hi(D, p[0]) - zone_lo(p[0]), bh = zone_hi(H, p[1]) - zone_lo(p[1]),
                  bw = zone_hi(W, p[2]) - zone_lo(p[2]);
  if (bd <= 0 || bh <= 0 || bw <= 0) return 0;
  return (bd * bh * bw + NR - 1) / NR;
}

constexpr int PC_MAX = GS_PATCH_MAX_MODALITIES;

// the per-modality columns, the leading base of ClipK, AffK and PrepK: the kernels read k.vol[c], k.lo[c], ...
struct ModTable {
  const void* vol[PC_MAX];
  int dtype[PC_MAX];
  float outside[PC_MAX], divisor[PC_MAX], lo[PC_MAX], hi[PC_MAX];
};

// checks the C caller-side entries and fills all PC_MAX slots, the unused ones from slot 0 (no kernel reads them)
int fill_table(const char* who, ModTable& t, const void* const* vols, const int32_t* dtypes, const float* outside,
               const float* divisor, const float* lo, const float* hi, int C) {
  for (int c = 0; c < PC_MAX; ++c) {
    const int s = c < C ? c : 0;
    GS_REQUIRE(vols[s], "%s: null volume %d", who, s);
    GS_REQUIRE(dtypes[s] == GS_VOL_F32 || dtypes[s] == GS_VOL_I16, "%s: dtype %d of volume %d (GS_VOL_F32 / GS_VOL_I16)", who,
               dtypes[s], s);
    GS_REQUIRE(hi[s] > lo[s], "%s: clip range [%g, %g] of volume %d is empty", who, lo[s], hi[s], s);
    GS_REQUIRE(divisor[s] != 0.f && divisor[s] == divisor[s], "%s: divisor %g of volume %d", who, divisor[s], s);
    t.vol[c] = vols[s];
    t.dtype[c] = dtypes[s];
    t.outside[c] = outside[s]; t.divisor[c] = divisor[s]; t.lo[c] = lo[s]; t.hi[c] = hi[s];
  }
  return 0;
}

int check_patch_fits(const char* who, int D, int H, int W, const int32_t* p) {
  GS_REQUIRE(D > 0 && H > 0 && W > 0 && p[0] > 0 && p[1] > 0 && p[2] > 0 && p[0] <= D && p[1] <= H && p[2] <= W,
             "%s: patch %d x %d x %d does not fit the %d x %d x %d volume", who, p[0], p[1], p[2], D, H, W);
  return 0;
}

// the patch start on one axis: point - patch / 2, clamped to [0, size - patch], so that no point reads outside the volume
__device__ __forceinline__ int patch_start(int point, int patch, int size) {
  int v = point - patch / 2;
  const int top = size - patch;
  v = v > top ? top : v;
  return v < 0 ? 0 : v;
}

struct ClipK : ModTable {
  const uint8_t* mask;
  const int32_t* point;
  int D, H, W, pd, ph, pw;
  long long n;
};

// the per-voxel chain behind the mask of gs_patch_clip_minmax and gs_volume_prepare: one rounding per step
__device__ __forceinline__ float clip_minmax(float v, float divisor, float lo, float hi, float span) {
  v = __fdiv_rn(v, divisor);
  v = v < lo ? lo : v;                     // NaN stays NaN, like torch.clamp
  v = v > hi ? hi : v;
  v = __fdiv_rn(__fsub_rn(v, lo), span);
  return __fsub_rn(__fmul_rn(2.f, v), 1.f);
}

__device__ __forceinline__ float voxel_or(const void* vol, int dtype, long long off, bool in, float outside) {
  if (!in) return outside;
  return dtype == GS_VOL_F32 ? static_cast<const float*>(vol)[off] : (float)static_cast<const short*>(vol)[off];
}

__global__ __launch_bounds__(256) void patch_clip_minmax_kernel(const ClipK k, float* out) {
  const int c = blockIdx.y;
  const int size[3] = {k.D, k.H, k.W}, patch[3] = {k.pd, k.ph, k.pw};
  int s[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) s[a] = patch_start(k.point[a], patch[a], size[a]);
  const void* vol = k.vol[c];
  const int dtype = k.dtype[c];
  const float outside = k.outside[c], divisor = k.divisor[c], lo = k.lo[c], hi = k.hi[c];
  const float span = __fsub_rn(hi, lo);
  float* dst = out + (long long)c * k.n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < k.n; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % k.pw);
    const long long row = i / k.pw;
    const int y = (int)(row % k.ph), z = (int)(row / k.ph);
    const long long off = ((long long)(s[0] + z) * k.H + (s[1] + y)) * k.W + (s[2] + x);
    const float v = voxel_or(vol, dtype, off, k.mask[off] != 0, outside);
    dst[i] = clip_minmax(v, divisor, lo, hi, span);
  }
}

// ---- gs_patch_affine_clip_minmax / gs_patch_affine --------------------------------------------------------------------
// The augmented patch (ganslate_hip.h states the definition): one thread per output voxel, W fastest, so the 64 lanes of a
// wave walk one line of the source and their eight corner reads fall into a few neighbouring rows. Coordinates (float64),
// the in-bounds tests and the mask bytes are per voxel; the modalities are looped inside the thread, each plane's store
// coalesced. hipcc contracts a * b + c to an fma by default, through __fmul_rn / __fadd_rn too (slidewin.hip), so the
// coordinate and lerp bodies switch contraction off.
struct AffK : ModTable {
  const uint8_t* mask;             // nullptr: no mask (gs_patch_affine)
  const int32_t* point;            // device focal point; nullptr: start[] is the patch start
  int start[3];
  double M[9];
  int C, D, H, W, pd, ph, pw;
  long long n;
};

__device__ __forceinline__ double affine_coord(const double* m, double r0, double r1, double r2, double base) {
#pragma clang fp contract(off)
  const double a = m[0] * r0;
  const double b = m[1] * r1;
  const double c = m[2] * r2;
  const double ab = a + b;
  const double abc = ab + c;
  return abc + base;
}

__device__ __forceinline__ float lerp_rn(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float p = t * d;
  return a + p;
}

// ---- the elastic variant (gs_patch_elastic_clip_minmax / gs_patch_elastic) ---------------------------------------------
// A free-form deformation in front of the matrix (ganslate_hip.h states the definition): r'_a = r_a + u_a(o), u the cubic
// B-spline interpolation of a coarse lattice of displacements that spans the patch. The lattice (up to 24 KB of float64)
// arrives as a device buffer. Two forms, the same bits by construction (the definition sums D innermost, W outermost, so
// R[a][n] of a lattice column is a function of the output row (o_0, o_1) alone):
//   ELA_ROWS   a workgroup's 256 consecutive voxels cover at most 255 / w + 2 rows; its threads compute R[row][a][k] for
//              every lattice column k of those rows once, from the lattice through L2, into LDS (rows * 3 * G_2 doubles);
//              a voxel then takes its W weights and 4 multiplies per component. Used when that table fits the option
//              elastic_rows (32 KB).
//   ELA_VOXEL  the lattice staged to LDS per workgroup, all 64 + 16 + 4 products per component in every thread: for short
//              rows under a wide lattice, whose row table would not fit.
struct ElaK : AffK {
  const double* field;             // DEVICE double[3][G0][G1][G2], voxels
  int G[3];
};

enum { ELA_NONE = 0, ELA_VOXEL = 1, ELA_ROWS = 2 };

// cooperative part, every thread of the workgroup: fills the LDS of its form and synchronises
template <int E>
__device__ __forceinline__ void elastic_stage(const ElaK& k, double* lds) {
  const int GN = k.G[0] * k.G[1] * k.G[2];
  if constexpr (E == ELA_VOXEL) {
    for (int e = threadIdx.x; e < 3 * GN; e += 256) lds[e] = k.field[e];
  } else {
    const long long first = (long long)blockIdx.x * 256;
    long long last = first + 255;
    last = last < k.n ? last : k.n - 1;
    const long long row0 = first / k.pw;
    const int rows = (int)(last / k.pw - row0) + 1;        // <= min(d h, 255 / w + 2), what the host sized the table for
    const int per = 3 * k.G[2];
    for (int e = threadIdx.x; e < rows * per; e += 256) {
      const int rl = e / per, a = (e % per) / k.G[2], col = e % k.G[2];
      const long long row = row0 + rl;
      double Bz[4], By[4];
      const int j0 = bspline_axis((int)(row / k.ph), k.pd, k.G[0], Bz);
      const int j1 = bspline_axis((int)(row % k.ph), k.ph, k.G[1], By);
      lds[e] = lattice_R(k.field + (long long)a * GN + (j0 * k.G[1] + j1) * k.G[2] + col, k.G[1], k.G[2], Bz, By);
    }
  }
  __syncthreads();
}

// u_a of output voxel o, added to r_a: one float64 add per axis
template <int E>
__device__ __forceinline__ void elastic_displace(const ElaK& k, const double* lds, const int o[3], long long i, double r[3]) {
#pragma clang fp contract(off)
  double Bx[4];
  const int j2 = bspline_axis(o[2], k.pw, k.G[2], Bx);
  double u[3];
  if constexpr (E == ELA_VOXEL) {
    const int GN = k.G[0] * k.G[1] * k.G[2];
    double Bz[4], By[4];
    const int j0 = bspline_axis(o[0], k.pd, k.G[0], Bz);
    const int j1 = bspline_axis(o[1], k.ph, k.G[1], By);
    const double* F = lds + (j0 * k.G[1] + j1) * k.G[2] + j2;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double R[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) R[n] = lattice_R(F + a * GN + n, k.G[1], k.G[2], Bz, By);
      u[a] = dot4(Bx, R[0], R[1], R[2], R[3]);
    }
  } else {
    const int rl = (int)(i / k.pw - ((long long)blockIdx.x * 256) / k.pw);
    const double* R = lds + rl * 3 * k.G[2] + j2;
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = dot4(Bx, R[a * k.G[2]], R[a * k.G[2] + 1], R[a * k.G[2] + 2], R[a * k.G[2] + 3]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) r[a] = r[a] + u[a];
}

// ---- the intensity variant (gs_patch_augment_clip_minmax) ----------------------------------------------------------------
// The chain of intensity.hpp in the CLIP epilogue, between (v - lo) / span and 2 n - 1 (ganslate_hip.h states the
// definition). IntK wraps the argument of the geometric form it rides on. The bias lattice BETA (one scalar lattice, up to
// 8 KB of float64, a grid of its own) is evaluated once per voxel in front of the modality loop, in the forms of the elastic
// part and behind its LDS: `bform` ELA_ROWS adds BG[2] doubles per row to the row table, ELA_VOXEL stages the lattice;
// ELA_NONE is a launch without a lattice. The host picks one form for both lattices, by the size of the combined table.
template <typename B>
struct IntK : B {
  GsPatchIntensity it[PC_MAX];
  const double* beta;              // DEVICE double[BG0][BG1][BG2], or nullptr
  int BG[3];
  int bform, boff;                 // boff: doubles of LDS in front of the bias part
};

template <typename K>
__device__ __forceinline__ void bias_stage(const K& k, double* lds) {
  if (k.bform == ELA_NONE) return;                         // uniform over the launch
  if (k.bform == ELA_VOXEL) {
    const int GN = k.BG[0] * k.BG[1] * k.BG[2];
    for (int e = threadIdx.x; e < GN; e += 256) lds[e] = k.beta[e];
  } else {
    const long long first = (long long)blockIdx.x * 256;
    long long last = first + 255;
    last = last < k.n ? last : k.n - 1;
    const long long row0 = first / k.pw;
    const int rows = (int)(last / k.pw - row0) + 1;        // as in elastic_stage
    const int per = k.BG[2];
    for (int e = threadIdx.x; e < rows * per; e += 256) {
      const long long row = row0 + e / per;
      double Bz[4], By[4];
      const int j0 = bspline_axis((int)(row / k.ph), k.pd, k.BG[0], Bz);
      const int j1 = bspline_axis((int)(row % k.ph), k.ph, k.BG[1], By);
      lds[e] = lattice_R(k.beta + (j0 * k.BG[1] + j1) * k.BG[2] + e % per, k.BG[1], k.BG[2], Bz, By);
    }
  }
  __syncthreads();
}

template <typename K>
__device__ __forceinline__ double bias_at(const K& k, const double* lds, const int o[3], long long i) {
  if (k.bform == ELA_NONE) return 0.0;
  if (k.bform == ELA_VOXEL) {
    const int patch[3] = {k.pd, k.ph, k.pw};
    return lattice_at(lds, k.BG, o, patch);
  }
  double Bx[4];
  const int j2 = bspline_axis(o[2], k.pw, k.BG[2], Bx);
  const int rl = (int)(i / k.pw - ((long long)blockIdx.x * 256) / k.pw);
  const double* R = lds + rl * k.BG[2] + j2;
  return dot4(Bx, R[0], R[1], R[2], R[3]);
}

// clip_minmax up to the normalised value n, and its last step
__device__ __forceinline__ float clip_unit(float v, float divisor, float lo, float hi, float span) {
  v = __fdiv_rn(v, divisor);
  v = v < lo ? lo : v;
  v = v > hi ? hi : v;
  return __fdiv_rn(__fsub_rn(v, lo), span);
}

template <bool CLIP, int E, typename K, bool INT = false>
__global__ __launch_bounds__(256) void patch_affine_kernel(const K k, float* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  extern __shared__ __attribute__((aligned(16))) double ela_lds[];
  if constexpr (E != ELA_NONE) elastic_stage<E>(k, ela_lds);
  if constexpr (INT) bias_stage(k, ela_lds + k.boff);
  if (i >= k.n) return;
  const int size[3] = {k.D, k.H, k.W}, patch[3] = {k.pd, k.ph, k.pw};
  int o[3];
  o[2] = (int)(i % k.pw);
  const long long row = i / k.pw;
  o[1] = (int)(row % k.ph);
  o[0] = (int)(row / k.ph);
  double r[3], base[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int s = k.start[a];
    if (k.point) s = patch_start(k.point[a], patch[a], size[a]);
    const double c = (double)(patch[a] - 1) * 0.5;       // exact
    r[a] = (double)o[a] - c;                             // exact
    base[a] = (double)s + c;                             // exact
  }
  double beta = 0.0;
  if constexpr (INT) beta = bias_at(k, ela_lds + k.boff, o, i);
  if constexpr (E != ELA_NONE) elastic_displace<E>(k, ela_lds, o, i, r);
  int ix[3];
  float t[3];
  bool reach = true;                                     // false: all eight corners are outside
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = affine_coord(k.M + 3 * a, r[0], r[1], r[2], base[a]);
    const double f = floor(s);
    t[a] = (float)__dsub_rn(s, f);
    const bool in = s >= -1.0 && s < (double)size[a];    // NaN: outside
    reach = reach && in;
    ix[a] = in ? (int)f : 0;                             // in [-1, size - 1]
    // a NaN or infinite displacement: s - floor(s) is no number. The corners are all `outside` then, which any finite t
    // lerps to `outside` itself, so 0 changes no finite case
    if constexpr (E != ELA_NONE) t[a] = in ? t[a] : 0.f;
  }
  // off[q], q = dz * 4 + dy * 2 + dx: where corner q is read. A corner that takes the outside value reads voxel 0 instead
  // (there always is one) and drops it: every load is unconditional, so the eight of a stage are in flight together
  // instead of one round trip per branch.
  const long long off0 = ((long long)ix[0] * k.H + ix[1]) * k.W + ix[2];
  const long long sz = (long long)k.H * k.W, sy = k.W;
  long long off[8];
  unsigned valid = 0;                                    // bit q: corner q is read
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int z = ix[0] + (q >> 2), y = ix[1] + ((q >> 1) & 1), x = ix[2] + (q & 1);
    const bool in = reach && (unsigned)z < (unsigned)k.D && (unsigned)y < (unsigned)k.H && (unsigned)x < (unsigned)k.W;
    off[q] = in ? off0 + (q >> 2) * sz + ((q >> 1) & 1) * sy + (q & 1) : 0;
    valid |= in ? 1u << q : 0u;
  }
  if (k.mask) {
    uint8_t m[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) m[q] = k.mask[off[q]];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (!m[q]) {
        valid &= ~(1u << q);
        off[q] = 0;
      }
    }
  }
  for (int c = 0; c < k.C; ++c) {
    const float outside = k.outside[c];
    float v[8];
    if (k.dtype[c] == GS_VOL_F32) {
      const float* vol = static_cast<const float*>(k.vol[c]);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = vol[off[q]];
    } else {
      const short* vol = static_cast<const short*>(k.vol[c]);
      short raw[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) raw[q] = vol[off[q]];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (float)raw[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = (valid >> q) & 1u ? v[q] : outside;
    const float c00 = lerp_rn(v[0], v[1], t[2]), c01 = lerp_rn(v[2], v[3], t[2]);
    const float c10 = lerp_rn(v[4], v[5], t[2]), c11 = lerp_rn(v[6], v[7], t[2]);
    float g = lerp_rn(lerp_rn(c00, c01, t[1]), lerp_rn(c10, c11, t[1]), t[0]);
    if constexpr (INT) {
      float n = clip_unit(g, k.divisor[c], k.lo[c], k.hi[c], __fsub_rn(k.hi[c], k.lo[c]));
      n = intensity_chain(n, k.it[c], beta, i, c);
      g = __fsub_rn(__fmul_rn(2.f, n), 1.f);
    } else if constexpr (CLIP) {
      g = clip_minmax(g, k.divisor[c], k.lo[c], k.hi[c], __fsub_rn(k.hi[c], k.lo[c]));
    }
    out[(long long)c * k.n + i] = g;
  }
}

// the intensity arguments of gs_patch_augment_clip_minmax, checked by the caller (check_intensity)
struct IntArgs {
  const GsPatchIntensity* it;      // host, k.C entries
  const int32_t* grid;             // nullptr: no bias lattice
  const double* field;
};

// the one launch line of the gather: E and K come with the caller's form, `clip` picks CLIP; with `ia` the intensity
// variant of that form, its bias part in LDS behind the lds bytes of the elastic part
template <int E, typename K>
void launch_gather(const K& k, bool clip, dim3 g, size_t lds, hipStream_t st, float* out, const IntArgs* ia = nullptr,
                   int bform = ELA_NONE, size_t lds_bias = 0) {
  if (ia) {
    IntK<K> q;
    static_cast<K&>(q) = k;
    for (int c = 0; c < PC_MAX; ++c) q.it[c] = ia->it[c < k.C ? c : 0];
    q.beta = ia->field;
    for (int a = 0; a < 3; ++a) q.BG[a] = ia->grid ? ia->grid[a] : 4;
    q.bform = bform;
    q.boff = (int)(lds / sizeof(double));
    hipLaunchKernelGGL((patch_affine_kernel<true, E, IntK<K>, true>), g, dim3(256), lds + lds_bias, st, q, out);
    return;
  }
  void (*kernel)(const K, float*) = clip ? patch_affine_kernel<true, E, K> : patch_affine_kernel<false, E, K>;
  hipLaunchKernelGGL(kernel, g, dim3(256), lds, st, k, out);
}

// grid (nullptr: no elastic part) and field: the lattice of gs_patch_elastic*, checked by the caller
int launch_affine(AffK& k, const int32_t* patch, const double* M, const int32_t* grid, const double* field, float* out,
                  bool clip, void* stream, const IntArgs* ia = nullptr) {
  for (int j = 0; j < 9; ++j) k.M[j] = M[j];
  k.pd = patch[0]; k.ph = patch[1]; k.pw = patch[2];
  k.n = (long long)patch[0] * patch[1] * patch[2];
  const long long blocks = (k.n + 255) / 256;            // one voxel per thread
  GS_REQUIRE(blocks <= 0x7fffffffLL, "gs_patch_affine: %lld voxels do not fit one grid", k.n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g((unsigned)blocks);
  // one form for both lattices: the row tables when together they fit the option, else both staged whole
  const int32_t* bg = ia ? ia->grid : nullptr;
  const long long rows_all = (long long)patch[0] * patch[1], rows_wg = 255 / patch[2] + 2;
  const size_t rows = (size_t)(rows_all < rows_wg ? rows_all : rows_wg);
  const size_t table = grid ? rows * 3 * grid[2] * sizeof(double) : 0;
  const size_t table_bias = bg ? rows * bg[2] * sizeof(double) : 0;
  int fits = gs_opt(GS_OPT_ELASTIC_ROWS);
  fits = fits < 0 ? 0 : (fits > 65536 ? 65536 : fits);
  const bool by_rows = table + table_bias <= (size_t)fits;
  const int bform = !bg ? ELA_NONE : (by_rows ? ELA_ROWS : ELA_VOXEL);
  const size_t lds_bias = !bg ? 0 : (by_rows ? table_bias : (size_t)bg[0] * bg[1] * bg[2] * sizeof(double));
  if (!grid) {
    launch_gather<ELA_NONE>(k, clip, g, 0, st, out, ia, bform, lds_bias);
  } else {
    ElaK e;
    static_cast<AffK&>(e) = k;
    e.field = field;
    e.G[0] = grid[0]; e.G[1] = grid[1]; e.G[2] = grid[2];
    if (by_rows) launch_gather<ELA_ROWS>(e, clip, g, table, st, out, ia, bform, lds_bias);
    else launch_gather<ELA_VOXEL>(e, clip, g, (size_t)3 * grid[0] * grid[1] * grid[2] * sizeof(double), st, out, ia, bform,
                                  lds_bias);
  }
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

// what the elastic entries refuse on top of the affine ones
int check_lattice(const char* who, const int32_t* patch, const int32_t* grid, const double* field) {
  GS_REQUIRE(grid && field, "%s: null grid or field", who);
  GS_REQUIRE(grid[0] >= 4 && grid[1] >= 4 && grid[2] >= 4, "%s: the lattice needs at least 4 control points per axis; got %d x %d x %d",
             who, grid[0], grid[1], grid[2]);
  GS_REQUIRE((long long)grid[0] * grid[1] * grid[2] <= GS_ELASTIC_MAX_POINTS,
             "%s: a lattice of %d x %d x %d control points exceeds %d", who, grid[0], grid[1], grid[2], GS_ELASTIC_MAX_POINTS);
  GS_REQUIRE(patch[0] >= 2 && patch[1] >= 2 && patch[2] >= 2, "%s: an elastic patch needs at least 2 voxels per axis; got %d x %d x %d",
             who, patch[0], patch[1], patch[2]);
  for (int a = 0; a < 3; ++a)
    GS_REQUIRE((long long)(patch[a] - 1) * (grid[a] - 3) <= 0x7fffffffLL, "%s: patch axis %d of %d voxels is too long for %d "
               "control points", who, a, patch[a], grid[a]);
  return 0;
}

inline bool finite9(const double* M) {
  for (int j = 0; j < 9; ++j)
    if (!(M[j] - M[j] == 0.0)) return false;             // inf - inf and NaN - NaN are NaN
  return true;
}

// ---- gs_volume_prepare ---------------------------------------------------------------------------------------------
constexpr int VP_MAX_MASKS = 1 + GS_VM_MAX_LABELS;
constexpr int VP_PARTS = 256;              // workgroups of the minimum pass per volume / mask

struct PrepK : ModTable {
  const uint8_t* mask[VP_MAX_MASKS];
  uint8_t* mask_out[VP_MAX_MASKS];
  int C, M;
  int D, H, W, Do, Ho, Wo, pz, py, px;     // input size, output size, pad in front
  long long n, no;
  int padded;
};

// np.min's rule: a NaN anywhere makes the minimum NaN
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? a + b : (b < a ? b : a); }

// partial[item * VP_PARTS + block]: item < C the minimum of where(body, v, outside) over the block's voxels, item >= C the
// minimum byte of mask item - C; a block without voxels contributes +inf
__global__ __launch_bounds__(256) void prepare_min_kernel(const PrepK k, float* partial) {
  __shared__ float s[256];
  const int item = blockIdx.y;
  float m = std::numeric_limits<float>::infinity();
  if (item < k.C) {
    const void* vol = k.vol[item];
    const int dtype = k.dtype[item];
    const float outside = k.outside[item];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < k.n; i += (long long)VP_PARTS * 256)
      m = min_nan(m, voxel_or(vol, dtype, i, k.mask[0][i] != 0, outside));
  } else {
    const uint8_t* mask = k.mask[item - k.C];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < k.n; i += (long long)VP_PARTS * 256)
      m = min_nan(m, (float)mask[i]);
  }
  s[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] = min_nan(s[threadIdx.x], s[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[item * VP_PARTS + blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void prepare_apply_kernel(const PrepK k, const float* partial, float* out) {
  __shared__ float s[256];
  const int item = blockIdx.y;
  float fill = 0.f;
  if (k.padded) {                          // every workgroup folds the VP_PARTS partials of its item in the same order
    s[threadIdx.x] = partial[item * VP_PARTS + threadIdx.x];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) s[threadIdx.x] = min_nan(s[threadIdx.x], s[threadIdx.x + o]);
      __syncthreads();
    }
    fill = s[0];
  }
  const bool image = item < k.C;
  const int c = image ? item : 0, mi = image ? 0 : item - k.C;
  const void* vol = k.vol[c];
  const int dtype = k.dtype[c];
  const float outside = k.outside[c], divisor = k.divisor[c], lo = k.lo[c], hi = k.hi[c];
  const float span = __fsub_rn(hi, lo);
  const uint8_t* body = k.mask[0];
  const uint8_t* msrc = k.mask[mi];
  float* dst = out + (long long)c * k.no;
  uint8_t* mdst = k.mask_out[mi];
  const uint8_t mfill = (uint8_t)fill;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < k.no; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % k.Wo) - k.px;
    const long long row = i / k.Wo;
    const int y = (int)(row % k.Ho) - k.py, z = (int)(row / k.Ho) - k.pz;
    const bool in = (unsigned)x < (unsigned)k.W && (unsigned)y < (unsigned)k.H && (unsigned)z < (unsigned)k.D;
    const long long off = ((long long)z * k.H + y) * k.W + x;
    if (image) {
      const float v = in ? voxel_or(vol, dtype, off, body[off] != 0, outside) : fill;
      dst[i] = clip_minmax(v, divisor, lo, hi, span);
    } else {
      mdst[i] = in ? msrc[off] : mfill;
    }
  }
}
}  // namespace

extern "C" int64_t gs_voxel_draw_ws_bytes(void) { return (int64_t)(2 * NR) * 8 + 16; }

extern "C" int64_t gs_voxel_draw_range_len(int32_t D, int32_t H, int32_t W, const int32_t* patch) {
  if (!patch) return 0;
  return range_len(D, H, W, patch);
}

extern "C" int gs_voxel_draw(const uint8_t* mask, const void* weight, int32_t wdtype, int32_t D, int32_t H, int32_t W,
                             const int32_t* patch, double u, const int32_t* focal_a, const int32_t* dims_a,
                             const double* proportion, int32_t* out, void* ws, void* stream) {
  GS_REQUIRE(mask && patch && out && ws, "gs_voxel_draw: null argument");
  GS_REQUIRE(!weight || wdtype == GS_VOL_F32 || wdtype == GS_VOL_I16,
             "gs_voxel_draw: weight dtype %d (GS_VOL_F32 / GS_VOL_I16)", wdtype);
  if (const int rc = check_patch_fits("gs_voxel_draw", D, H, W, patch)) return rc;
  GS_REQUIRE(u >= 0.0 && u < 1.0, "gs_voxel_draw: u = %.17g is not in [0, 1)", u);
  GS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gs_voxel_draw: the workspace must be 8-byte aligned");
  GS_REQUIRE(!focal_a || (dims_a && proportion), "gs_voxel_draw: a focal point needs A's dims and the proportions");
  DrawK k;
  k.mask = mask;
  k.weight = weight;
  k.D = D; k.H = H; k.W = W;
  k.z0 = zone_lo(patch[0]); k.y0 = zone_lo(patch[1]); k.x0 = zone_lo(patch[2]);
  k.bd = zone_hi(D, patch[0]) - k.z0; k.bh = zone_hi(H, patch[1]) - k.y0; k.bw = zone_hi(W, patch[2]) - k.x0;
  if (k.bd <= 0 || k.bh <= 0 || k.bw <= 0) { k.bd = k.bh = k.bw = 0; }      // empty zone: every partial is 0, out = -1
  k.n = (long long)k.bd * k.bh * k.bw;
  k.L = (k.n + NR - 1) / NR;
  k.S = (k.L + NT - 1) / NT;
  if (k.bw == 0) k.bw = k.bh = 1;                                            // never divided by: n == 0 walks nothing
  k.u = u;
  k.focal_a = focal_a;
  const int size[3] = {D, H, W};
  for (int a = 0; a < 3; ++a) {
    k.da[a] = 1;
    k.region[a] = 0;
    if (focal_a) {
      GS_REQUIRE(dims_a[a] > 0 && proportion[a] >= 0.0 && proportion[a] <= 1.0,
                 "gs_voxel_draw: A's dims must be positive and the focal region proportions in [0, 1]");
      k.da[a] = dims_a[a];
      k.region[a] = (int)(proportion[a] * (double)size[a]);                 // one rounding, then truncation
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!weight) return launch_draw<void>(k, out, ws, st);
  return wdtype == GS_VOL_F32 ? launch_draw<float>(k, out, ws, st) : launch_draw<short>(k, out, ws, st);
}

extern "C" int gs_patch_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask,
                                    int32_t D, int32_t H, int32_t W, const int32_t* patch, const int32_t* point,
                                    const float* outside, const float* divisor, const float* lo, const float* hi, float* out,
                                    void* stream) {
  GS_REQUIRE(vols && dtypes && mask && patch && point && outside && divisor && lo && hi && out,
             "gs_patch_clip_minmax: null argument");
  GS_REQUIRE(C >= 1 && C <= PC_MAX, "gs_patch_clip_minmax: between 1 and %d modalities per call; got %d", PC_MAX, C);
  if (const int rc = check_patch_fits("gs_patch_clip_minmax", D, H, W, patch)) return rc;
  ClipK k;
  if (const int rc = fill_table("gs_patch_clip_minmax", k, vols, dtypes, outside, divisor, lo, hi, C)) return rc;
  k.mask = mask;
  k.point = point;
  k.D = D; k.H = H; k.W = W;
  k.pd = patch[0]; k.ph = patch[1]; k.pw = patch[2];
  k.n = (long long)patch[0] * patch[1] * patch[2];
  const long long blocks = (k.n + 256 * 4 - 1) / (256 * 4);
  hipLaunchKernelGGL(patch_clip_minmax_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)C), dim3(256), 0,
                     static_cast<hipStream_t>(stream), k, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}

namespace {
// the bodies of the affine and the elastic entry points: grid == nullptr is the affine one, `who` names the entry in messages
int gather_clip_minmax(const char* who, const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask,
                       int32_t D, int32_t H, int32_t W, const int32_t* point, const int32_t* patch, const double* M,
                       const int32_t* grid, const double* field, const float* outside, const float* divisor, const float* lo,
                       const float* hi, float* out, void* stream, const IntArgs* ia = nullptr) {
  GS_REQUIRE(vols && dtypes && mask && point && patch && M && outside && divisor && lo && hi && out, "%s: null argument", who);
  GS_REQUIRE(C >= 1 && C <= PC_MAX, "%s: between 1 and %d modalities per call; got %d", who, PC_MAX, C);
  if (const int rc = check_patch_fits(who, D, H, W, patch)) return rc;
  GS_REQUIRE(finite9(M), "%s: the matrix has a non-finite entry", who);
  AffK k;
  if (const int rc = fill_table(who, k, vols, dtypes, outside, divisor, lo, hi, C)) return rc;
  k.mask = mask;
  k.point = point;
  k.start[0] = k.start[1] = k.start[2] = 0;
  k.C = C; k.D = D; k.H = H; k.W = W;
  return launch_affine(k, patch, M, grid, field, out, true, stream, ia);
}

int gather_raw(const char* who, const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
               const int32_t* size, const double* M, const int32_t* grid, const double* field, float fill, float* out,
               void* stream) {
  GS_REQUIRE(vol && start && size && M && out, "%s: null argument", who);
  GS_REQUIRE(dtype == GS_VOL_F32 || dtype == GS_VOL_I16, "%s: dtype %d (GS_VOL_F32 / GS_VOL_I16)", who, dtype);
  if (const int rc = check_patch_fits(who, D, H, W, size)) return rc;
  GS_REQUIRE(start[0] >= 0 && start[1] >= 0 && start[2] >= 0 && start[0] <= D - size[0] && start[1] <= H - size[1] &&
                 start[2] <= W - size[2],
             "%s: patch [%d+%d, %d+%d, %d+%d] outside the %d x %d x %d volume", who, start[0], size[0], start[1], size[1],
             start[2], size[2], D, H, W);
  GS_REQUIRE(finite9(M), "%s: the matrix has a non-finite entry", who);
  AffK k;
  for (int c = 0; c < PC_MAX; ++c) {
    k.vol[c] = vol;
    k.dtype[c] = dtype;
    k.outside[c] = fill; k.divisor[c] = 1.f; k.lo[c] = 0.f; k.hi[c] = 1.f;
  }
  k.mask = nullptr;
  k.point = nullptr;
  k.start[0] = start[0]; k.start[1] = start[1]; k.start[2] = start[2];
  k.C = 1; k.D = D; k.H = H; k.W = W;
  return launch_affine(k, size, M, grid, field, out, false, stream);
}
}  // namespace

extern "C" int gs_patch_affine_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask,
                                           int32_t D, int32_t H, int32_t W, const int32_t* point, const int32_t* patch,
                                           const double* M, const float* outside, const float* divisor, const float* lo,
                                           const float* hi, float* out, void* stream) {
  return gather_clip_minmax("gs_patch_affine_clip_minmax", vols, dtypes, C, mask, D, H, W, point, patch, M, nullptr, nullptr,
                            outside, divisor, lo, hi, out, stream);
}

extern "C" int gs_patch_affine(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                               const int32_t* size, const double* M, float fill, float* out, void* stream) {
  return gather_raw("gs_patch_affine", vol, dtype, D, H, W, start, size, M, nullptr, nullptr, fill, out, stream);
}

extern "C" int gs_patch_elastic_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask,
                                            int32_t D, int32_t H, int32_t W, const int32_t* point, const int32_t* patch,
                                            const double* M, const int32_t* grid, const double* field, const float* outside,
                                            const float* divisor, const float* lo, const float* hi, float* out, void* stream) {
  GS_REQUIRE(patch, "gs_patch_elastic_clip_minmax: null argument");
  if (const int rc = check_lattice("gs_patch_elastic_clip_minmax", patch, grid, field)) return rc;
  return gather_clip_minmax("gs_patch_elastic_clip_minmax", vols, dtypes, C, mask, D, H, W, point, patch, M, grid, field,
                            outside, divisor, lo, hi, out, stream);
}

extern "C" int gs_patch_elastic(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                                const int32_t* size, const double* M, const int32_t* grid, const double* field, float fill,
                                float* out, void* stream) {
  GS_REQUIRE(size, "gs_patch_elastic: null argument");
  if (const int rc = check_lattice("gs_patch_elastic", size, grid, field)) return rc;
  return gather_raw("gs_patch_elastic", vol, dtype, D, H, W, start, size, M, grid, field, fill, out, stream);
}

extern "C" int gs_patch_augment_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask,
                                            int32_t D, int32_t H, int32_t W, const int32_t* point, const int32_t* patch,
                                            const double* M, const int32_t* grid, const double* field,
                                            const GsPatchIntensity* intensity, const int32_t* bias_grid,
                                            const double* bias_field, const float* outside, const float* divisor,
                                            const float* lo, const float* hi, float* out, void* stream) {
  const char* who = "gs_patch_augment_clip_minmax";
  GS_REQUIRE(patch, "%s: null argument", who);
  GS_REQUIRE(C >= 1 && C <= PC_MAX, "%s: between 1 and %d modalities per call; got %d", who, PC_MAX, C);
  GS_REQUIRE((grid != nullptr) == (field != nullptr), "%s: grid and field come together", who);
  if (grid)
    if (const int rc = check_lattice(who, patch, grid, field)) return rc;
  bool lattice;
  if (const int rc = check_intensity(who, intensity, C, patch, bias_grid, bias_field, &lattice)) return rc;
  const IntArgs ia = {intensity, bias_grid, bias_field};
  return gather_clip_minmax(who, vols, dtypes, C, mask, D, H, W, point, patch, M, grid, field, outside, divisor, lo, hi, out,
                            stream, &ia);
}

extern "C" int64_t gs_volume_prepare_ws_bytes(void) { return (int64_t)(PC_MAX + VP_MAX_MASKS) * VP_PARTS * 4; }

extern "C" int gs_volume_prepare(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* const* masks,
                                 int32_t M, int32_t D, int32_t H, int32_t W, const int32_t* target, const float* outside,
                                 const float* divisor, const float* lo, const float* hi, float* out,
                                 uint8_t* const* masks_out, void* ws, void* stream) {
  GS_REQUIRE(vols && dtypes && masks && target && outside && divisor && lo && hi && out && masks_out && ws,
             "gs_volume_prepare: null argument");
  GS_REQUIRE(C >= 1 && C <= PC_MAX, "gs_volume_prepare: between 1 and %d volumes per call; got %d", PC_MAX, C);
  GS_REQUIRE(M >= 1 && M <= VP_MAX_MASKS, "gs_volume_prepare: between 1 and %d masks per call (the body mask first); got %d",
             VP_MAX_MASKS, M);
  GS_REQUIRE(D > 0 && H > 0 && W > 0 && target[0] > 0 && target[1] > 0 && target[2] > 0,
             "gs_volume_prepare: volume %d x %d x %d, target %d x %d x %d", D, H, W, target[0], target[1], target[2]);
  GS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "gs_volume_prepare: the workspace must be 4-byte aligned");
  PrepK k;
  if (const int rc = fill_table("gs_volume_prepare", k, vols, dtypes, outside, divisor, lo, hi, C)) return rc;
  for (int m = 0; m < VP_MAX_MASKS; ++m) {
    const int s = m < M ? m : 0;
    GS_REQUIRE(masks[s] && masks_out[s], "gs_volume_prepare: null mask %d", s);
    k.mask[m] = masks[s];
    k.mask_out[m] = masks_out[s];
  }
  k.C = C; k.M = M;
  k.D = D; k.H = H; k.W = W;
  k.Do = target[0] > D ? target[0] : D; k.Ho = target[1] > H ? target[1] : H; k.Wo = target[2] > W ? target[2] : W;
  k.pz = (k.Do - D) / 2; k.py = (k.Ho - H) / 2; k.px = (k.Wo - W) / 2;
  k.n = (long long)D * H * W;
  k.no = (long long)k.Do * k.Ho * k.Wo;
  k.padded = k.no != k.n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(ws);
  if (k.padded)
    hipLaunchKernelGGL(prepare_min_kernel, dim3(VP_PARTS, (unsigned)(C + M)), dim3(256), 0, st, k, partial);
  const long long blocks = (k.no + 256 * 4 - 1) / (256 * 4);
  hipLaunchKernelGGL(prepare_apply_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks), (unsigned)(C + M)), dim3(256), 0,
                     st, k, partial, out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
