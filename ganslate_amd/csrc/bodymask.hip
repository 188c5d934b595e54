// Patient body mask from a CT on the device (data/utils/body_mask.py states the definition; ganslate_hip.h repeats it as
// the contract of gs_body_mask): threshold, largest 6-connected component (ties: the one whose first voxel in C order comes
// first), per-slice hole filling. The reference (ganslate/data/utils/body_mask.py) runs scipy.ndimage.label and
// binary_fill_holes on the host, seconds per 512 x 512 x ~100 case; its OpenCV contour smoothing is not part of the
// definition here.
//
// ONE labelling routine, used twice: in 3-D with 6 neighbours on b = (v >= t), then per slice with 4 neighbours on the
// complement of the chosen component (a complement component that owns a pixel of the slice's border is "outside").
// State: parent[i] for every voxel of the set, with the invariants  parent[i] <= i  and  parent[i] lies in i's component.
// A ROUND is two launches:
//   hook     every voxel reads its own parent r (a root after the previous flatten) and its neighbours' parents; if the
//            smallest of them, m, is below r:  atomic_min(parent[r], m)  and the round is marked as not quiet
//   flatten  every voxel walks parent[] down to a root (strictly decreasing indices, so the walk is bounded by the data)
//            and stores that root as its parent
// Both invariants survive every interleaving: a hook only ever lowers a parent to a member of the same component, and
// flatten replaces a parent by one of its ancestors. A round is quiet only if no hook fired, i.e. all adjacent voxels read
// equal parents while nothing was being written; parent is then constant on every component, and by the invariants that
// constant is the component's smallest index — its first voxel in C order, whatever happened before. So the RESULT does
// not depend on which values the racing reads of earlier rounds returned; only the number of rounds does. Within a launch
// every access to parent[] is an agent-scope atomic (the XCDs' L2s are not coherent for plain accesses inside a launch);
// everything else a launch reads was written by an earlier launch.
// Hooking ROOTS (union-find style) instead of spreading labels voxel to voxel is what keeps the number of rounds from
// growing with the length of a thin path: every round merges each tree with at least one neighbouring tree and the
// flatten collapses the chains of roots that result; a serpentine of 23 000 voxels takes a handful of rounds.
// Rounds are enqueued ROUNDS_PER_SYNC at a time; rounds behind a quiet one return at once; the host then reads the last
// flag of the batch back (one stream synchronisation per batch, a few per case).
// Sizes: integer atomic adds on the roots. Argmax: per-workgroup maxima of the 64-bit key (count << 32 | ~root), a fixed
// tree in LDS, then one workgroup over the partial maxima — integers, so the order cannot change the result anyway.
#include "common.hpp"

namespace {
constexpr int NT = 256;
constexpr int ROUNDS_PER_SYNC = 8;
constexpr int NPART = 1024;                  // workgroups of the argmax's first level
constexpr int HDR_INTS = 16;                 // [0], [1]: rounds of the two phases; [2 .. 2 + ROUNDS_PER_SYNC): "hook fired" flags
constexpr int MAX_BLOCKS = 1 << 16;

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct Dims {
  int D, H, W;
  long long n;
};

template <typename T>
__global__ __launch_bounds__(NT) void threshold_kernel(const T* vol, Dims d, float thr, uint8_t* fg, int* parent, int* cnt) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    const bool in = (float)vol[i] >= thr;                  // NaN: false
    fg[i] = in;
    parent[i] = in ? (int)i : -1;
    cnt[i] = 0;
  }
}

// planar != 0: the 4 neighbours inside the depth slice only
__global__ __launch_bounds__(NT) void hook_kernel(const uint8_t* fg, int* parent, Dims d, int planar, int* hdr, int r,
                                                  int phase) {
  int* flags = hdr + 2;
  if (r > 0 && flags[r - 1] == 0) return;                  // the previous round was quiet (uniform over the grid)
  const long long plane = (long long)d.H * d.W;
  int fired = 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    if (!fg[i]) continue;
    const int x = (int)(i % d.W);
    const long long row = i / d.W;
    const int y = (int)(row % d.H), z = (int)(row / d.H);
    const int own = ld(parent + i);
    int m = own;
    if (x > 0 && fg[i - 1]) m = min(m, ld(parent + i - 1));
    if (x + 1 < d.W && fg[i + 1]) m = min(m, ld(parent + i + 1));
    if (y > 0 && fg[i - d.W]) m = min(m, ld(parent + i - d.W));
    if (y + 1 < d.H && fg[i + d.W]) m = min(m, ld(parent + i + d.W));
    if (!planar) {
      if (z > 0 && fg[i - plane]) m = min(m, ld(parent + i - plane));
      if (z + 1 < d.D && fg[i + plane]) m = min(m, ld(parent + i + plane));
    }
    if (m < own) {
      __hip_atomic_fetch_min(parent + own, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      fired = 1;
    }
  }
  fired = __syncthreads_or(fired);
  if (threadIdx.x == 0) {
    if (fired) st(flags + r, 1);
    if (blockIdx.x == 0) hdr[phase] += 1;                  // one thread of the whole launch; launches are ordered
  }
}

__global__ __launch_bounds__(NT) void flatten_kernel(const uint8_t* fg, int* parent, Dims d, const int* hdr, int r) {
  if (hdr[2 + r] == 0) return;                             // no hook fired: parent[] is flat already
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    if (!fg[i]) continue;
    int p = ld(parent + i);
    for (int q = ld(parent + p); q != p; q = ld(parent + p)) p = q;      // q < p at every step
    st(parent + i, p);
  }
}

__global__ __launch_bounds__(NT) void count_kernel(const uint8_t* fg, const int* parent, Dims d, int* cnt) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT)
    if (fg[i]) atomicAdd(cnt + parent[i], 1);
}

__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o && s[threadIdx.x + o] > s[threadIdx.x]) s[threadIdx.x] = s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}

// key of a root: more voxels first, then the lower index
__global__ __launch_bounds__(NT) void argmax_partial_kernel(const uint8_t* fg, const int* parent, const int* cnt, Dims d,
                                                            unsigned long long* part) {
  __shared__ unsigned long long s[NT];
  unsigned long long best = 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    if (!fg[i] || parent[i] != (int)i) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)cnt[i] << 32) | (unsigned)(0x7fffffff - (int)i);
    best = key > best ? key : best;
  }
  best = block_max(best, s);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ __launch_bounds__(NT) void argmax_final_kernel(const unsigned long long* part, int nparts, int* info) {
  __shared__ unsigned long long s[NT];
  unsigned long long best = 0;
  for (int i = threadIdx.x; i < nparts; i += NT) best = part[i] > best ? part[i] : best;
  best = block_max(best, s);
  if (threadIdx.x == 0) {
    const int count = (int)(best >> 32);
    info[0] = count;
    info[1] = count > 0 ? 0x7fffffff - (int)(best & 0xffffffffu) : -1;
  }
}

// the set of the second phase: every voxel that is not of the chosen component
__global__ __launch_bounds__(NT) void complement_kernel(uint8_t* fg, int* parent, int* cnt, Dims d, const int* info) {
  const int root = info[1];
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    const bool out = !(fg[i] && parent[i] == root);
    fg[i] = out;
    parent[i] = out ? (int)i : -1;
    cnt[i] = 0;
  }
}

// cnt[root] = 1 for every complement component with a pixel on its slice's border
__global__ __launch_bounds__(NT) void border_kernel(const uint8_t* fg, const int* parent, int* cnt, Dims d) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT) {
    if (!fg[i]) continue;
    const int x = (int)(i % d.W), y = (int)((i / d.W) % d.H);
    if (x == 0 || y == 0 || x == d.W - 1 || y == d.H - 1) st(cnt + parent[i], 1);
  }
}

__global__ __launch_bounds__(NT) void fill_kernel(const uint8_t* fg, const int* parent, const int* cnt, Dims d, uint8_t* mask) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < d.n; i += (long long)gridDim.x * NT)
    mask[i] = fg[i] ? (cnt[parent[i]] ? 0 : 1) : 1;
}

struct Ws {
  int* hdr;
  unsigned long long* part;
  int* parent;
  int* cnt;
  uint8_t* fg;
};

inline long long ws_bytes(long long n) {
  return ((long long)HDR_INTS * 4 + (long long)NPART * 8 + n * 9 + 7) / 8 * 8;
}

// rounds until a quiet one; returns a HIP error or 0
int label(const Ws& w, const Dims& d, int planar, int phase, unsigned blocks, hipStream_t st) {
  const long long max_batches = d.n / ROUNDS_PER_SYNC + 2;                  // every round but the last lowers a parent
  for (long long batch = 0; batch < max_batches; ++batch) {
    GS_CHECK_HIP(hipMemsetAsync(w.hdr + 2, 0, ROUNDS_PER_SYNC * sizeof(int), st));
    for (int r = 0; r < ROUNDS_PER_SYNC; ++r) {
      hipLaunchKernelGGL(hook_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, d, planar, w.hdr, r, phase);
      hipLaunchKernelGGL(flatten_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, d, w.hdr, r);
    }
    GS_CHECK_HIP(hipGetLastError());
    int last = 0;
    GS_CHECK_HIP(hipMemcpyAsync(&last, w.hdr + 2 + ROUNDS_PER_SYNC - 1, sizeof(int), hipMemcpyDeviceToHost, st));
    GS_CHECK_HIP(hipStreamSynchronize(st));
    if (!last) return 0;
  }
  gs_set_error("gs_body_mask: labelling did not settle");
  return 1;
}
}  // namespace

extern "C" int64_t gs_body_mask_ws_bytes(int32_t D, int32_t H, int32_t W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  return ws_bytes((long long)D * H * W);
}

// Round form with a device "hook fired" flag per round: ROUNDS_PER_SYNC rounds per batch, one read-back and stream
// synchronisation per batch (the header comment of this file has the argument for exactness).
extern "C" int gs_body_mask(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, float threshold,
                            uint8_t* mask_out, int32_t* info, void* ws, void* stream) {
  GS_REQUIRE(vol && mask_out && info && ws, "gs_body_mask: null argument");
  GS_REQUIRE(dtype == GS_VOL_F32 || dtype == GS_VOL_I16, "gs_body_mask: dtype %d (GS_VOL_F32 / GS_VOL_I16)", dtype);
  GS_REQUIRE(D > 0 && H > 0 && W > 0, "gs_body_mask: volume %d x %d x %d", D, H, W);
  GS_REQUIRE((long long)D * H * W < (1ll << 31), "gs_body_mask: %d x %d x %d voxels do not fit 31-bit indices", D, H, W);
  GS_REQUIRE(threshold == threshold, "gs_body_mask: the threshold is NaN");
  GS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gs_body_mask: the workspace must be 8-byte aligned");
  Dims d{D, H, W, (long long)D * H * W};
  Ws w;
  w.hdr = static_cast<int*>(ws);
  w.part = reinterpret_cast<unsigned long long*>(w.hdr + HDR_INTS);
  w.parent = reinterpret_cast<int*>(w.part + NPART);
  w.cnt = w.parent + d.n;
  w.fg = reinterpret_cast<uint8_t*>(w.cnt + d.n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long want = (d.n + NT - 1) / NT;
  const unsigned blocks = (unsigned)(want > MAX_BLOCKS ? MAX_BLOCKS : want);
  const int nparts = (int)(want > NPART ? NPART : want);

  GS_CHECK_HIP(hipMemsetAsync(w.hdr, 0, HDR_INTS * sizeof(int), st));
  if (dtype == GS_VOL_F32)
    hipLaunchKernelGGL(threshold_kernel<float>, dim3(blocks), dim3(NT), 0, st, static_cast<const float*>(vol), d, threshold,
                       w.fg, w.parent, w.cnt);
  else
    hipLaunchKernelGGL(threshold_kernel<short>, dim3(blocks), dim3(NT), 0, st, static_cast<const short*>(vol), d, threshold,
                       w.fg, w.parent, w.cnt);
  if (int e = label(w, d, 0, 0, blocks, st)) return e;
  hipLaunchKernelGGL(count_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, d, w.cnt);
  hipLaunchKernelGGL(argmax_partial_kernel, dim3(nparts), dim3(NT), 0, st, w.fg, w.parent, w.cnt, d, w.part);
  hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(NT), 0, st, w.part, nparts, info);
  hipLaunchKernelGGL(complement_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, w.cnt, d, info);
  if (int e = label(w, d, 1, 1, blocks, st)) return e;
  hipLaunchKernelGGL(border_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, w.cnt, d);
  hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(NT), 0, st, w.fg, w.parent, w.cnt, d, mask_out);
  GS_CHECK_HIP(hipGetLastError());
  return 0;
}
