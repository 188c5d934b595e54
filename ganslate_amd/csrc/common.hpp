// Shared device helpers for the gfx950 kernels of libganslate_hip.so.
// Wave = 64 lanes everywhere; fragment layouts pinned by tools/probe/probe.hip (profiles/r01_hw_probe.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/ganslate_hip.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

#define GS_LDS(p) ((__attribute__((address_space(3))) void*)(p))
#define GS_GLB(p) ((const __attribute__((address_space(1))) void*)(p))

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// two fp32 -> packed bf16x2 (round-to-nearest-even, v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf2(float a, float b) {
  f32x2 v = {a, b};
  bf16x2_t r = __builtin_convertvector(v, bf16x2_t);
  return *reinterpret_cast<unsigned*>(&r);
}
__device__ __forceinline__ unsigned short f2bf(float a) { return (unsigned short)(pack_bf2(a, 0.f) & 0xffffu); }
// 16 bytes = 8 bf16 channels <-> eight floats
__device__ __forceinline__ void unpack_bf8(float* f, const uint4 v) {
  f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
  f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}
__device__ __forceinline__ void add_bf8(float* f, const uint4 v) {
  f[0] += bf_lo(v.x); f[1] += bf_hi(v.x); f[2] += bf_lo(v.y); f[3] += bf_hi(v.y);
  f[4] += bf_lo(v.z); f[5] += bf_hi(v.z); f[6] += bf_lo(v.w); f[7] += bf_hi(v.w);
}
__device__ __forceinline__ uint4 pack_bf8(const float* f) {
  uint4 o;
  o.x = pack_bf2(f[0], f[1]); o.y = pack_bf2(f[2], f[3]); o.z = pack_bf2(f[4], f[5]); o.w = pack_bf2(f[6], f[7]);
  return o;
}
// the Cp (a multiple of 8) bf16 lanes of one pixel at px (16-byte aligned) from value(c), eight lanes per 16-byte store
template <class F>
__device__ __forceinline__ void store_bf_lanes(unsigned short* px, int Cp, F&& value) {
  for (int c0 = 0; c0 < Cp; c0 += 8) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = value(c0 + k);
    *reinterpret_cast<uint4*>(px + c0) = pack_bf8(f);
  }
}

// 16-byte LDS-DMA: LDS destination = wave-uniform base + lane*16; global source is per lane.
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(GS_GLB(gsrc), GS_LDS(lds_wave_base), 16, 0, 0);
}

// ---- LDS fragment reads the compiler does not count --------------------------------------------------------------
// With an LDS-DMA (global_load_lds) anywhere in a loop, hipcc (ROCm 7.2) no longer emits counted lgkmcnt(N) waits for
// ds_read results: every consumer waits lgkmcnt(0), i.e. also for the reads issued AFTER the ones it needs (the
// software-pipelined "issue the next fragments, then run the MFMAs on the current ones" degenerates into read - wait -
// MFMA; verified on a 20-line kernel: lgkmcnt(6)/(5)/(4) ladders without the DMA, lgkmcnt(0) with it). Reads issued
// through these statements are invisible to that bookkeeping; the kernel waits for them itself with gs_lgkm_wait<N>(...)
// naming every destination ("+v": no consumer can be scheduled above the wait, cdna_hip_programming.md §5.7 form (ii)).
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}
template <int OFF>
__device__ __forceinline__ void lds_read128(bf16x8& v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void gs_lgkm_wait(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d, bf16x8& e, bf16x8& f) {
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void gs_lgkm_wait(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d, bf16x8& e) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void gs_lgkm_wait(bf16x8& a, bf16x8& b, bf16x8& c, bf16x8& d, bf16x8& e, bf16x8& f,
                                             bf16x8& g, bf16x8& h) {
  asm volatile("s_waitcnt lgkmcnt(%8)"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : "i"(N) : "memory");
}

// wait-only statement + per-fragment register fences (any number of fragments): nothing that consumes x can be scheduled
// above reg_fence(x), and the fences follow the wait in program order (all are asm volatile)
template <int N>
__device__ __forceinline__ void gs_lgkm_wait_only() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(N) : "memory"); }
__device__ __forceinline__ void reg_fence(bf16x8& x) { asm volatile("" : "+v"(x)); }

// Workgroup barrier for data exchanged through LDS that does NOT drain the vector-memory counter: __syncthreads() carries
// a release fence, and with an LDS-DMA (or, in a persistent kernel, the previous tile's output stores) in flight that fence
// waits vmcnt(0). This one waits for this wave's LDS operations only; the "memory" clobbers keep the compiler from moving
// LDS accesses across it.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// 64-bit transpose read (pixel-major operands of the weight-gradient kernels): 4 bf16 of one k-column per lane
template <int OFF>
__device__ __forceinline__ void lds_read64_tr(uint2& v, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void gs_lgkm_wait64(uint2& a, uint2& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void gs_lgkm_wait64(uint2& a, uint2& b, uint2& c, uint2& d, uint2& e, uint2& f) {
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "i"(N) : "memory");
}
// per-fragment fence behind gs_lgkm_wait_only<N>() (any number of fragments, see reg_fence(bf16x8&) above)
__device__ __forceinline__ void reg_fence(uint2& lo, uint2& hi) { asm volatile("" : "+v"(lo), "+v"(hi)); }
// compile-time loop: f(std::integral_constant<int, I>{}) for I in [B, E)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// m / d for 0 <= m < 2^24 with rcp = 1.0f/d (exact after one fix-up step each way)
__device__ __forceinline__ int div_small(int m, int d, float rcp) {
  int q = (int)((float)m * rcp);
  int r = m - q * d;
  if (r < 0) { --q; } else if (r >= d) { ++q; }
  return q;
}

// branch-free border handling (mode is wave-uniform): returns the source index and clears `ok` for a
// zero-padded tap that falls outside [0, n)
__device__ __forceinline__ int border_index(int x, int n, int mode, bool& ok) {
  const bool inb = (unsigned)x < (unsigned)n;
  int xr = x < 0 ? -x : x;
  xr = xr >= n ? 2 * n - 2 - xr : xr;
  int xc = x < 0 ? 0 : x;
  xc = xc >= n ? n - 1 : xc;
  ok = ok & (inb | (mode != GS_BORDER_ZERO));
  return mode == GS_BORDER_REFLECT ? xr : (mode == GS_BORDER_REPLICATE ? xc : x);
}

// the adjoint of that padding along one axis: the positions, in coordinates padded by p, that the padding maps onto x
// (x + p itself first; reflect: <= 3 in all, replicate: a border cell and its p pad cells, p <= 3) -> their count
__device__ __forceinline__ int fold_sources(int* idx, int x, int n, int p, int mode) {
  int cnt = 1;
  idx[0] = x + p;
  if (p > 0) {
    if (mode == GS_BORDER_REFLECT) {
      if (x >= 1 && x <= p) idx[cnt++] = p - x;
      if (x >= n - 1 - p && x <= n - 2) idx[cnt++] = p + 2 * (n - 1) - x;
    } else if (mode == GS_BORDER_REPLICATE) {
      if (x == 0) for (int k = 0; k < p; ++k) idx[cnt++] = k;
      if (x == n - 1) for (int k = 1; k <= p; ++k) idx[cnt++] = n - 1 + p + k;
    }
  }
  return cnt;
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
  if (act == GS_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == GS_ACT_LRELU) return v > 0.f ? v : v * slope;
  if (act == GS_ACT_TANH) return tanhf(v);
  return v;
}
// The same with tanh as a CALL: inlined into an unrolled 64-128 element conv epilogue, tanhf's ~40 instructions per element
// (skipped at run time for the other activations, but fetched around and allocated for) made hstrip's tile code longer than
// the instruction cache and cost its kernels up to 127 registers (profiles/r04_hstrip_forms.txt).
static __device__ __noinline__ float gs_tanh_call(float v) { return tanhf(v); }
__device__ __forceinline__ float apply_act_small(float v, int act, float slope) {
  if (act == GS_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == GS_ACT_LRELU) return v > 0.f ? v : v * slope;
  if (act == GS_ACT_TANH) return gs_tanh_call(v);
  return v;
}
// derivative expressed through the activation OUTPUT o (valid for relu / lrelu with slope>0 / tanh)
__device__ __forceinline__ float act_grad_from_out(float o, int act, float slope) {
  if (act == GS_ACT_RELU) return o > 0.f ? 1.f : 0.f;
  if (act == GS_ACT_LRELU) return o > 0.f ? 1.f : slope;
  if (act == GS_ACT_TANH) return 1.f - o * o;
  return 1.f;
}

// dy of the InstanceNorm backward, dy = rstd * (ghat - mean ghat - yhat * mean(ghat * yhat)) with ghat = g * act'(yhat), from the
// pieces norm.hip's apply pass by channel group holds — with explicit roundings, so that no fma contraction decides the bits
__device__ __forceinline__ float inorm_dy(float g, float yh, float m, float s1, float s2, float rs) {
  const float gh = __fmul_rn(g, m);
  return __fmul_rn(rs, __fsub_rn(__fsub_rn(gh, s1), __fmul_rn(yh, s2)));
}

// ---- lane reductions on the DPP path -----------------------------------------------------------------------------
// __shfl_xor compiles to ds_bpermute_b32: an LDS instruction with ~100 cycles of latency per step. The statistics
// epilogue of the conv kernels ran 64 of them per wave in dependent chains of four (4.5 us of a 44 us launch, measured
// by leaving the statistics out). The same sums through DPP modifiers are plain VALU adds (v_add_f32_dpp).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row (lanes 16r .. 16r+15), result in all of them
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);    // row_half_mirror: quads 0<->1, 2<->3 (values are quad-uniform by now)
  v += dpp_mov<0x140>(v);    // row_mirror: halves of the row
  return v;
}
// v[i] + v[i ^ STEP] for lanes whose values are NOT uniform below STEP (lane i keeps its low bits): STEP = 4, 8 inside a
// row via rotations (ror:4 then ror:8 sums the 4 lanes with equal i mod 4; ror:8 alone the 2 with equal i mod 8)
__device__ __forceinline__ float row_sum_stride4(float v) { v += dpp_mov<0x124>(v); v += dpp_mov<0x128>(v); return v; }
__device__ __forceinline__ float row_sum_stride8(float v) { v += dpp_mov<0x128>(v); return v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// out = scale * the sum of n per-workgroup partials (float or double), by one workgroup of 256, in double: thread t takes
// t, t + 256, ... in index order, then a fixed tree over the threads. MAX_THREADS is the launch bound the code is generated
// for (1024 = none: SSIM's reducer never had one and keeps its code).
template <typename P, int MAX_THREADS>
__global__ __launch_bounds__(MAX_THREADS) void final_sum_kernel(const P* partial, int n, double scale, float* out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sh[0] * scale);
}

// ---- Adam (optim.hip; wgrad.hip's fused epilogue) ----------------------------------------------------------------------
// One element of the update; the same expression for the scalar tail and the four lanes of a 16-byte access.
__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, float b1, float b2, float eps,
                                         float bc2_sqrt, float step_size, float gscale, int zero_grad) {
  const float gi = g * gscale;
  const float mi = m + (gi - m) * (1.f - b1);                  // torch: exp_avg.lerp_(grad, 1-beta1)
  const float vi = v * b2 + (1.f - b2) * gi * gi;              // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = p - step_size * (mi / denom);
  m = mi;
  v = vi;
  if (zero_grad) g = 0.f;
}


// kernel-selection switches (set through gs_set_option, never read from the environment by the library).
// THE list: X(id suffix, option name, default), one row per option. enum GsOpt below and g_opts[] in api.hip are both
// generated from it, so an id and its name / default cannot drift apart; ganslate_amd/switches.py holds the same names
// with the environment variable that drives each (tests/test_abi_cpu.py compares the two sets).
#define GS_OPTIONS(X) \
  X(SPLITK, "splitk", 1)                       /* split-K for launches with few output tiles and a long K loop (gconv.hip) */ \
  X(SPLITK_MAX_BLOCKS, "splitk_max_blocks", 128) /* ... only below this many output tiles */ \
  X(SPLITK_TARGET, "splitk_target", 256)       /* ... aiming at this many workgroups */ \
  X(HCONV, "hconv", 1)                         /* halo-resident forward kernel for narrow stride-1 layers (hconv.hip) */ \
  X(HCONV_WIDE, "hconv_wide", 1)               /* halo-resident forward kernel for the wide 3x3 layers (hconvw.hip) */ \
  X(HWGRAD, "hwgrad", 1)                       /* halo-resident weight-gradient kernels (hwgrad.hip) */ \
  X(HWGRAD_WIDE, "hwgrad_wide", 1)             /* ... the wide 3x3 form */ \
  X(HWGRAD_PLANES, "hwgrad_planes", 1)         /* ... 3x3x3 layers as three depth planes of it */ \
  X(NORM_BWD_PPB, "norm_bwd_ppb", 0)           /* pixels per workgroup of the norm-backward reduction (0 = heuristic; tuning aid) */ \
  X(NORM_APPLY_UNROLL, "norm_apply_unroll", 4) /* elements per thread of the norm-backward apply pass (tuning aid) */ \
  X(GCONV_TILE288, "gconv_tile288", 1)         /* 288-pixel im2col tiles where they make exactly one round of workgroups (else 320) */ \
  X(GCONV_MULTI, "gconv_multi", 1)             /* the parity classes of a stride-2 transposed conv / data gradient as one launch */ \
  X(HCONVW_RING, "hconvw_ring", 1)             /* fused data gradient of the reflect-padded wide 3x3 layers on the unpadded domain (hconvw.hip RING) */ \
  X(HCONVT, "hconvt", 192)                     /* halo-resident kernel for the four parity classes of a stride-2 layer in one pass (hconvt.hip): */ \
                                               /* smallest grid (boxes x channel tiles x batch) it takes, 0 = off */ \
  X(HSTRIP, "hstrip", 1024)                    /* halo-resident kernel for the W-folded k7 boundary convs (hstrip.hip): smallest grid, 0 = off */ \
  X(WFOLD_ROWS, "wfold_rows", 1)               /* row-staged forms of the four W-fold boundary transforms (wfold.hip) instead of one thread per pixel */ \
  X(HWGRAD_FT, "hwgrad_ft", 1)                 /* halo-resident weight gradient of narrow layers with few taps (hwgrad.hip: the 2-D k7 boundary convs) */ \
  X(GCONV_BIG, "gconv_big", 192)               /* smallest number of 256 x 128 im2col tiles that selects them (one workgroup per CU) over 128 x 128 (two) */ \
  X(HCONV_BOX8, "hconv_box8", 1)               /* hconv.hip: 8 x 8 x 8 boxes on 8 waves for volumes (4 x 8 x 8 on 4 waves otherwise) */ \
  X(HCONVW_PERSIST, "hconvw_persist", 1)       /* hconvw.hip: launches with more tiles than CUs run ceil(tiles / CUs) tiles per workgroup (0: one each) */ \
  X(HSTRIP_REGS, "hstrip_regs", 1)             /* hstrip.hip: persistent form with the weights in registers for the k7 boundary convs (0: one tile per workgroup) */ \
  X(GCONV_TWIN, "gconv_twin", 1)               /* gconv.hip: twin batches on the im2col kernel as one launch (0: the two halves as two launches) */ \
  X(WGRAD_TWIN, "wgrad_twin", 1)               /* wgrad.hip: twin batches on the im2col weight-gradient kernel as one launch (0: two launches) */ \
  X(GCONV_PERSIST, "gconv_persist", 16)        /* pconv.hip: 256 x 128 im2col launches with more tiles than CUs and at most this many K-steps run as */ \
                                               /* persistent workgroups (the K-step stream continues across tiles); 0 = off */ \
  X(HCONVT_PERSIST, "hconvt_persist", 1)       /* hconvt.hip: launches with more tiles than CUs run as persistent workgroups (0: one tile each) */ \
  X(WGRAD_ROWS, "wgrad_rows", 1)               /* wgrad.hip: the im2col weight gradient stores whole tile rows through LDS; one split adds without atomics */ \
  X(SPLITK_MULTI, "splitk_multi", 1)           /* gconv.hip: split-K over the merged parity classes of a small stride-2 layer (one launch + one finalize) */ \
  X(SPLITK_RING, "splitk_ring", 1)             /* gconv.hip: split-K launches of the 128 x 128 tile run a 4-stage ring (three K-steps of cold weights in flight) */ \
  X(GCONV_RING4, "gconv_ring4", 16)            /* gconv.hip: 128-pixel im2col tiles in a grid of <= 2 workgroups per CU with at least this many K-steps run a 4-stage ring; 0 = off */ \
  X(HCONV5, "hconv5", 64)                      /* hconv5.hip: register-resident-weights kernel for the 16 -> 16 channel k5 volume convs; smallest volume */ \
                                               /* (batch x voxels / 2048) it takes (0 = off) */ \
  X(HCONV5_SEG, "hconv5_seg", 0)               /* ... z segments per column (0 = as many as fill the chip; tests force long segments with 1 / 2) */ \
  X(HWGRAD2, "hwgrad2", 2)                     /* hwgrad.hip: double-buffered, decode-once form of the narrow volume weight gradient with 65..128 taps */ \
                                               /* (>= 2: also for layers wide on both sides, 33..64 x 17..64 channels, instead of the im2col kernel) */ \
  X(HCONV2, "hconv2", 4)                       /* hconv.hip: persistent double-buffered form of the narrow volume forward / data-gradient kernel (17..64 output channels; */ \
                                               /* >= 2: also 64 -> 64 channels — wide on both sides — instead of the split-K im2col launch + its finalize; */ \
                                               /* >= 3: 32-channel layers on <= 128 boxes as two 16-channel groups per box; >= 4: 64-channel layers on <= 64 boxes as four) */ \
  X(PWISE, "pwise", 8)                         /* pwise.hip: register-operand kernels for one-tap layers with <= 8 channels on one side (smallest volume in 2048-voxel units, 0 = off) */ \
  X(DAXIS, "daxis", 8192)                         /* daxis.hip: streaming kernel for layers whose taps all lie on the row axis, 8..64 channels (the (k,1,1) half of a */ \
                                               /* separable volume conv and its data gradient): smallest launch in 64-voxel units (default: 2^19 voxels, where it measured */ \
                                               /* 2.9 x the other kernels; a tie at 2^18 voxels x 32 channels, a loss at 2^15 x 64: DESIGN.md 4.6), 0 = off */ \
  X(ELASTIC_ROWS, "elastic_rows", 32768)       /* volsample.hip: largest per-workgroup row table (bytes of LDS, at most 65536) with which the elastic gather runs */ \
                                               /* its row-shared form; beyond it, and with 0 always, the per-voxel form (tests and the timing tool force it) */
enum GsOpt {
#define GS_OPT_ENUM(id, name, def) GS_OPT_##id,
  GS_OPTIONS(GS_OPT_ENUM)
#undef GS_OPT_ENUM
  GS_OPT_COUNT
};
int gs_opt(int id);

// host-side error plumbing shared by the launchers
void gs_set_error(const char* fmt, ...);
const void* gs_zero_page();
void* gs_dump_page();          // 256 writable bytes nobody reads: destination of masked store lanes (pconv.hip)
#define GS_CHECK_HIP(x)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      gs_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)
#define GS_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      gs_set_error(__VA_ARGS__);   \
      return 2;                    \
    }                              \
  } while (0)
