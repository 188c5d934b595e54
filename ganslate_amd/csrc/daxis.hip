// Streaming single-axis convolution: the (k,1,1) half of a separable volume conv (ganslate/nn/separable.py:5-78,
// conv_pointwise / conv_transp_pointwise) and, with the taps mirrored, its data gradient. The lowering (nn/native/spec.py)
// hands it over as a stride-1 class on the view [N', rows, H W, C] whose taps all lie on the row axis (dw = dd = 0):
//   out[n, o, p, co] = bias[co] + sum_u sum_ci in[n, o + omin + u, p, ci] * w[co][tap(u) Ci + ci]      (rows outside = 0)
// Its taps are a whole H W plane apart, so for the im2col and halo-box kernels every tap is a far-away gather and a box
// re-reads its row halo; at 8-64 channels the layer is pure streaming (S Ci MACs per output element against 2 + 2 bytes).
//
// A workgroup (4 waves) owns a strip of 64 pixels of the H W plane and a segment of rows; a wave owns 16 pixels = the 16
// columns of v_mfma_f32_16x16x32_bf16. A lane keeps the last S input rows of its pixel's channel octets in registers (the
// window), the weights (A operand, rows = output channels) stay in registers for the whole walk, and every step down the row
// axis loads ONE new row (16 bytes per lane and octet, two rows ahead of its use), runs the MFMAs over K = S Ci and stores
// one output row: inside a segment every input element is read once and every output element written once (a segment
// re-reads the S - 1 rows above its first). With Ci < 32 one 32-wide K step spans several taps: the lane groups (lane >> 4)
// then hold the same octets and pick different window slots.
// Epilogue: bias, activation, InstanceNorm partial sums — one slot of [2][Co] floats per workgroup, summed over the
// workgroup's lanes and waves in a fixed order (no atomics: two runs give the same bits).
#include "internal.hpp"

namespace {
struct DaxK {
  const char* in;
  const char* w;               // [w_rows][Kp] bf16 pack, k = tap * Ci + ci
  const float* bias;
  char* out;
  float* stats;
  int N, Hi, Ho, W;            // rows of the input / output view image, pixels per row
  int in_cs, in_co, out_cs, out_co, Co, Kp, w_rows, act;
  float slope;
  int omin;                    // input row of window slot 0 relative to the output row
  int tap_of_slot[8];
  int seg_len, nseg, nstrips, stats_slots, stats_slot0;
};

template <int CI>
struct DaxCfg {
  static constexpr int OCT = CI / 8;                         // octets per tap
  static constexpr int OPL = CI >= 32 ? CI / 32 : 1;         // octets a lane holds per window slot
};

// CI: input channels; CT: 16-row output tiles (Co <= 16 CT); S: window span (taps)
template <int CI, int CT, int S>
__global__ __launch_bounds__(256) void daxis_kernel(const DaxK p) {
  constexpr int OCT = DaxCfg<CI>::OCT, OPL = DaxCfg<CI>::OPL;
  constexpr int KS = (S * CI + 31) / 32;                     // 32-wide K steps
  constexpr bool PAIR = (CT % 2) == 0;                       // two tiles give a lane 8 consecutive channels: 16-byte stores
  __shared__ float red[4][2][64];
  const int lane = threadIdx.x & 63, col = lane & 15, ko = lane >> 4;
  const int wave = threadIdx.x >> 6;
  const int strip = blockIdx.x, seg = blockIdx.y, n = blockIdx.z;
  const int pix = strip * 64 + wave * 16 + col;
  const bool pix_ok = pix < p.W;
  const int o0 = seg * p.seg_len;
  const int o1 = min(o0 + p.seg_len, p.Ho);

  // ---- weights: A operand, row = col -> output channel, k octet = 4 s + ko -> (window slot, channel octet) ----------------
  bf16x8 wa[CT][KS];
  float bs[CT][4];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int ch_row = PAIR ? (c >> 1) * 32 + (col >> 2) * 8 + (c & 1) * 4 + (col & 3) : c * 16 + col;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int q = s * 4 + ko, u = q / OCT, oct = q - u * OCT;
      uint4 v{0u, 0u, 0u, 0u};
      if (u < S && ch_row < p.Co && ch_row < p.w_rows)
        v = *reinterpret_cast<const uint4*>(p.w + ((size_t)ch_row * p.Kp + p.tap_of_slot[u] * CI + oct * 8) * 2);
      wa[c][s] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = PAIR ? (c >> 1) * 32 + ko * 8 + (c & 1) * 4 + i : c * 16 + ko * 4 + i;
      bs[c][i] = (p.bias && ch < p.Co) ? p.bias[ch] : 0.f;
    }
  }

  // ---- the window ---------------------------------------------------------------------------------------------------------
  const char* in_n = p.in + ((size_t)n * p.Hi * p.W * p.in_cs + p.in_co) * 2;
  char* out_n = p.out + ((size_t)n * p.Ho * p.W * p.out_cs + p.out_co) * 2;
  auto load_row = [&](int row, uint4 (&dst)[OPL]) {
    const bool ok = pix_ok && row >= 0 && row < p.Hi;
#pragma unroll
    for (int j = 0; j < OPL; ++j) {
      const int oct = CI >= 32 ? ko + 4 * j : (ko & (OCT - 1));
      dst[j] = ok ? *reinterpret_cast<const uint4*>(in_n + (((size_t)row * p.W + pix) * p.in_cs + oct * 8) * 2)
                  : uint4{0u, 0u, 0u, 0u};
    }
  };
  uint4 win[S][OPL], nx1[OPL], nx2[OPL];
#pragma unroll
  for (int u = 0; u < S; ++u) load_row(o0 + p.omin + u, win[u]);
  load_row(o0 + p.omin + S, nx1);

  float s1[CT][4], s2[CT][4];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) { s1[c][i] = 0.f; s2[c][i] = 0.f; }

#pragma unroll 1
  for (int o = o0; o < o1; ++o) {
    load_row(o + p.omin + S + 1, nx2);                       // two rows ahead of its use as the window's last slot
    f32x4 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = f32x4{bs[c][0], bs[c][1], bs[c][2], bs[c][3]};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 b{0u, 0u, 0u, 0u};
      if constexpr (CI >= 32) {
        b = win[s / OPL][s % OPL];
      } else {
        // slot of this lane's octet in K step s: (4 s + ko) / OCT — one of 32 / CI slots, picked per lane group
        constexpr int SPS = 4 / OCT;                         // slots per K step
#pragma unroll
        for (int e = 0; e < SPS; ++e) {
          const int u = s * SPS + e;
          if (u < S && (ko / OCT) == e) b = win[u][0];
        }
      }
      const bf16x8 bx = __builtin_bit_cast(bf16x8, b);
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[c][s], bx, acc[c], 0, 0, 0);
    }
    // ---- epilogue of the row -----------------------------------------------------------------------------------------------
    char* orow = out_n + ((size_t)o * p.W + pix) * p.out_cs * 2;
    if constexpr (PAIR) {
#pragma unroll
      for (int m = 0; m < CT / 2; ++m) {
        const int ch = m * 32 + ko * 8;
        float r[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          r[i] = apply_act_small(acc[2 * m][i], p.act, p.slope);
          r[4 + i] = apply_act_small(acc[2 * m + 1][i], p.act, p.slope);
        }
        if (pix_ok && ch < p.Co) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s1[2 * m][i] += acc[2 * m][i];         s2[2 * m][i] += acc[2 * m][i] * acc[2 * m][i];
            s1[2 * m + 1][i] += acc[2 * m + 1][i]; s2[2 * m + 1][i] += acc[2 * m + 1][i] * acc[2 * m + 1][i];
          }
          *reinterpret_cast<uint4*>(orow + (size_t)ch * 2) =
              uint4{pack_bf2(r[0], r[1]), pack_bf2(r[2], r[3]), pack_bf2(r[4], r[5]), pack_bf2(r[6], r[7])};
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int ch = c * 16 + ko * 4;
        if (pix_ok && ch < p.Co) {
          float r[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s1[c][i] += acc[c][i];
            s2[c][i] += acc[c][i] * acc[c][i];
            r[i] = apply_act_small(acc[c][i], p.act, p.slope);
          }
          *reinterpret_cast<uint2*>(orow + (size_t)ch * 2) = uint2{pack_bf2(r[0], r[1]), pack_bf2(r[2], r[3])};
        }
      }
    }
    // ---- slide the window ---------------------------------------------------------------------------------------------------
#pragma unroll
    for (int u = 0; u + 1 < S; ++u)
#pragma unroll
      for (int j = 0; j < OPL; ++j) win[u][j] = win[u + 1][j];
#pragma unroll
    for (int j = 0; j < OPL; ++j) { win[S - 1][j] = nx1[j]; nx1[j] = nx2[j]; }
  }

  // ---- InstanceNorm partial sums: lanes of a row (the 16 pixels), then the 4 waves in wave order --------------------------
  if (p.stats_slots > 0) {
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = row16_sum(s1[c][i]), q = row16_sum(s2[c][i]);
        const int ch = PAIR ? (c >> 1) * 32 + ko * 8 + (c & 1) * 4 + i : c * 16 + ko * 4 + i;
        if (col == 0 && ch < 64) { red[wave][0][ch] = a; red[wave][1][ch] = q; }
      }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * p.Co) {
      const int which = t / p.Co, ch = t - which * p.Co;
      const float v = ((red[0][which][ch] + red[1][which][ch]) + red[2][which][ch]) + red[3][which][ch];
      const int slot = p.stats_slot0 + seg * p.nstrips + strip;
      p.stats[(((size_t)n * p.stats_slots + slot) * 2 + which) * p.Co + ch] = v;
    }
  }
}

struct DaxPlan {
  int ok, omin, S, nstrips, nseg, seg_len;
  int tap_of_slot[8];
};

// What only a LAUNCH knows: channel slices and accumulate go to the existing kernels. gs_gconv_stat_slots is asked with a dense
// descriptor (HipOps.stat_slots), so a sliced launch of an eligible class WITH statistics would get this kernel's slot count and
// another kernel's slot layout: gs_daxis_try refuses that combination instead of mis-running it. (No caller has it: the
// (k,1,1) statistics launches read the dense intermediate, and accumulate excludes statistics.)
bool daxis_dense(const gs_gconv_desc* d) {
  return !d->accumulate && !d->in_co && !d->out_co && d->in_cs == d->Ci && d->out_cs == d->Co;
}

DaxPlan daxis_plan(const gs_gconv_desc* d) {
  DaxPlan pl{};
  const int opt = gs_opt(GS_OPT_DAXIS);
  if (!opt || !d) return pl;
  if (d->so != 1 || d->si != 1 || d->border != GS_BORDER_ZERO || d->pz || d->py || d->px) return pl;
  if (d->Di != 1 || d->Do != 1 || d->Dc != 1 || d->Wi != d->Wo || d->Wc != d->Wo || d->Hc != d->Ho) return pl;
  if (d->Ci != 8 && d->Ci != 16 && d->Ci != 32 && d->Ci != 64) return pl;
  if (d->Co != 8 && d->Co != 16 && d->Co != 32 && d->Co != 64) return pl;
  if (d->w_rows < d->Co || (d->T != 2 && d->T != 5)) return pl;
  int omin = 127;
  for (int t = 0; t < d->T; ++t) {
    if (d->dw[t] || d->dd[t]) return pl;                     // all taps on the row axis
    if (d->dh[t] < omin) omin = d->dh[t];
  }
  for (int u = 0; u < 8; ++u) pl.tap_of_slot[u] = -1;
  for (int t = 0; t < d->T; ++t) {
    const int u = d->dh[t] - omin;
    if (u >= d->T || pl.tap_of_slot[u] >= 0) return pl;      // consecutive, distinct offsets
    pl.tap_of_slot[u] = t;
  }
  const long long vox = (long long)d->N * d->Ho * d->Wo;
  if (vox < (long long)opt * 64 || d->N > 65535) return pl;    // (option: smallest launch in 64-voxel units)
  pl.omin = omin;
  pl.S = d->T;
  pl.nstrips = (d->Wo + 63) / 64;
  // row segments: enough workgroups to fill the chip (8 per CU), but at least 8 rows each (a segment re-reads S - 1 rows)
  long long want = 2048 / ((long long)d->N * pl.nstrips);
  int nseg = want < 1 ? 1 : (want > 65535 ? 65535 : (int)want);
  const int max_seg = d->Ho / 8 > 1 ? d->Ho / 8 : 1;
  if (nseg > max_seg) nseg = max_seg;
  pl.seg_len = (d->Ho + nseg - 1) / nseg;
  pl.nseg = (d->Ho + pl.seg_len - 1) / pl.seg_len;
  pl.ok = 1;
  return pl;
}
}  // namespace

// gconv.hip (gs_gconv_stat_slots): statistics slots per image this kernel writes for the class, 0 = it does not take it
int gs_daxis_slots(const gs_gconv_desc* d) {
  const DaxPlan pl = daxis_plan(d);
  return pl.ok && daxis_dense(d) ? pl.nstrips * pl.nseg : 0;
}

// gconv.hip (gs_gconv_forward): *handled = 1 when the launch went out here
int gs_daxis_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                 void* stream, int* handled) {
  *handled = 0;
  const DaxPlan pl = daxis_plan(d);
  if (!pl.ok) return 0;
  if (!daxis_dense(d)) {
    GS_REQUIRE(d->stats_slots == 0, "gs_gconv_forward: a channel-sliced launch with statistics of a class the row-axis kernel "
                                    "takes: gs_gconv_stat_slots answered for the dense launch");
    return 0;
  }
  DaxK k;
  k.in = static_cast<const char*>(in); k.w = static_cast<const char*>(w_pack); k.bias = bias;
  k.out = static_cast<char*>(out); k.stats = stats;
  k.N = d->N; k.Hi = d->Hi; k.Ho = d->Ho; k.W = d->Wo;
  k.in_cs = d->in_cs; k.in_co = d->in_co; k.out_cs = d->out_cs; k.out_co = d->out_co;
  k.Co = d->Co; k.Kp = d->Kp; k.w_rows = d->w_rows; k.act = d->act; k.slope = d->slope;
  k.omin = pl.omin;
  for (int u = 0; u < 8; ++u) k.tap_of_slot[u] = pl.tap_of_slot[u] < 0 ? 0 : pl.tap_of_slot[u];
  k.seg_len = pl.seg_len; k.nseg = pl.nseg; k.nstrips = pl.nstrips;
  k.stats_slots = d->stats_slots; k.stats_slot0 = d->stats_slot0;
  if (k.stats_slots > 0)
    GS_REQUIRE(k.stats_slot0 + pl.nstrips * pl.nseg <= k.stats_slots, "gs_gconv_forward: class writes statistics slots %d..%d of %d",
               k.stats_slot0, k.stats_slot0 + pl.nstrips * pl.nseg - 1, k.stats_slots);
  const dim3 grid((unsigned)pl.nstrips, (unsigned)pl.nseg, (unsigned)d->N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ct = d->Co <= 16 ? 1 : d->Co / 16;
#define GS_DAX(CI_, CT_, S_)                                                                        \
  if (d->Ci == CI_ && ct == CT_ && pl.S == S_) {                                                    \
    hipLaunchKernelGGL((daxis_kernel<CI_, CT_, S_>), grid, dim3(256), 0, st, k);                    \
    GS_CHECK_HIP(hipGetLastError());                                                                \
    *handled = 1;                                                                                   \
    return 0;                                                                                       \
  }
#define GS_DAX_CI(CI_) GS_DAX(CI_, 1, 5) GS_DAX(CI_, 2, 5) GS_DAX(CI_, 4, 5) GS_DAX(CI_, 1, 2) GS_DAX(CI_, 2, 2) GS_DAX(CI_, 4, 2)
  GS_DAX_CI(8) GS_DAX_CI(16) GS_DAX_CI(32) GS_DAX_CI(64)
#undef GS_DAX_CI
#undef GS_DAX
  return 0;
}
