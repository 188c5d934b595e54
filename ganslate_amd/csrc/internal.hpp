// Host functions that one .hip file of libganslate_hip.so defines and another calls: one declaration each, included by the
// defining file and by every caller (default arguments live here only). Not part of the C ABI (include/ganslate_hip.h).
// The GConvK-dependent pair of pconv.hip is declared in gconv.hpp.
#pragma once
#include "common.hpp"

// Raise Kernel's dynamic-LDS limit to `bytes`, once per process and kernel instantiation: the first call sets the attribute, later
// calls return at once — so `bytes` must be the largest value any launch of that instantiation asks for. Sites whose launch
// size is a constant of the instantiation (hconv5.hip, wgrad.hip) pass that size; the others pass the limit of the
// workgroup-per-CU class they were written for. An error of hipFuncSetAttribute is returned (GS_CHECK_HIP) and tried again.
template <auto Kernel>
int gs_allow_lds(int bytes) {
  static bool configured = false;
  if (!configured) {
    GS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    configured = true;
  }
  return 0;
}

// ---- api.hip ------------------------------------------------------------------------------------------------------------------
// 1024 floats + 1 counter for a loss reduction, one workspace per launching stream; nullptr (error set) before gs_init
float* gs_reduce_workspace(void* stream);

// ---- forward / data-gradient kernels that gconv.hip tries before the im2col kernel -------------------------------------------
// *_slots: partial-statistics slots per image the class writes when it runs on that kernel, 0 when the kernel does not take it.
// *_try: returns 0 and sets *handled = 1 when the launch went out there; *handled = 0: the caller goes on to the next kernel.
// daxis.hip: streaming kernel for layers whose taps all lie on the row axis (the (k,1,1) half of a separable volume conv)
int gs_daxis_slots(const gs_gconv_desc* d);
int gs_daxis_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                 void* stream, int* handled);
// pwise.hip: register-operand kernels for one-tap layers with <= 8 channels on one side; _multi: the 8 one-tap parity classes
// of a k2 stride-2 volume layer in one launch
int gs_pwise_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, void* stream,
                 int* handled);
int gs_pwise_multi_try(const gs_gconv_desc* const* descs, int count, const void* in, const void* const* w_packs, const float* bias,
                       void* out, float* stats, void* stream, int* handled);
// hconv.hip: halo-resident kernel for narrow stride-1 layers (asks hconv5.hip first)
int gs_hconv_slots(const gs_gconv_desc* d);
int gs_hconv_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                 void* stream, int* handled);
// hconv5.hip: register-resident-weights kernel for the 16 -> 16 channel k5 volume convs (one slot per 4 x 16 x 16 step of a column)
int gs_hconv5_slots(const gs_gconv_desc* d);
int gs_hconv5_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                  void* stream, int* handled);
// hconvw.hip: halo-resident kernel for the wide 3x3 stride-1 layers (one slot per 16 x 16 box); tw: twin batch
int gs_hconvw_slots(const gs_gconv_desc* d);
int gs_hconvw_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                  const gs_twin* tw, void* stream, int* handled);
// ... its RING form: the fused data gradient on the unpadded domain; an error unless gs_gconv_ring_slots(d) > 0
int gs_hconvw_ring(const gs_gconv_desc* d, const void* in, const void* w_pack, void* out, const gs_gconv_fuse* fuse,
                   const gs_twin* tw, void* stream);
// hstrip.hip: W-folded k7 boundary convs (vertical taps, <= 64 channels) out of a resident input strip (one slot per 32 x 8
// tile of a launch WITH statistics)
int gs_hstrip_slots(const gs_gconv_desc* d);
int gs_hstrip_try(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out, float* stats,
                  void* stream, int* handled, const gs_twin* tw);
// hconvt.hip: the four parity classes of a stride-2 layer out of one halo-resident pass. _pattern: 0 (1/2/2/4 taps) or
// 1 (4/4/4/4) when the layer runs there, -1 when it does not; _launch takes that pattern
int gs_hconvt_pattern(const gs_gconv_desc* const* descs, int count);
int gs_hconvt_launch(const gs_gconv_desc* const* descs, int pat, const void* in, const void* const* w_packs,
                     const float* bias, void* out, float* stats, const gs_gconv_fuse* fuse, void* stream,
                     const gs_twin* tw = nullptr);

// ---- weight-gradient kernels that wgrad.hip tries before the im2col kernel ---------------------------------------------------
// Both return 0 and set *handled when the layer ran there (*handled = 0: the caller falls back). ws != nullptr: partial sums go
// to slabs of ws and *handled is the number of slabs written (the caller adds them to dw in slab order), else 1 after atomic
// adds into dw; plan_only: nothing is launched, *handled is what a launch would return.
// hwgrad.hip: halo-resident kernels for narrow stride-1 layers and the wide 3x3 layers. a2/g2 != nullptr: a second operand
// pair of the same layer (only the wide kernel merges; otherwise *handled stays 0). tw != nullptr: twin batch (only the wide
// and few-tap kernels take it; *handled then is the number of slabs PER NETWORK, the second network's slabs follow the first's)
int gs_hwgrad_try2(const gs_wgrad_desc* d, const void* a, const void* g, const void* a2, const void* g2, float* dw,
                   float* ws, int plan_only, void* stream, int* handled, const gs_twin* tw);
// pwise.hip: one-tap layers with 8 channels on one side
int gs_pwise_wgrad_try(const gs_wgrad_desc* d, const void* a, const void* g, float* dw, float* ws, int plan_only, void* stream,
                       int* handled);

// ---- fixed-order reductions shared between files --------------------------------------------------------------------------------
// wgrad.hip: dst[e] += slab 0 [e] + slab 1 [e] + ... in slab order over n4 float4s, slabs stride4 float4s apart (nets = 2: the
// same for the second network of a twin launch, its slabs ws_y4 and its buffer dw_y4 float4s further on)
void gs_launch_slab_reduce(const float* ws, float* dst, long long n4, int slabs, long long stride4, hipStream_t st, int nets,
                           long long ws_y4, long long dw_y4);
// norm.hip: per-slot sums [N][slots][3][C] of an InstanceNorm backward -> per-image totals out [N][3][C]; one image with db and
// mean_rstd: the conv's bias gradient is added there too (shared with norm_ex.hip)
int gs_launch_slot_sum3(const float* in, float* out, int N, int slots, int C, float inv_hw, const float* mean_rstd,
                        float* db, hipStream_t st);
// norm.hip: the same for R = 3 or 4 sums per slot (R = 4, prelu.hip: the fourth total is the PReLU slope gradient, added to dslope);
// narrow: 4 channels per workgroup, not 16. Several images: the parameter gradients go through gs_launch_norm_param_grads.
int gs_launch_slot_sum(int R, bool narrow, const float* in, float* out, int N, int slots, int C, float inv_hw,
                       const float* mean_rstd, float* db, float* dslope, hipStream_t st);
// norm.hip: parameter gradients (bias, PReLU slope) summed over the images in a fixed order (shared with prelu.hip)
int gs_launch_norm_param_grads(const float* sums, int R, const float* mean_rstd, float* db, float* dslope, int N, int C,
                               float inv_hw, hipStream_t st);
