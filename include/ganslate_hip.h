/*
 * ganslate_hip.h — C ABI of libganslate_hip.so, the MI355X (gfx950) drop-in for the arithmetic of
 * ganslate's GAN training step.
 *
 * The reference (ganslate-team/ganslate @ v1) has no native code: every entry point below replaces a
 * torch / cuDNN / apex call site on the hot path `BaseGAN.optimize_parameters`
 * (ganslate/nn/gans/unpaired/cyclegan.py:92-124). The reference call site each function stands in for is
 * cited next to it. Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host";
 *   - every call enqueues on the caller's `stream` (a hipStream_t passed as void*) and never
 *     synchronises; the caller owns all tensors, the library owns nothing but a 256-byte zero page;
 *   - return value 0 = ok, non-zero = error, message via gs_last_error();
 *   - one process per GPU, like the reference's DDP launch: the library's state (zero page, loss-reduction workspaces per
 *     launching stream, kernel-selection options) is per process. Launch calls may come from several host threads (the
 *     autograd engine runs backward on its own): workspace assignment is locked and gs_last_error() is per thread — read
 *     it on the thread whose call failed. gs_set_option is not synchronised against concurrent launches.
 *
 * Data layout: activations are NHWC bf16 with the channel count padded to a multiple
 * of 8 ("act" below); images at the network boundary are NCHW fp32 exactly as the reference's
 * `visuals` (cyclegan.py:39); master weights/grads/Adam state are fp32 in the "OTI" layout
 * [P][T][Q] (P = out channels for Conv, in channels for ConvTranspose; T = kh*kw taps, row-major;
 * Q = the other channel count, padded to a multiple of 8); bf16 weight packs are [rows][Kp] with
 * Kp = roundup(T_class*Q, 64), K contiguous.
 */
#ifndef GANSLATE_HIP_H
#define GANSLATE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_MAX_TAPS 352   /* 7x7x7 = 343 taps of the 3-D stem / output convs (resnet3d.py:25,64) */

/* border handling of the gathered operand (reference: nn.ReflectionPad2d resnet2d.py:24,
 * nn.ReplicationPad3d resnet3d.py:15, Conv2d(padding=1) zero padding resnet2d.py:35) */
enum { GS_BORDER_ZERO = 0, GS_BORDER_REFLECT = 1, GS_BORDER_REPLICATE = 2 };
/* activations (nn.ReLU resnet2d.py:27, nn.LeakyReLU(0.2) patchgan2d.py:30, nn.Tanh resnet2d.py:65) */
enum { GS_ACT_NONE = 0, GS_ACT_RELU = 1, GS_ACT_LRELU = 2, GS_ACT_TANH = 3 };

/* One "generalised convolution" class:
 *   out[n, z*so+pz, i*so+py, j*so+px, co] = bias[co] + sum_{t<T} sum_{ci<Ci}
 *        in[n, B(z*si+dd[t]), B(i*si+dh[t]), B(j*si+dw[t]), ci] * w[co][t*Ci+ci]     (z<Dc, i<Hc, j<Wc)
 * With so=1 it is nn.Conv2d/Conv3d forward (stride si) or the data-gradient of a stride-1 conv; with so=2
 * it is one output-parity class of nn.ConvTranspose2d/3d(stride=2) forward or of the data-gradient of a
 * stride-2 conv. B() applies `border`. 2-D tensors are the depth-1 case (Di=Do=Dc=1, pz=0, dd[]=0);
 * volumes are NDHWC (resnet3d.py:25-64, patchgan3d.py:28-60). Di*Hi must stay below 32768. */
typedef struct gs_gconv_desc {
  int32_t N, Hi, Wi, Ci;       /* gathered input: logical dims; Ci multiple of 8, Ci/8 a power of two */
  int32_t Di, Do, Dc, pz;      /* depth of the input / output / class and the depth phase (1,1,1,0 in 2-D) */
  int32_t in_cs, in_co;        /* input channel stride / channel offset in elements (concat views) */
  int32_t Ho, Wo, Co;          /* full output dims; Co = number of channels written, multiple of 8 */
  int32_t out_cs, out_co;      /* output channel stride / offset */
  int32_t Hc, Wc;              /* class extent */
  int32_t so, py, px, si;      /* output stride+phase, input stride */
  int32_t T;                   /* taps in this class */
  int32_t Kp;                  /* padded K of the weight pack = roundup(T*Ci, 64) */
  int32_t w_rows;              /* rows present in the weight pack (>= Co) */
  int32_t border;              /* GS_BORDER_* */
  int32_t act;                 /* GS_ACT_* applied in the epilogue (after bias) */
  float   slope;               /* LeakyReLU slope */
  int32_t stats_slots;         /* partial-stat slots per image in `stats` (0 = no stats) */
  int32_t stats_slot0;         /* first slot this class writes; it writes ceil(Dc*Hc*Wc/tile_m) slots */
  int32_t accumulate;          /* != 0: out += result (bf16 read-modify-write; the gradient joins of the additive
                                * coupling blocks, ganslate/nn/invertible.py:8-48); no bias/activation/stats then */
  int8_t  dh[GS_MAX_TAPS];
  int8_t  dw[GS_MAX_TAPS];
  int8_t  dd[GS_MAX_TAPS];
} gs_gconv_desc;

/* Weight-gradient of the same family:
 *   dw[p][t*Q+q] += sum_{n,z,i,j} a[n,z,i,j,p] * g[n, B(z*si+dd[t]), B(i*si+dh[t]), B(j*si+dw[t]), q]
 * (`a` is the dense side: dY for Conv, X for ConvTranspose; `g` the gathered side; Da=Dg=1 in 2-D). */
typedef struct gs_wgrad_desc {
  int32_t N, Ha, Wa, P, a_cs, a_co;
  int32_t Hg, Wg, Q, g_cs, g_co;    /* Q multiple of 8, Q/8 a power of two */
  int32_t Da, Dg;
  int32_t si, T, border;
  int32_t dw_ld;                    /* leading dimension of dw rows = T*Q */
  int32_t dw_fresh;                 /* hint: the caller guarantees that dw holds zeros (first weight gradient of this layer since
                                     * the optimiser cleared the buffer): a launch that is the only contributor of its elements
                                     * stores instead of read-add-store. 0 is always valid. The hint covers the FIRST operand
                                     * pair of a call only (gs_wgrad_pair / gs_wgrad_ws with a2: the second pair always adds).
                                     * One-split launches add to dw with plain loads / stores, not atomics: two weight-gradient
                                     * launches of the same layer must not overlap on different streams (order them with an
                                     * event, as NativeNet does between the backward passes of a network). */
  int8_t  dh[GS_MAX_TAPS];
  int8_t  dw_[GS_MAX_TAPS];
  int8_t  dd[GS_MAX_TAPS];
} gs_wgrad_desc;

/* Twin batch: two networks of IDENTICAL architecture over one batch — the two generators (discriminators) of a CycleGAN
 * step see independent data in every phase (cyclegan.py:126-152: G_AB(real_A) next to G_BA(real_B), G_AB(fake_A) next to
 * G_BA(fake_B); :154-189 for D_B / D_A), and with per-sample InstanceNorm nothing couples the images of a batch. Images
 * [0, n_split) use the weights / bias / gradient buffers passed to the call, images [n_split, N) the same layouts
 * `*_delta` BYTES further on (the second network's pack, master and gradient buffers have the first one's layout). */
typedef struct gs_twin {
  int32_t n_split, pad_;
  int64_t w_delta;             /* bf16 weight pack */
  int64_t bias_delta;          /* fp32 bias vector (master buffer) */
  int64_t dw_delta;            /* fp32 weight-gradient buffer (gs_wgrad_ws_twin) */
} gs_twin;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int gs_init(int device);                 /* torch.cuda.set_device + lazy cuDNN handle (base.py:84-91) */
void gs_shutdown(void);
const char* gs_last_error(void);
/* Kernel-selection switches (A/B measurements, parity tests): the library reads NO environment variable; the host
 * side maps its GS_* variables onto these (ganslate_amd/hip/ops.py). Names, in the order of the table in api.hip:
 * splitk, splitk_max_blocks, splitk_target, hconv, hconv_wide, hwgrad, hwgrad_wide, hwgrad_planes, norm_bwd_ppb,
 * norm_apply_unroll, gconv_tile288, gconv_multi, hconvw_ring, hconvt (smallest grid the parity-class halo kernel takes,
 * 0 = off), hstrip (same for the k7 boundary-conv kernel), wfold_rows, hwgrad_ft, gconv_big, hconv_box8, hconvw_persist,
 * hstrip_regs, gconv_twin, wgrad_twin, gconv_persist, hconvt_persist, wgrad_rows, splitk_multi, splitk_ring, gconv_ring4,
 * hconv5 (register-resident-weights kernel for the 16 -> 16 channel k5 volume convs: smallest volume in units of 2048 voxels,
 * 0 = off), hconv5_seg (z segments per column, 0 = auto), hwgrad2 / hconv2 (double-buffered volume forms of the narrow weight
 * gradient / forward kernels), pwise (one-tap layers with <= 8 channels on one side — the V-Net's 32 -> 1 output conv — on
 * register-operand kernels: smallest volume in units of 2048 voxels, 0 = off), daxis (streaming kernel for stride-1 classes
 * whose taps all lie on the row axis with 8..64 channels — the (k,1,1) half of a separable volume conv on its [N, D, H W, C]
 * view, and its data gradient: smallest launch in units of 64 voxels, 0 = off; default 8192), elastic_rows (largest row table,
 * in bytes of LDS, with which gs_patch_elastic* run their row-shared form; 0 = always per voxel; both give the same bits).
 * Every setting computes the same function (up to
 * the fp32 summation order and, for hconvw_ring, where the bf16 rounding of the folded gradient happens); none skips work.
 * Unknown name -> non-zero. */
int gs_set_option(const char* name, int value);
int gs_get_option(const char* name, int* value);
int gs_tile_m(const gs_gconv_desc* d);   /* pixel-tile height of the im2col kernel for this class */
/* number of partial-statistics slots per image gs_gconv_forward writes for this class (pixel tiles of the im2col
 * kernel, or output boxes of the halo-resident kernel narrow stride-1 layers run on): size `stats` with it */
int gs_gconv_stat_slots(const gs_gconv_desc* d);

/* ---- convolution family (torch.nn.Conv2d / ConvTranspose2d forward + autograd backward) --------- */
/* resnet2d.py:25,35,52-57,65,80-87; patchgan2d.py:29,36-62; backward via loss.backward() base.py:170 */
int gs_gconv_forward(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias,
                     void* out, float* stats, void* stream);
/* The output-parity classes of ONE layer (stride-2 transposed conv forward, data gradient of a stride-2 conv: 4 classes in
 * 2-D, 8 in 3-D — SURVEY.md §2.3 K3/K4; resnet2d.py:52-57, patchgan2d.py:36-48 backward) in one launch. descs[c] /
 * w_packs[c] are what `count` calls of gs_gconv_forward would take; the classes must agree in everything but taps, Kp,
 * output phase (pz,py,px) and stats_slot0, with at most 8 taps each — otherwise (and for count == 1) the call runs them one
 * after the other, so it is always valid to use. On the im2col kernel the results equal the separate launches bit for bit.
 * 2-D k3 / k4 layers with channel counts that are multiples of 64, a class grid that is a multiple of 16 and a large enough
 * grid run all four classes out of one halo-resident pass instead (hconvt.hip, option `hconvt`): same function, another
 * fp32 summation order, and of the layer's `stats_slots` slots the first (class grid / 256) hold the per-box sums over all
 * classes while the others are written as zeros — consumers sum the slots, as gs_inorm_finalize does. */
int gs_gconv_forward_multi(const gs_gconv_desc* const* descs, int32_t count, const void* in, const void* const* w_packs,
                           const float* bias, void* out, float* stats, void* stream);
/* The same with split-K over the MERGED grid (unet2d.py:110-157: the U-Net's inner stride-2 transposed convs and the data
 * gradients of its inner stride-2 convs — four classes of 1-512 pixels each with K = 4 x 256..2048): (classes x tiles x
 * splits) workgroups write fp32 partial sums to ws[split][output pixel][Co] (the classes partition the output pixels) and
 * one finalize pass applies bias / activation / statistics for all classes. gs_gconv_multi_splitk_ws_floats: floats of ws
 * the call wants, 0 when it would not split (classes that do not merge, a layer the halo-resident class kernel takes, a
 * merged grid that is large enough). ws == NULL or smaller than that: exactly gs_gconv_forward_multi. Deterministic (fixed
 * summation order); per-class launches through gs_gconv_forward_ws give the same sums in another split. */
int64_t gs_gconv_multi_splitk_ws_floats(const gs_gconv_desc* const* descs, int32_t count);
int gs_gconv_forward_multi_ws(const gs_gconv_desc* const* descs, int32_t count, const void* in, const void* const* w_packs,
                              const float* bias, void* out, float* stats, float* ws, int64_t ws_floats, void* stream);

/* Data-gradient launch of a stride-1 conv with the first pass of the consumer's InstanceNorm backward fused into its
 * epilogue: while the tile of the (padded-domain) gradient g is stored, the per-tile sums of ghat = (fold(g) + g2) *
 * act'(yhat), ghat * yhat and yhat over the pixels of the tile are written to partial[N][slots][3][C] (slots =
 * gs_gconv_stat_slots(d)), exactly what the reduction pass of gs_inorm_act_backward would produce — pass that buffer to it
 * as `scratch` with pre_slots = slots. y / mean_rstd: raw output and statistics of the conv in front of that norm on the
 * unpadded domain Dy x Hy x Wy; the launch's output domain is that domain padded by `fold` (resnet2d.py:80-87 backward). */
typedef struct gs_gconv_fuse {
  const void* y;
  const float* mean_rstd;
  const void* g2;              /* optional residual-join gradient on the unpadded domain */
  float* partial;
  int32_t Dy, Hy, Wy;
  int32_t fold, fold_mode, act;
  float slope;
} gs_gconv_fuse;
int gs_gconv_forward_fused(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out,
                           float* stats, const gs_gconv_fuse* fuse, void* stream);

/* The fused data gradient (contract of gs_gconv_forward_fused: sums over the consumer's InstanceNorm-backward terms in the
 * epilogue, one slot of [3][Co] floats per workgroup tile) for the output-parity classes of a stride-2 conv's data gradient
 * (resnet2d.py:35 backward) when the layer runs on the halo-resident class kernel: gs_gconv_multi_fused_slots says whether
 * (0 = no) and how many slots per image the launch writes; fuse->fold must be 0 (zero-padded layers). */
int gs_gconv_multi_fused_slots(const gs_gconv_desc* const* descs, int32_t count);
int gs_gconv_forward_multi_fused(const gs_gconv_desc* const* descs, int32_t count, const void* in, const void* const* w_packs,
                                 void* out, const gs_gconv_fuse* fuse, void* stream);
/* Unpadded form of the same launch for the reflect-padded (pad 1) wide 3x3 residual convs (resnet2d.py:80-87): when
 * gs_gconv_ring_slots(d) > 0 for the ZERO-border data-gradient descriptor on the unpadded domain (Hi x Wi = Ho x Wo = the
 * conv's input extent, taps t = 3*ry + rx at (dh, dw) = (1 - ry, 1 - rx)), gs_gconv_forward_fused may be called with that
 * descriptor and fold = 1, fold_mode = reflect, Hy x Wy = Ho x Wo: the launch computes the gradient pixels one step
 * outside the image as well and adds them to the pixels the reflection folds them onto (in fp32, before rounding), so
 * `out` is the finished input gradient and the consumer runs with fold = 0. partial is [N][slots][3][C] with
 * slots = gs_gconv_ring_slots(d). Returns 0 slots when the layer / grid does not suit the halo kernel; the padded form
 * above is always available. */
int gs_gconv_ring_slots(const gs_gconv_desc* d);
/* Twin batches (gs_twin above). gs_gconv_twin_native: 1 when the kernel gs_gconv_forward (fuse == NULL) or
 * gs_gconv_forward_fused (fuse != NULL) would pick for `d` — d->N = the whole batch of both networks — selects the weight
 * set per image; 0: the caller runs the two halves as two launches (always possible: the halves are contiguous).
 * gs_gconv_forward_twin is that launch (fuse == NULL: gs_gconv_forward, else gs_gconv_forward_fused) and fails where
 * gs_gconv_twin_native says 0. The wide 3x3 residual convs (resnet2d.py:80-87) are native: a twin launch at batch 2 x 8 has
 * 512 tiles for 256 CUs and every workgroup walks two of them, the second tile's operands arriving under the first one's
 * K loop (csrc/hconvw.hip). */
int gs_gconv_twin_native(const gs_gconv_desc* d, const gs_gconv_fuse* fuse);
/* The same for the output-parity classes of one layer (gs_gconv_forward_multi / _multi_fused): native where the classes run on
 * the halo-resident class kernel (2-D k3 / k4 stride-2 layers with 64-multiple channels, csrc/hconvt.hip), which picks the
 * packs per 16 x 16 box; the descriptors carry the whole batch of both networks. fuse == NULL: bias / stats as in
 * gs_gconv_forward_multi; else the contract of gs_gconv_forward_multi_fused (bias = stats = NULL). */
int gs_gconv_multi_twin_native(const gs_gconv_desc* const* descs, int32_t count);
int gs_gconv_forward_multi_twin(const gs_gconv_desc* const* descs, int32_t count, const void* in, const void* const* w_packs,
                                const float* bias, void* out, float* stats, const gs_gconv_fuse* fuse, const gs_twin* tw,
                                void* stream);
int gs_gconv_forward_twin(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out,
                          float* stats, const gs_gconv_fuse* fuse, const gs_twin* tw, void* stream);
/* Same launch as gs_gconv_forward with a caller-owned fp32 workspace for split-K: layers with few output tiles and a
 * long K loop (U-Net bottleneck convs unet2d.py:129-136, the PatchGAN 512->1 tail patchgan2d.py:62) run their K range
 * split over the chip and a second pass sums the partial results and applies bias / statistics / activation.
 * gs_gconv_splitk_ws_floats(d) is the workspace the launch wants (0: it does not split; gs_gconv_forward_ws then
 * equals gs_gconv_forward). Results match gs_gconv_forward up to the fp32 summation order. */
int64_t gs_gconv_splitk_ws_floats(const gs_gconv_desc* d);
int gs_gconv_forward_ws(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias,
                        void* out, float* stats, float* ws, int64_t ws_floats, void* stream);
int gs_wgrad(const gs_wgrad_desc* d, const void* a, const void* g, float* dw, void* stream);
/* dw += wgrad(a1, g1) + wgrad(a2, g2): two operand pairs of the same layer and shapes — the two backward passes a
 * generator sees per step (cyclegan.py:139-150: G_AB(real_A) and G_AB(fake_A)) — in one launch where possible */
int gs_wgrad_pair(const gs_wgrad_desc* d, const void* a1, const void* g1, const void* a2, const void* g2, float* dw,
                  void* stream);
/* Weight gradient + Adam in one launch, for a layer whose gradient has ONE contributor in the optimiser step (a network that
 * takes one backward pass per step — Pix2Pix's generator, pix2pix.py:84-88 — and a layer of few pixels, where the launch is one
 * workgroup per output tile): the tile's sums never go to memory; its workgroup updates the parameters, the moments and the bf16
 * pack groups right away (the arithmetic of gs_adam_step_dev_packs with grad_scale 1, element for element). The gradient buffer of
 * the layer is neither read nor written (it stays cleared). Pointers are to the LAYER's slice (element 0 = dw[0][0], a multiple of
 * 8 elements into the flat buffers, 16-byte aligned); inv_f / inv_d as in gs_adam_step_dev_packs, offset to the slice's first
 * group. gs_wgrad_adam_eligible: 1 when the layer runs as a one-split launch of the im2col kernel; else run gs_wgrad_ws and the
 * optimiser as usual. */
typedef struct gs_adam_fuse {
  float *p, *m, *v;
  const float* hyper;          /* device float[6]: lr, beta1, beta2, eps, 1 - beta1^t, sqrt(1 - beta2^t) */
  const int32_t* inv_f; void* fpack;
  const int32_t* inv_d; void* dpack;
  /* optional (tr_pack != NULL): the layer's TRANSPOSED pack (data-gradient pack of a conv, forward pack of a transposed conv:
   * 8 consecutive pack elements = 8 consecutive rows p of one (tap, q) column) written by the same launch, so that no refresh
   * from the master is needed afterwards: pack element of W[p][t][q] = tr_base[t] + q * tr_kp[t] + p (device int32[T]; tr_base[t]
   * < 0: the tap is in no class; all three multiples of 8) */
  const int32_t* tr_base; const int32_t* tr_kp; void* tr_pack;
} gs_adam_fuse;
int gs_wgrad_adam_eligible(const gs_wgrad_desc* d);
int gs_wgrad_adam(const gs_wgrad_desc* d, const void* a, const void* g, const gs_adam_fuse* adam, void* stream);
/* Deterministic form of gs_wgrad (a2 = g2 = NULL) / gs_wgrad_pair: workgroups that share output elements (split-K over
 * pixels) write partial sums to slabs of a caller-owned workspace and a second launch adds the slabs to dw in a fixed
 * order, instead of fp32 atomics on dw — two runs give bit-identical gradients (torch.use_deterministic_algorithms-like
 * behaviour of the reference's cuDNN weight gradients is NOT guaranteed either; this is what the loss-curve parity tests
 * run on). gs_wgrad_ws_floats: workspace the call wants (floats; < 0: bad descriptor; 0: every output element has a single
 * contributing workgroup, which then accumulates straight into dw — ws may be NULL). */
int64_t gs_wgrad_ws_floats(const gs_wgrad_desc* d, int32_t pair);
int gs_wgrad_ws(const gs_wgrad_desc* d, const void* a1, const void* g1, const void* a2, const void* g2, float* dw,
                float* ws, int64_t ws_floats, void* stream);
/* Twin batches (gs_twin): d->N = all images of both networks (each operand tensor holds the first network's N / 2 images,
 * then the second's); the second network's gradient goes to dw + tw->dw_delta bytes. gs_wgrad_twin_native: 1 when the
 * layer's kernel takes both networks in one launch (the wide 3x3 residual convs, resnet2d.py:80-87 backward: half the pixel
 * splits per network, half the slab traffic); else the caller runs gs_wgrad_ws on the two halves. Workspace:
 * gs_wgrad_ws_floats_twin (both networks' slabs). Deterministic like gs_wgrad_ws. */
int gs_wgrad_twin_native(const gs_wgrad_desc* d, int32_t pair);
int64_t gs_wgrad_ws_floats_twin(const gs_wgrad_desc* d, int32_t pair);
int gs_wgrad_ws_twin(const gs_wgrad_desc* d, const void* a1, const void* g1, const void* a2, const void* g2, float* dw,
                     float* ws, int64_t ws_floats, const gs_twin* tw, void* stream);
/* db[c] += sum over pixels of dy[pix, c]  (bias gradient of any conv) */
int gs_bias_grad(const void* dy, int64_t pixels, int32_t C, int32_t cs, int32_t co, float* db, void* stream);
/* deterministic form (per-chunk partial sums in a caller-owned workspace, added in chunk order) */
int64_t gs_bias_grad_ws_floats(int64_t pixels, int32_t C);
int gs_bias_grad_ws(const void* dy, int64_t pixels, int32_t C, int32_t cs, int32_t co, float* db, float* ws,
                    int64_t ws_floats, void* stream);
/* the same over the first 8 channels of the window, adding only db[0 .. c_valid), c_valid <= 8: a bias whose channel count is
 * not a multiple of 8 (the generators' 3-channel output conv, resnet2d.py:62-65) is followed by the next parameter in the flat
 * gradient buffer. Workspace: gs_bias_grad_ws_floats(pixels, 8) */
int gs_bias_grad_head_ws(const void* dy, int64_t pixels, int32_t cs, int32_t co, int32_t c_valid, float* db, float* ws,
                         int64_t ws_floats, void* stream);

/* ---- InstanceNorm + activation (nn.InstanceNorm2d eps=1e-5 affine=False, nn/utils.py:53-59) ------ */
/* partial [N][slots][2][C] -> mean_rstd [N][2][C] */
int gs_inorm_finalize(const float* partial, int32_t N, int32_t slots, int32_t C, int64_t hw, float eps,
                      float* mean_rstd, void* stream);
/* x = act((y-mean)*rstd) [+ res]   (resnet2d.py:26-27, 83-84, 87, 93) */
int gs_inorm_act_forward(const void* y, const float* mean_rstd, const void* res, void* x, int32_t N,
                         int64_t hw, int32_t C, int32_t act, float slope, void* stream);
/* The two calls above as ONE launch: every workgroup adds up the partial slots of its own 64 channels in its prologue,
 * the first pixel chunk's workgroups also write mean_rstd [N][2][C] (needed by the backward pass), then x is produced as
 * in gs_inorm_act_forward. (C % 64 != 0: falls back to the two launches.) */
int gs_inorm_stats_act_forward(const void* y, const float* partial, int32_t slots, float eps, float* mean_rstd,
                               const void* res, void* x, int32_t N, int64_t hw, int32_t C, int32_t act, float slope,
                               void* stream);
/* Backward of the above. g_pad is the incoming gradient on a domain padded by `fold` on each side of every
 * spatial axis with extent > 1 (the data-gradient of a reflect/replicate-padded conv; fold=0 for a plain gradient)
 * — the border is folded back here (adjoint of nn.ReflectionPad2d resnet2d.py:24 / nn.ReplicationPad3d
 * resnet3d.py:24,78). D = 1 for 2-D tensors. g2 (optional, unpadded) is added (residual join).
 * Outputs dy (gradient w.r.t. the conv output y) and optionally gsum = fold(g_pad)+g2 (skip path).
 * If mean_rstd is NULL there is no norm: `y` then holds the activation OUTPUT and dy = g*act'(y).
 * bias_grad (optional, norm only): db[c] += sum over pixels of dy — the gradient of the bias of the conv in front
 * of the norm, obtained from the reduction sums (it is identically zero up to rounding, like the reference's). */
int gs_inorm_act_backward(const void* g_pad, const void* g2, const void* y, const float* mean_rstd,
                          void* dy, void* gsum, float* scratch, float* bias_grad, int32_t N, int32_t D, int32_t H,
                          int32_t W, int32_t C, int32_t fold, int32_t fold_mode, int32_t act, float slope,
                          int32_t pre_slots, void* stream);
/* pre_slots > 0: `scratch` already holds the partial sums [N][pre_slots][3][C] (written by gs_gconv_forward_fused)
 * followed by room for the [N][3][C] totals; the reduction pass is skipped. */
int64_t gs_inorm_backward_scratch_floats(int32_t N, int32_t D, int32_t H, int32_t W, int32_t C);
/* gs_inorm_act_backward always leaves the per-image totals [N][3][C] (sum ghat, sum ghat*yhat, sum yhat) behind the
 * partial slots, at scratch + N * slots * 3 * C (slots = pre_slots, or the chunk count of its own reduction pass =
 * gs_inorm_backward_scratch_floats / (3 N C) - 1). An executor that passes bias_grad = NULL there can add the bias
 * gradients of ALL its norm layers with one launch afterwards: item i does db[c] += sum over images (in order) of
 * -rstd * S2 * S3 / hw. */
#define GS_NORM_DB_MAX 32
typedef struct gs_norm_db_item {
  const float* sums;        /* [N][3][C] totals left by gs_inorm_act_backward */
  const float* mean_rstd;   /* [N][2][C] */
  float* db;                /* [C], accumulated into */
  int32_t N, C;
  float inv_hw;             /* 1 / (D*H*W) */
  int32_t pad_;
} gs_norm_db_item;
int gs_norm_bias_grads(const gs_norm_db_item* items, int32_t count, void* stream);

/* Generalised form for skip-connection graphs (nn/generators/unet/unet2d.py:110-157): the normalised tensor is read
 * through up to two activations (LeakyReLU by the next down-conv, ReLU by the up-conv on the skip half of
 * torch.cat([x, y], 1)), outputs / gradient inputs are channel slices of wider concat buffers, and nn.Dropout(p) may sit
 * between the norm and the consumer's activation (mask = counter-based hash of (seed, image, element)).
 *   forward : v = drop(norm(y));  x1 = act1(v);  x2 = act2(v) (x2 optional)
 *   backward: ghat = mask/(1-p) * (g1*act1'(yhat) + g2*act2'(yhat)) (g2 optional), dy as in gs_inorm_act_backward.
 * mean_rstd == NULL: no norm, `y` holds a sign-preserving activation output. */
typedef struct gs_norm_ex_desc {
  int32_t N, H, W, C;
  int32_t act1, act2;          /* GS_ACT_* */
  float   slope;
  int32_t x1_cs, x1_co, x2_cs, x2_co;      /* forward outputs: channel stride / offset (elements) */
  int32_t g1_cs, g1_co, g2_cs, g2_co;      /* backward gradient inputs */
  float   drop_p;              /* 0 = no dropout */
  uint32_t seed_lo, seed_hi;   /* host part of the 64-bit mask seed */
  const uint32_t* seed_dev;    /* optional DEVICE part (2 words, lo/hi), added to the host part: lets a captured hipGraph
                                * of the step draw a fresh nn.Dropout mask per replay (unet2d.py:146-147) */
} gs_norm_ex_desc;
int gs_norm_act_forward_ex(const gs_norm_ex_desc* d, const void* y, const float* mean_rstd, void* x1, void* x2,
                           void* stream);
int gs_norm_act_backward_ex(const gs_norm_ex_desc* d, const void* g1, const void* g2, const void* y,
                            const float* mean_rstd, void* dy, float* scratch, float* bias_grad, void* stream);
int64_t gs_norm_backward_ex_scratch_floats(const gs_norm_ex_desc* d);

/* ---- V-Net elementwise family (nn/generators/vnet/vnet3d.py:155-267; memcnn.AdditiveCoupling via nn/invertible.py) ----
 * InstanceNorm3d(affine=False) -> [+ residual] -> nn.PReLU(C) -> [+ residual] on channel slices, and its backward incl.
 * the gradient of the learnable slope:
 *   forward : u = norm(y) (mean_rstd == NULL: u = y);  res_mode 1: u += res;  v = u > 0 ? u : slope[c]*u (slope == NULL:
 *             v = u);  res_mode 2: v += res;  res_mode 3: v = res - v (the inverse of an additive coupling, x = y - F(.),
 *             memcnn AdditiveCoupling.inverse through nn/invertible.py:21-24);  out = v
 *   backward: gt = g (+ g2), negated for res_mode 3;  gu = gt*(u > 0 ? 1 : slope[c]);  dslope[c] += sum gt*min(u, 0);  gres = gu (optional);
 *             dy = rstd*(gu - mean gu - yhat*mean(gu*yhat)) (no norm: dy = gu);  bias_grad[c] += sum over pixels of dy
 * res_mod > 0: channel c reads residual channel c % res_mod (InputBlock's x.repeat, vnet3d.py:162-167). */
typedef struct gs_pnorm_desc {
  int64_t pixels;                           /* D*H*W of one image */
  int32_t N, C;                             /* C multiple of 8 */
  int32_t y_cs, y_co;                       /* channel stride / offset (elements) of every operand view */
  int32_t res_mode, res_cs, res_co, res_mod;
  int32_t out_cs, out_co;
  int32_t g_cs, g_co, g2_cs, g2_co;
  int32_t dy_cs, dy_co, gres_cs, gres_co;
} gs_pnorm_desc;
int gs_pnorm_forward(const gs_pnorm_desc* d, const void* y, const float* mean_rstd, const void* res, const float* slope,
                     void* out, void* stream);
int gs_pnorm_backward(const gs_pnorm_desc* d, const void* g, const void* g2, const void* y, const float* mean_rstd,
                      const void* res, const float* slope, void* dy, void* gres, float* dslope, float* bias_grad,
                      float* scratch, void* stream);
int64_t gs_pnorm_backward_scratch_floats(const gs_pnorm_desc* d);
/* dst[view] = src[view] (accumulate == 0) or dst[view] += src[view]: gradient joins (out + down, torch.cat skip halves,
 * vnet3d.py:198-200,239-243) */
int gs_add_views(void* dst, int32_t dst_cs, int32_t dst_co, const void* src, int32_t src_cs, int32_t src_co,
                 int64_t pixels, int32_t C, int32_t accumulate, void* stream);
/* adjoint of x.repeat(1, C/Cin, 1, 1, 1): g_img[n][c0][pix] += sum over c = c0 (mod Cin) of g[pix][c] */
int gs_repeat_backward(const void* g, int32_t g_cs, int32_t g_co, float* g_img, int32_t N, int32_t Cin, int32_t C,
                       int64_t pixels, void* stream);

/* ---- network boundary: NCHW fp32 images <-> NHWC bf16 activations ------------------------------- */
/* x NCHW fp32 [N,C,H,W] -> act [N,H,W,Cp]  (set_input, cyclegan.py:84-90) */
int gs_image_to_act(const float* img, void* act, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                    void* stream);
/* Channel sources: K (1..GS_CAT_MAX_SRCS) image tensors side by side along the channel axis -> act in one pass. Source k is a
 * channel window of a dense fp32 [N][C_k][S] tensor (S = D*H*W): src[k] points at the window's first element (c0 * S floats
 * into the tensor), sample_stride[k] = C_k * S floats lead from one sample to the next, channels[k] is the window's width.
 * src, sample_stride and channels are HOST arrays of K that reach the kernel by value; no source needs any alignment. Rounding
 * and the zeroed pad lanes are gs_image_to_act's. One windowed source is a discriminator's real input real_B[:, tB], two are
 * the splice torch.cat([fake_Bt, real_A[:, guide]], dim=1) of the balanced CycleGAN, two whole tensors the conditional
 * discriminator's input torch.cat([real_A, fake_B], dim=1) (pix2pix.py:70,80). */
#define GS_CAT_MAX_SRCS 4
int gs_image_cat_to_act(const float* const* src, const int64_t* sample_stride, const int32_t* channels, int32_t K, void* act,
                        int32_t N, int64_t S, int32_t Cp, void* stream);
/* its gradient: for every source with grad[k] != NULL its channels of g as a dense fp32 [N][channels[k]][S] tensor; a NULL
 * grad[k] is skipped (nothing of it is written), at least one must be given */
int gs_image_cat_to_act_backward(const void* g, float* const* grad, const int32_t* channels, int32_t K, int32_t N, int64_t S,
                                 int32_t Cp, void* stream);
/* dst [N][C][S] = zeros with src [N][t][S] at channels [c0, c0 + t); every element of dst is written once. N * C <= 65535 */
int gs_channel_embed(const float* src, float* dst, int32_t N, int32_t C, int32_t c0, int32_t t, int64_t S, void* stream);
/* act -> NCHW fp32, optional tanh (resnet2d.py:65) */
int gs_act_to_image(const void* act, float* img, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp,
                    int32_t act_kind, void* stream);
/* gradient of gs_act_to_image: g_img NCHW fp32, out = forward output image (for tanh') -> g_act */
int gs_act_to_image_backward(const float* g_img, const float* out_img, void* g_act, int32_t N, int32_t C,
                             int32_t H, int32_t W, int32_t Cp, int32_t act_kind, void* stream);
/* gradient of gs_image_to_act composed with the first conv's padding fold: g_pad act (padded by fold)
 * -> NC(D)HW fp32 image gradient; accumulate != 0 adds into g_img. A reflect fold needs every folded extent (H, W, and D
 * when D > 1) > fold, a replicate fold <= 3. The other three boundary functions are layout-only: a volume goes through them
 * with H := D*H. */
int gs_image_to_act_backward(const void* g_pad, float* g_img, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                             int32_t Cp, int32_t fold, int32_t fold_mode, int32_t accumulate, void* stream);

/* ---- "W-fold" of the k7 boundary convolutions (resnet2d.py:24-25,64-65; resnet3d.py:24-25,64) --------------------
 * A conv with 1-3 input (stem) or output (last layer) channels wastes the 16-wide matrix tile, so the taps of the W
 * axis are moved into the channel axis and the conv itself runs with a k x [k x] 1 kernel through gs_gconv_forward /
 * gs_wgrad; these are the boundary transforms and their adjoints. `rows` = D*H of a volume (or H of an image).
 *   unfold   : act[n, r, j][dw*C + c] = img[n][c][r][B(j + dw - p)], channels >= k*C zero (fused NCHW fp32 -> NHWC bf16)
 *   shift-add: img[n][co][r][j] = act(bias[co] + sum_dw z[n, r, j + dw][dw*Co + co]),  z is W + k - 1 wide
 * A reflect border needs W > p and W > k - 1 - p (and, in the adjoint, H > fold, D > fold when D > 1). */
int gs_image_unfold(const float* img, void* act, int32_t N, int32_t C, int64_t rows, int32_t W, int32_t Qp, int32_t k,
                    int32_t p, int32_t border, void* stream);
/* adjoint of gs_image_unfold composed with the (depth, row) padding fold of the stem conv: g is the data gradient of the
 * transformed conv on the domain padded by `fold` along depth (D > 1) and rows, W unpadded */
int gs_image_unfold_backward(const void* g, float* g_img, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                             int32_t Qp, int32_t k, int32_t p, int32_t fold, int32_t border, int32_t accumulate,
                             void* stream);
int gs_shiftadd_to_image(const void* z, const float* bias, float* img, int32_t N, int32_t Co, int64_t rows, int32_t W,
                         int32_t Pp, int32_t k, int32_t act_kind, void* stream);
/* gz[n, r, j'][dw*Co + co] = g_img[n][co][r][j' - dw] * act'(out) (zero outside [0, W)), channels >= k*Co zero */
int gs_shiftadd_to_image_backward(const float* g_img, const float* out_img, void* gz, int32_t N, int32_t Co,
                                  int64_t rows, int32_t W, int32_t Pp, int32_t k, int32_t act_kind, void* stream);

/* Partial InstanceNorm statistics of a channel slice [co, co + C) of an activation tensor with channel stride cs — for a
 * norm whose input is not a conv output (the pre-norm of Piresnet3D's coupling function, piresnet3d.py:104-108):
 * partial [N][slots][2][C] with slots = gs_slice_stats_slots(pixels), finalised by gs_inorm_finalize. */
int32_t gs_slice_stats_slots(int64_t pixels);
int gs_slice_stats(const void* x, int32_t N, int64_t pixels, int32_t cs, int32_t co, int32_t C, float* partial,
                   void* stream);

/* ---- device-side image preprocessing --------------------------------------------- */
/* What ganslate/data/utils/transforms.py:9-61 composes on the host from torchvision / PIL for the image-folder datasets
 * (unpaired_image_dataset.py:31-62, paired_image_dataset.py): Resize(load_size, Image.BICUBIC) / scale_width / random_zoom, RandomCrop(final_size),
 * RandomHorizontalFlip, ToTensor, Normalize(0.5, 0.5) — here on decoded 8-bit HWC images (C = 1 or 3) in device memory.
 * The resize is Pillow's two-pass 8-bit resampler bit for bit (src/libImaging/Resample.c): the caller supplies, per axis,
 * bounds[out][2] = (first input index, count) and kk[out][ksize] = 22-bit fixed-point coefficients
 * (precompute_coeffs + normalize_coeffs_8bpc; identity tables when an axis keeps its size).
 * Pass 1, horizontal: out[y][xx][c] = clip8((2^21 + sum_k in[y][xmin+k][c] * kk[xx][k]) >> 22), all in_h rows. */
int gs_u8_resample_h(const void* in, void* out, int32_t in_h, int32_t in_w, int32_t out_w, int32_t C,
                     const int32_t* bounds, const int32_t* kk, int32_t ksize, void* stream);
/* Pass 2 as a plain 8-bit image (out_h x w): the intermediate of two consecutive resizes — `scale_width` / `resize` followed by
 * `random_zoom` (transforms.py:22-37,127-137,163-169). */
int gs_u8_resample_v(const void* tmp, void* out, int32_t tmp_h, int32_t w, int32_t out_h, int32_t C, const int32_t* bounds,
                     const int32_t* kk, int32_t ksize, void* stream);
/* Pass 2, vertical, only for the crop window [top, top+fh) x [left, left+fw) of the out_h x tmp_w resized image, then flip,
 * x/255 and (x-0.5)/0.5 in torchvision's fp32 order: out[c][i][j] (planes of fh*fw floats — a slice of the NCHW batch). */
int gs_u8_resample_v_crop_normalize(const void* tmp, float* out, int32_t tmp_h, int32_t tmp_w, int32_t out_h, int32_t C,
                                    const int32_t* bounds, const int32_t* kk, int32_t ksize, int32_t top, int32_t left,
                                    int32_t fh, int32_t fw, int32_t flip, void* stream);

/* The same two passes for a whole batch of decoded images of different sizes, one launch per pass (the val / test / infer
 * engines push folders through at batch sizes where launches, allocations and copies per image dominate). One descriptor
 * per image, in a device array; the pointers are device pointers. The horizontal pass computes only the input rows
 * [row0, row0 + rows) that the vertical pass of the crop rows [top, top + fh) reads (bounds_v[top].first up to
 * bounds_v[top+fh-1].first + count) into tmp + tmp_off, rows x rw x C bytes; the vertical pass indexes that slice
 * relative to row0 and writes image i of the fp32 [n][C][fh][fw] batch. Arithmetic, rounding and operation order are those
 * of the per-image entry points above. */
typedef struct GsU8BatchItem {
  const void* src;              /* in_h x in_w x C bytes, HWC */
  const int32_t* bounds_h;      /* [rw][2], kk_h [rw][ksize_h]: in_w -> rw */
  const int32_t* kk_h;
  const int32_t* bounds_v;      /* [rh][2], kk_v [rh][ksize_v]: in_h -> rh */
  const int32_t* kk_v;
  int64_t tmp_off;              /* byte offset of this image's slice of the tmp arena */
  int32_t in_h, in_w, rh, rw;   /* decoded size, resized size */
  int32_t row0, rows;           /* input rows the horizontal pass computes */
  int32_t top, left, flip;      /* crop window origin in the resized image; horizontal flip of the window */
  int32_t ksize_h, ksize_v, pad_;
} GsU8BatchItem;
/* Host-side validation of a descriptor table BEFORE it is uploaded (the kernels cannot report a bad descriptor): `items` is
 * a HOST array here. Every pointer non-null, sizes positive, the fh x fw crop window inside the rh x rw resized image,
 * [row0, row0 + rows) inside [0, in_h), every tmp slice inside [0, tmp_bytes). */
int gs_u8_batch_check(const GsU8BatchItem* items, int32_t n, int32_t C, int32_t fh, int32_t fw, int64_t tmp_bytes);
/* items: DEVICE array of n descriptors; grid_w >= every rw, grid_rows >= every rows (blocks outside their image's extent
 * return); grid (ceil(grid_w / 256), grid_rows, n). */
int gs_u8_batch_resample_h(const GsU8BatchItem* items, int32_t n, int32_t C, void* tmp, int32_t grid_w, int32_t grid_rows,
                           void* stream);
/* grid (ceil(fw / 256), fh, n): out[i][c][y][x] fp32. */
int gs_u8_batch_resample_v_crop_normalize(const GsU8BatchItem* items, int32_t n, int32_t C, const void* tmp, int32_t fh,
                                          int32_t fw, float* out, void* stream);

/* ---- device-side multi-modal 2-D samples (csrc/imgstack.hip) --------------------------------------- */
/* What the reference's ClearGrasp datasets do per modality on the host (projects/cleargrasp_depth_estimation/datasets/
 * train_dataset.py:75-146, val_test_dataset.py:80-167): transforms.Resize(load_size, BICUBIC) on the fp32 tensor — torch's
 * bicubic interpolation without antialiasing, cubic convolution A = -0.75, align_corners = False — clamp to the modality's
 * range, min-max to [-1, 1], one noise plane on domain B's RGB, concat along channels; here one launch builds a whole fp32
 * [N][C][H][W] batch from decoded images resident in device memory as stored. One descriptor per (sample, modality), in a
 * device array; the pointers are device pointers. Tap tables of an axis n_in -> n_out: idx[o][4] the source indices
 * f-1 .. f+2 clamped to [0, n_in - 1] and w[o][4] their weights c2(t+1), c1(t), c1(1-t), c2(2-t), with
 * s = (o + 0.5) * n_in / n_out - 0.5, f = floor(s), t = s - f, computed by the caller in float64 and rounded once to
 * fp32 (rows of 16 bytes, 16-byte aligned); the kernel computes no coordinate. Per element, fp32:
 *   r = sum_j w_y[y][j] * sum_i w_x[x][i] * src[idx_y[y][j]][idx_x[x][i]][ch];  v = min(max(r, lo), hi);
 *   rescale != 0: v = (v - lo) / (hi - lo), v = 2 v - 1;
 *   noise_std > 0: v = min(max(v + noise_std * z, -1), 1), z = sqrt(-2 ln u1) * cos(2 pi u2) with
 *   u1 = ((r0 >> 9) + 0.5) * 2^-23, u2 = (r1 >> 8) * 2^-24 from the first two words of Philox4x32-10 on the counter
 *   (y * W + x, 0, 0, 0) and the key (key0, key1): the channels of a descriptor share the plane.
 * src == NULL: the descriptor's c channels are written as zeros (tables and source fields unused). */
enum { GS_IMG_U8 = 0, GS_IMG_F32 = 1 };
typedef struct GsImgStackItem {
  const void* src;              /* in_h x in_w x c (hwc != 0) or c x in_h x in_w (hwc == 0) elements of `dtype`, or NULL */
  const int32_t* idx_y;         /* [H][4], w_y [H][4]: in_h -> H */
  const float* w_y;
  const int32_t* idx_x;         /* [W][4], w_x [W][4]: in_w -> W */
  const float* w_x;
  int32_t dtype, hwc;
  int32_t in_h, in_w, c;        /* stored size, channels of the modality */
  int32_t item, c0;             /* batch item and first output channel: out[item][c0 .. c0 + c) */
  int32_t rescale;              /* 0: clamp only */
  float lo, hi, noise_std;
  uint32_t key0, key1;          /* Philox key of the noise plane */
  int32_t pad_;
} GsImgStackItem;
/* Host-side validation of a descriptor table BEFORE it is uploaded (the kernel cannot report a bad descriptor): `items` is a
 * HOST array here. Batch item inside [0, N), channels [c0, c0 + c) inside [0, C), every channel of every batch item written
 * by exactly one descriptor; with a source: tables non-null, sizes positive, dtype known, lo < hi, noise_std >= 0. */
int gs_img_stack_check(const GsImgStackItem* items, int32_t n, int32_t N, int32_t C, int32_t H, int32_t W);
/* items: DEVICE array of n descriptors; grid (ceil(W / 256), H, n); out: N * C * H * W floats, each written once. */
int gs_img_stack(const GsImgStackItem* items, int32_t n, float* out, int32_t N, int32_t C, int32_t H, int32_t W,
                 void* stream);

/* ---- device-side 3-D training patches ------------------------------------------- */
/* What the 3-D datasets' workers do per sample on the host (projects/brats_mri_sequence_translation/datasets/
 * train_dataset.py:83-86 -> ganslate/data/utils/normalization.py:18-30): out = z_score_normalize(volume[z:z+d, y:y+h,
 * x:x+w], scale_to_range=(lo, hi)) — t = (v - mean) / std with the patch's own mean and unbiased std, then
 * (hi - lo) * (t - min t) / (max t - min t) + lo when rescale != 0 — on a dense D x H x W volume resident in device
 * memory (dtype GS_VOL_F32 or GS_VOL_I16). start / size: host arrays {z, y, x} / {d, h, w}; out: d*h*w floats;
 * scratch: gs_patch_zscore_ws_floats() floats, 8-byte aligned, private to the launch. A constant patch gives NaN, as in
 * the reference. The start coordinates come from data/utils/stochastic_focal_patching.py (host RNG). */
enum { GS_VOL_F32 = 0, GS_VOL_I16 = 1 };
int64_t gs_patch_zscore_ws_floats(void);
int gs_patch_zscore(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                    const int32_t* size, int32_t rescale, float lo, float hi, float* out, float* scratch, void* stream);

/* ---- device-side multi-modal patch sampling (csrc/volsample.hip) ---------------------------------- */
/* The training-patch path of the reference's HX4-PET dataset (projects/maastro_hx4_pet_translation/datasets/
 * train_dataset.py, datasets/utils/patch_samplers.py, basic.py) on volumes and body masks resident in device memory.
 *
 * gs_voxel_draw draws one patch centre ("focal point") of a dense D x H x W case. mask: uint8, non-zero = body.
 * weight: NULL (uniform schemes) or a volume of dtype GS_VOL_F32 / GS_VOL_I16 (weighted schemes). patch: host {d, h, w}.
 * The valid zone of an axis is [floor(p / 2), size - ceil(p / 2)), upper bound exclusive; the weight of a voxel of the
 * zone is (mask != 0) for mask-only draws and (mask != 0) * max(w, 0) for weighted ones (NaN counts as 0). With u in
 * [0, 1), over the zone in C order:
 *   mask-only: count = non-zero voxels, k = min((int64)floor(u * count), count - 1) in float64; the k-th non-zero voxel;
 *   weighted:  C_i = float64 inclusive prefix sums, T their total; the first voxel with C_i > u * T, else the last voxel
 *              of positive weight.
 * This picks the voxel np.random.choice(p = map / map.sum()) picks from the same uniform. Mask-only draws are integer
 * exact; weighted sums are taken in a fixed order (per run, per range, then over ranges), so a draw is bitwise
 * reproducible, and equal to the C-order rule whenever the sums are exact.
 * focal_a != NULL makes it the stochastic-focal draw of domain B: focal_a is a DEVICE int32[3] holding the point drawn in
 * A, dims_a (host int32[3]) A's dims, proportion (host double[3]) the focal region proportions. In float64, per axis:
 * f = (focal_a / dims_a) * size; region = (int)(proportion * size); box = [max((int)(f - region / 2), 0),
 * min((int)(f + region / 2), size)). The draw is over zone ∩ body ∩ box; if that is empty, over zone ∩ body and
 * out[3] = 1.
 * out: device int32[4] = {z, y, x, fallback_used}; {-1, -1, -1, flag} when the set is empty or its total weight is 0.
 * ws: gs_voxel_draw_ws_bytes() bytes, 8-byte aligned, private to the launch. No atomics, no host synchronisation.
 * gs_voxel_draw_range_len: voxels of the zone's box each of the 256 workgroups of the first pass owns (for tests that
 * aim at range boundaries); 0 for an empty zone. */
int64_t gs_voxel_draw_ws_bytes(void);
int64_t gs_voxel_draw_range_len(int32_t D, int32_t H, int32_t W, const int32_t* patch);
int gs_voxel_draw(const uint8_t* mask, const void* weight, int32_t wdtype, int32_t D, int32_t H, int32_t W,
                  const int32_t* patch, double u, const int32_t* focal_a, const int32_t* dims_a, const double* proportion,
                  int32_t* out, void* ws, void* stream);
/* gs_patch_clip_minmax: crop + normalise all C (1..GS_PATCH_MAX_MODALITIES) modalities of one case in one launch.
 * vols / dtypes: host tables of C device volumes (all D x H x W) and their GS_VOL_* dtypes; mask: the case's body mask;
 * point: DEVICE int32[3], the focal point; start = point - floor(patch / 2), clamped to [0, size - patch] per axis, so no
 * point can make the kernel read outside a volume. outside / divisor / lo / hi: host float[C]. Per voxel, in fp32 with
 * one IEEE operation per step:
 *   v = mask ? (float)x : outside;  v = v / divisor;  v = min(max(v, lo), hi);  v = (v - lo) / (hi - lo);  v = 2 * v - 1
 * (np.where(body_mask, image, fill), the per-case divisor, torch.clamp, min_max_normalize). out: dense [C, d, h, w] fp32.
 * Shape, pointer, dtype, empty-range and zero-divisor errors are refused before the launch. */
#define GS_PATCH_MAX_MODALITIES 8
int gs_patch_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask, int32_t D,
                         int32_t H, int32_t W, const int32_t* patch, const int32_t* point, const float* outside,
                         const float* divisor, const float* lo, const float* hi, float* out, void* stream);
/* Random affine augmentation of a training patch: one trilinear gather through a 3 x 3 matrix, in the launch that crops.
 * THE DEFINITION (data/utils/patch_affine.py states it in numpy, tests/patch_affine_ref.py as a per-voxel loop). For a
 * dense volume of size (D, H, W), a patch p = (d, h, w) starting at `start`, and M (host double[9], row-major, maps patch
 * offsets to source offsets; data/utils/patch_affine.py affine_matrix builds it from flips, angles, zoom and spacing):
 *   c_a = (p_a - 1) / 2                                                               float64, exact
 *   r = o - c for output voxel o                                                      float64, exact
 *   s_a = ((M[a][0] r_0 + M[a][1] r_1) + M[a][2] r_2) + (start_a + c_a)               float64, one IEEE operation per step,
 *                                                                                     no fused multiply-add
 *   i_a = floor(s_a), t_a = (float)(s_a - i_a)
 *   if any s_a < -1 or s_a >= size_a (float64, before any integer conversion; a NaN s_a counts as such): all eight
 *   corners are outside
 *   corner (i_0 + dz, i_1 + dy, i_2 + dx) has the value (float)vol[corner] when it lies inside the volume and, with a
 *   mask, mask[corner] != 0; otherwise the `outside` value (mask, then interpolate: continuous, no nearest-neighbour
 *   rounding)
 *   lerp(a, b, t) = a + t * (b - a) in float32: sub, mul, add, each rounded; along W first (c00, c01, c10, c11), then
 *   along H, then along D
 * M = I gives the plain crop, M = diag(+-1) the flipped crop, a signed permutation matrix on a patch with equal sides in
 * the rotated plane np.rot90 of the crop — as equal numbers (a zero may come out with the other sign: an upper corner of
 * weight 0 still enters as 0 * (b - a)).
 *
 * gs_patch_affine_clip_minmax: the gather, then the per-voxel chain of gs_patch_clip_minmax unchanged (/ divisor, clamp,
 * min-max to [-1, 1]) for all C (1..GS_PATCH_MAX_MODALITIES) modalities of one case. Arguments as gs_patch_clip_minmax
 * (point: DEVICE int32[3]; start = point - floor(patch / 2) clamped to [0, size - patch]) plus M. out: dense
 * [C, d, h, w] fp32, every element written exactly once.
 * gs_patch_affine: the raw gather of one volume, no mask, no normalisation, `fill` outside the volume; start / size: host
 * int32[3], the window inside the volume as for gs_patch_zscore. out: [d, h, w] fp32 — a dense patch that
 * gs_patch_zscore then takes as a volume of its own with start 0 (UnpairedVolumeDataset's z-score follows the gather).
 * One thread per output voxel, W fastest: coordinates, in-bounds tests and the eight mask bytes once per voxel, the
 * modalities looped inside the thread. M and the per-modality constants travel in the kernel argument. No atomics, no
 * workspace, no host synchronisation. Null pointers, C out of range, non-positive sizes, a patch larger than the volume
 * on any axis (or, for gs_patch_affine, a window that leaves it), an unknown dtype, a non-finite entry of M, lo >= hi and
 * a zero or NaN divisor are refused before any launch. */
int gs_patch_affine_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask, int32_t D,
                                int32_t H, int32_t W, const int32_t* point, const int32_t* patch, const double* M,
                                const float* outside, const float* divisor, const float* lo, const float* hi, float* out,
                                void* stream);
int gs_patch_affine(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                    const int32_t* size, const double* M, float fill, float* out, void* stream);
/* Elastic deformation inside the same gather: a free-form deformation, i.e. a coarse lattice of control-point
 * displacements interpolated by uniform cubic B-splines and aligned with the patch, added to the patch offset BEFORE the
 * matrix is applied — the two compose as maps, in one launch, without an intermediate volume.
 * THE DEFINITION (data/utils/patch_affine.py states it in numpy, tests/patch_elastic_ref.py as a per-voxel loop).
 *   lattice G = (G_0, G_1, G_2) control points per axis (D, H, W), every G_a >= 4, G_0 G_1 G_2 <= GS_ELASTIC_MAX_POINTS
 *   field   PHI[a][i][j][k], float64, C order: component a of the displacement at control point (i, j, k), already in
 *           voxels of axis a (millimetres / spacing[a] on the host)
 *   patch   p = (d, h, w), every p_a >= 2; the extent [0, p_a - 1] spans the G_a - 3 inner intervals of the lattice
 * Per output voxel o and axis a, in integers:
 *   num = o_a (G_a - 3),  den = p_a - 1,  j_a = min(num / den, G_a - 4) (integer division),
 *   f = (double)(num - j_a den) / (double)den      one correctly rounded float64 division of two exact integers; the last
 *                                                  voxel of an axis gets j_a = G_a - 4, f = 1
 * Basis weights in float64, one IEEE operation per step, no fused multiply-add:
 *   f2 = f f,  f3 = f2 f,  g = 1 - f
 *   B0 = ((g g) g) / 6,  B1 = ((3 f3 - 6 f2) + 4) / 6,  B2 = (((3 f2 - 3 f3) + 3 f) + 1) / 6,  B3 = f3 / 6
 * Displacement component a — innermost over D (weights Bz of axis 0), then H (By), outermost over W (Bx), every sum left
 * to right with separate multiply and add:
 *   q[m][n] = ((Bz0 PHI[a][j_0][j_1 + m][j_2 + n] + Bz1 PHI[a][j_0 + 1][..]) + Bz2 PHI[a][j_0 + 2][..]) + Bz3 PHI[a][j_0 + 3][..]
 *   R[n]    = ((By0 q[0][n] + By1 q[1][n]) + By2 q[2][n]) + By3 q[3][n]
 *   u_a     = ((Bx0 R[0] + Bx1 R[1]) + Bx2 R[2]) + Bx3 R[3]
 * r'_a = r_a + u_a (one float64 add), and s_a = ((M[a][0] r'_0 + M[a][1] r'_1) + M[a][2] r'_2) + (start_a + c_a) onwards
 * is the affine definition above, unchanged: floor, t, the reach test, masked corners, the three float32 lerps — with one
 * addition: t_a = 0 on an axis whose s_a fails the reach test. For a finite s_a that changes no bit (the eight corners are
 * all the outside value, which every finite t lerps to itself); for a NaN or infinite s_a, where s_a - i_a is no number,
 * it makes the result that same value. So a NaN or infinite displacement gives a NaN or out-of-range coordinate, by the
 * reach rule "all eight corners outside": the voxel takes the outside value and nothing is read out of bounds. A zero
 * field is the affine gather bit for bit.
 * The order is chosen so that R[n] of a lattice column depends on (o_0, o_1) only: the kernel computes it once per output
 * row a workgroup covers (into LDS) and every voxel of the row reads it — the same bits as the per-voxel evaluation,
 * which is what it launches instead when that row table passes 32 KB of LDS (the option elastic_rows): rows of a few
 * voxels under a wide lattice. The divisions and weights reproduce between hipcc and numpy, so no host-built tables are involved.
 *
 * gs_patch_elastic_clip_minmax / gs_patch_elastic: gs_patch_affine_clip_minmax / gs_patch_affine plus grid (host
 * int32[3] = G) and field (DEVICE double[3 G_0 G_1 G_2], read through L2 or staged to LDS, never modified). They refuse
 * everything the affine entries refuse and, before any launch, a null grid or field, any G_a < 4, more than
 * GS_ELASTIC_MAX_POINTS control points, any p_a < 2, and (p_a - 1) (G_a - 3) beyond int32. */
#define GS_ELASTIC_MAX_POINTS 1024
int gs_patch_elastic_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask, int32_t D,
                                 int32_t H, int32_t W, const int32_t* point, const int32_t* patch, const double* M,
                                 const int32_t* grid, const double* field, const float* outside, const float* divisor,
                                 const float* lo, const float* hi, float* out, void* stream);
int gs_patch_elastic(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                     const int32_t* size, const double* M, const int32_t* grid, const double* field, float fill, float* out,
                     void* stream);
/* Intensity augmentation in the same launches: a smooth multiplicative bias field, contrast and brightness, gamma and
 * additive Gaussian noise, applied to the value the patch kernels hold in a register just before they store it.
 * THE DEFINITION (data/utils/patch_intensity.py states it in numpy, tests/patch_intensity_ref.py as a per-voxel loop).
 * The chain acts on the normalised value n that both normalisations form:
 *   clip / min-max chain:  n = (v - lo) / (hi - lo), between that step and 2 n - 1
 *   z-score with rescale:  t = (v - mean) / std, n = (t - min t) / (max t - min t); the last step is then
 *                          (hi - lo) * n + lo, one multiply and one add
 * Per modality one GsPatchIntensity. All arithmetic is fp32, one IEEE operation per step, no fused multiply-add; voxel
 * i is the linear index of the output voxel in its [d, h, w] patch, c its channel (0 for the z-score entry).
 *   1. bias != 0:  beta = the cubic B-spline interpolation at the voxel of ONE scalar lattice BETA[i][j][k] (float64, C
 *      order, G = bias_grid, aligned with the patch), exactly as one component of the elastic field above: the same num /
 *      den / j / f, the same weights, D innermost, then H, W outermost, every sum left to right.
 *      m = (float)(1.0 + (double)bias * beta), one float64 multiply and one float64 add;  n = n * m
 *   2. contrast != 1 or brightness != 0:  n = (((n - 0.5) * contrast) + 0.5) + brightness
 *   3. n = n < 0 ? 0 : n;  n = n > 1 ? 1 : n          (NaN stays NaN)
 *   4. gamma != 1:  n = powf(n, gamma) — the one step whose bits the host restatement and the device need not share
 *   5. noise_std > 0:  n = n + noise_std * z, z = sqrt(-2 ln u1) * cos(2 pi u2) as in gs_img_stack, u1 and u2 from the
 *      first two words of Philox4x32-10 on the counter (i & 0xffffffff, i >> 32, c, 0) and the key (key0, key1)
 *   6. step 3 again
 * A step whose parameters are neutral is skipped, not evaluated ((n - 0.5) + 0.5 is not n for a small n), and the clamps
 * change no bit of a value in [0, 1]: a neutral descriptor gives the bits of gs_patch_elastic_clip_minmax /
 * gs_patch_affine_clip_minmax. (gs_patch_zscore rounds (hi - lo) * (t - min t) / (max t - min t) in another order than
 * (hi - lo) * n; a neutral sample takes gs_patch_zscore.) The lattice is shared by the modalities of a launch, each
 * scales it by its own bias. A NaN lattice entry gives NaN inside its 4 x 4 x 4 support and nothing outside; a constant
 * z-score patch gives NaN as in gs_patch_zscore.
 *
 * gs_patch_augment_clip_minmax: gs_patch_elastic_clip_minmax with grid / field nullable together (null: the affine
 * gather) plus intensity (HOST array of C descriptors, copied into the kernel argument), bias_grid (host int32[3],
 * nullable) and bias_field (DEVICE double[G_0 G_1 G_2], nullable, never modified). beta is evaluated once per voxel in
 * front of the modality loop in the two forms of the elastic part, by the size of the combined row table against the
 * option elastic_rows; the forms give the same bits. The elastic and the bias lattice may have different grids.
 * gs_patch_zscore_intensity: gs_patch_zscore with rescale plus the same three arguments (one descriptor): the stats
 * and finalize launches unchanged, then an apply pass that stages the lattice in LDS per workgroup.
 * Both refuse, before any launch, what their base entries refuse and: a null intensity; a gamma that is not positive and
 * finite; a contrast or noise_std that is negative or not finite; a brightness that is not finite; |bias| >= 1 or NaN;
 * a non-zero bias without bias_grid / bias_field (and one of the two without the other); for bias_grid what the elastic
 * entries refuse for grid. No atomics, no further workspace, no host synchronisation; every output element is written
 * exactly once. */
typedef struct {
  float gamma, contrast, brightness, noise_std, bias;
  uint32_t key0, key1;
  int32_t pad_;
} GsPatchIntensity;
int gs_patch_augment_clip_minmax(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* mask, int32_t D,
                                 int32_t H, int32_t W, const int32_t* point, const int32_t* patch, const double* M,
                                 const int32_t* grid, const double* field, const GsPatchIntensity* intensity,
                                 const int32_t* bias_grid, const double* bias_field, const float* outside,
                                 const float* divisor, const float* lo, const float* hi, float* out, void* stream);
int gs_patch_zscore_intensity(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, const int32_t* start,
                              const int32_t* size, float lo, float hi, const GsPatchIntensity* intensity,
                              const int32_t* bias_grid, const double* bias_field, float* out, float* scratch, void* stream);
/* gs_volume_prepare: one whole case for the val / test engines (the reference's val_test_dataset.py:136-161): body
 * masking, centred padding to a target shape and the per-voxel chain of gs_patch_clip_minmax, for all C
 * (1..GS_PATCH_MAX_MODALITIES) volumes and M (1..1 + GS_VM_MAX_LABELS) byte masks of a D x H x W case. masks[0] is the
 * body mask (non-zero = inside), masks[1..] are further region masks. target: host {Dt, Ht, Wt}; the output size of an
 * axis is max(size, target), pad = output - size, pad / 2 voxels in front and pad / 2 + pad % 2 behind (integer
 * division), as ganslate/data/utils/ops.py pad() does. Per volume c, in fp32, one IEEE operation per step:
 *   x = masks[0] ? (float)v : outside[c];    pad voxels: x = min of x over the whole case (NaN if any x is NaN, like
 *   np.min);    x = x / divisor;  x = min(max(x, lo), hi);  x = (x - lo) / (hi - lo);  x = 2 * x - 1
 * out: dense fp32 [C, Do, Ho, Wo]. masks_out[m]: dense bytes [Do, Ho, Wo] = masks[m] copied, padded with its own
 * minimum byte. Two launches: per-block partial minima of every volume and mask (256 blocks each, skipped when no axis is
 * padded), then the apply pass, whose workgroups each fold the 256 partials in index order. No atomics, no host
 * synchronisation. ws: gs_volume_prepare_ws_bytes() bytes, 4-byte aligned, private to the call. Null pointers, C or M
 * out of range, non-positive sizes, an empty clip range, a zero or NaN divisor and a dtype other than GS_VOL_F32 /
 * GS_VOL_I16 are refused before any launch. */
int64_t gs_volume_prepare_ws_bytes(void);
int gs_volume_prepare(const void* const* vols, const int32_t* dtypes, int32_t C, const uint8_t* const* masks, int32_t M,
                      int32_t D, int32_t H, int32_t W, const int32_t* target, const float* outside, const float* divisor,
                      const float* lo, const float* hi, float* out, uint8_t* const* masks_out, void* ws, void* stream);

/* ---- patient body mask from a CT (csrc/bodymask.hip) ---------------------------------------------- */
/* The reference's ganslate/data/utils/body_mask.py without its contour smoothing. For a dense D x H x W volume v (dtype
 * GS_VOL_F32 or GS_VOL_I16) and a threshold t (compared in fp32; int16 values are exact in fp32):
 *   1. b = v >= t; a NaN voxel is outside.
 *   2. components of b under 6-connectivity (scipy.ndimage.label's default structure).
 *   3. the component with the most voxels; ties go to the component whose first voxel in C order comes first.
 *   4. per depth slice, every pixel that is NOT a non-component pixel 4-connected to the slice's border through
 *      non-component pixels (scipy.ndimage.binary_fill_holes per slice): holes are filled, a cavity that opens to the
 *      border in a slice stays open in that slice, a hole that touches the outside only diagonally is filled.
 *   5. no voxel reaches t: an all-zero mask and a count of 0.
 * mask_out: D*H*W bytes of 0 / 1. info: DEVICE int32[2] = {voxels of the chosen component, flat index of its first voxel
 * in C order or -1}. All quantities are integers, so the result is exact and the same on every run.
 * Labelling runs in ROUNDS of launches, once in 3-D on b and once per slice on the complement of the chosen component,
 * by one routine: every voxel holds a parent index <= its own inside its component; a hook launch lowers the parent of
 * each voxel's root to the smallest root among its neighbours (integer atomic min), a flatten launch replaces every
 * parent by its root (a walk over strictly decreasing indices). Every access to the parent array inside those launches
 * is an agent-scope atomic, and nothing depends on a store of another workgroup of the same launch being seen; a round
 * in which no hook fired ends the phase. Rounds are enqueued eight at a time (rounds after a quiet one return at once)
 * and the host then reads the quiet flag back: gs_body_mask SYNCHRONISES the stream once per eight rounds, a few times
 * per case, and therefore cannot be captured into a graph. The number of rounds grows with the number of merges a
 * component needs, not with the length of a path. Component sizes are integer atomic adds on the roots; the argmax is a
 * two-level reduction over (count, lowest root) in a fixed order.
 * ws: gs_body_mask_ws_bytes(D, H, W) bytes, 8-byte aligned, private to the call; after the call its first two int32 hold
 * the rounds the two phases ran (diagnostic). D * H * W must be below 2^31; that, null pointers, non-positive sizes, the
 * dtype and a NaN threshold are refused before any launch. */
int64_t gs_body_mask_ws_bytes(int32_t D, int32_t H, int32_t W);
int gs_body_mask(const void* vol, int32_t dtype, int32_t D, int32_t H, int32_t W, float threshold, uint8_t* mask_out,
                 int32_t* info, void* ws, void* stream);

/* ---- losses (fp32, on the boundary images / discriminator maps) --------------------------------- */
/* loss[0] = mean((x-target)^2); if grad != NULL: grad = grad_scale * 2*(x-target)/n
 * (nn.MSELoss vs expanded constant, adversarial_loss.py:28-29,60-62) */
int gs_mse_const(const float* x, int64_t n, float target, float* loss, float* grad, const float* grad_scale,
                 void* stream);
/* Every objective of AdversarialLoss.calculate_loss (adversarial_loss.py:52-73) on one discriminator map of n floats.
 * mode GS_ADV_LSGAN      mean((x-label)^2)                                    (= gs_mse_const)
 *      GS_ADV_VANILLA    nn.BCEWithLogitsLoss vs the expanded label            (:31-32,60-62)
 *      GS_ADV_WGANGP     -mean(x) if target_is_real else +mean(x)             (:63-67)
 *      GS_ADV_NONSAT     per-sample mean of softplus(-x) / softplus(x): loss and grad_scale hold `rows` floats, rows = the
 *                        batch (:68-73; the reference's branch dies on an unimported F — this is what it spells out)
 * loss and/or grad (n floats, = grad_scale * d loss / d x) are written; either may be NULL. */
enum { GS_ADV_LSGAN = 0, GS_ADV_VANILLA = 1, GS_ADV_WGANGP = 2, GS_ADV_NONSAT = 3 };
int gs_adv_loss(const float* x, int64_t n, int32_t rows, int32_t mode, int32_t target_is_real, float label,
                float* loss, float* grad, const float* grad_scale, void* stream);
/* loss[0] = mean(|a-b|); if grad_a != NULL: grad_a = grad_scale * sign(a-b)/n
 * (nn.L1Loss, cyclegan_losses.py:64,75,97-101) */
int gs_l1(const float* a, const float* b, int64_t n, float* loss, float* grad_a, const float* grad_scale,
          void* stream);
/* gs_l1 with a channel window as the first operand: sample n of `a` is the `per` contiguous floats at a + n * a_sample_stride,
 * `b` is dense [N][per]. loss[0] = mean(|a-b|) over the N * per elements, summed in gs_l1's order; if grad_b != NULL:
 * grad_b = grad_scale * sign(b-a) / (N * per), dense like b (grad_scale: device scalar, NULL = 1). `a` needs no alignment. */
int gs_l1_window(const float* a, int64_t a_sample_stride, const float* b, int32_t N, int64_t per, float* loss, float* grad_b,
                 const float* grad_scale, void* stream);
/* out[0] = mean(x)  (train_metrics.py:27-33) */
int gs_mean(const float* x, int64_t n, float* out, void* stream);
/* out[r] = c[r] + sum_k m[r*K + k] * x[k][0], r < R <= 8, k < K <= 16: the scalar algebra of a recipe's loss assembly
 * (lambda * (alpha * ssim + beta * l1), loss_real + loss_fake, the sum of the G losses: cyclegan_losses.py:21-32,70-90,
 * cyclegan.py:150,182) as one launch. x = HOST array of K device pointers to fp32 scalars (a null entry counts as 0), m / c =
 * host arrays (c may be null). The backward of a combination is the same call with the transposed matrix over the rows'
 * upstream gradients. */
int gs_scalar_affine(const float* const* x, int32_t K, const float* m, const float* c, int32_t R, float* out, void* stream);
/* out = a + b over n floats (16-byte aligned): the join of the two gradients of a generated image that feeds a
 * discriminator and the other generator (cyclegan.py:131-141) */
int gs_sum2_f32(const float* a, const float* b, float* out, int64_t n, void* stream);
/* SSIM distance of ganslate/nn/losses/utils/ssim.py:65-99 on (x+1)/2,(y+1)/2, window 11, sigma 1.5:
 * out[0] = mean(sqrt(relu(2 - S1 - S2))) over [N*C, H-10, W-10] */
int gs_ssim_distance(const float* x, const float* y, int32_t NC, int32_t H, int32_t W, float* out,
                     float* scratch, void* stream);
int64_t gs_ssim_scratch_floats(int32_t NC, int32_t H, int32_t W);
/* gradient of gs_ssim_distance w.r.t. y (the distance is symmetric: swap x and y for the other one), scaled by the
 * upstream scalar grad_scale[0] (device pointer, NULL = 1): the SSIM-weighted cycle loss, cyclegan_losses.py:78-90 */
int gs_ssim_distance_backward(const float* x, const float* y, int32_t NC, int32_t H, int32_t W,
                              const float* grad_scale, float* grad_y, float* scratch, void* stream);
int64_t gs_ssim_backward_scratch_floats(int32_t NC, int32_t H, int32_t W);
/* The same two with a channel window as the constant image x: plane p (0 <= p < x_planes) of sample n sits at
 * x + n * x_sample_stride + p * H * W; NC = samples * x_planes planes in all, y (and grad_y) dense [NC][H][W]. The gradient
 * is the dense entry point's (same kernels, scratch size, arithmetic and summation order: the dense form is the
 * x_sample_stride = x_planes * H * W case). The forward evaluates the same formula with the same fp32 Gaussian weights in double
 * and rounds the mean once — the windows of this recipe are often single small planes, where a handful of valid pixels does not
 * average the fp32 error of the variance terms out; its scratch is one DOUBLE per tile: 2 * gs_ssim_scratch_floats(NC, H, W)
 * floats, 8-byte aligned. */
int gs_ssim_distance_window(const float* x, int64_t x_sample_stride, int32_t x_planes, const float* y, int32_t NC, int32_t H,
                            int32_t W, float* out, float* scratch, void* stream);
int gs_ssim_distance_window_backward(const float* x, int64_t x_sample_stride, int32_t x_planes, const float* y, int32_t NC,
                                     int32_t H, int32_t W, const float* grad_scale, float* grad_y, float* scratch,
                                     void* stream);

/* ---- MIND structure-consistency loss (mind.hip) ----
 * The reference's MINDDescriptor / StructureLoss of
 * projects/cleargrasp_depth_estimation/modules/old/cyclegan_losses_with_structure.py (Yang et al. 2018). Images are fp32
 * NCHW, contiguous; an image with C > 1 channels is reduced to one plane by the mean over its channels first (:69,:81-82).
 * Only nl_size 9, patch_size 7, neighbor_size 3 (MIND_DESCRIPTOR_CONFIG, :7) are built, anything else is refused; sigma
 * (gaussian_patch_sigma) is free. The patch weights are exp(-|q|_2 / sigma^2) with the Euclidean distance, not its square,
 * not normalised (:126-135). No float atomics: results are bitwise reproducible. All launches go to `stream`. */
/* out = [N, 81, H, W] features, channel i = the shift with row offset i % 9 - 4, column offset i / 9 - 4
 * (MINDDescriptor.forward, :158-182) */
int gs_mind_descriptor(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t nl_size, int32_t patch_size,
                       int32_t neighbor_size, float sigma, float* out, void* stream);
/* out[0] = sum_{n,a,p} |f_a^x - f_a^y| / (H W 81): StructureLoss.__call__ (:72-74,:89-91) without its lambda_structure; a sum
 * over the batch, not a mean. x has Cx channels, y has Cy. No 81-channel map is written to memory. scratch =
 * gs_mind_scratch_bytes(N, H, W, 0) bytes. */
int gs_mind_l1(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t H, int32_t W, int32_t nl_size,
               int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* scratch, void* stream);
/* gradient of gs_mind_l1 w.r.t. y (the loss is symmetric: swap x and y for the other one), [N, Cy, H, W], scaled by the
 * upstream scalar grad_scale[0] (device pointer, NULL = 1): autograd's backward through :72-74,:89-91 and :158-182.
 * scratch = gs_mind_scratch_bytes(N, H, W, 1) bytes. */
int gs_mind_l1_backward(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t H, int32_t W,
                        int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma, const float* grad_scale,
                        float* grad_y, void* scratch, void* stream);
/* bytes of scratch for gs_mind_l1 (backward = 0: one partial per tile) or gs_mind_l1_backward (backward = 1: 171 planes
 * per sample, in place of the tensors autograd keeps for :172-181) */
int64_t gs_mind_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t backward);

/* ---- MIND structure-consistency loss for volumes (mind3d.hip) ----
 * The reference has no volumetric MIND: this is the definition. Volumes are fp32 NCDHW, contiguous; I is the mean over the
 * channels of a sample, zero outside the volume. With the 27 shifts a of the 3x3x3 non-local region, the 5x5x5 patch and the
 * 3x3x3 neighbourhood (the only sizes built: anything else is refused with a message), eps = 1e-8:
 *   d_a(r) = I(r + a) - I(r)                           (r inside; I(r + a) = 0 outside)
 *   D_a(p) = sum_{q in 5^3, p+q inside} g(q) d_a(p+q)^2,  g(q) = exp(-|q|_2 / sigma^2)  (Euclidean distance, not squared;
 *            distance and quotient in fp32, the exponential in double, stored as fp32, as gs_mind_* round theirs)
 *   B_b(p) = sum_{q in 5^3, p+q inside} I(p+q+b) for the 27 shifts b of the neighbourhood;  V = variance of the 27, divisor 26
 *   n_a = exp(-D_a / (V + eps));  f_a = n_a / sum_c n_c
 *   L(X, Y) = sum_{n,a,p} |f_a^X - f_a^Y| / (D H W 27)   (a sum over the batch, not a mean)
 * Channel i of the features has depth offset i % 3 - 1, row offset (i / 3) % 3 - 1 and column offset i / 9 - 1 (the first
 * spatial axis runs fastest, as in gs_mind_descriptor). No float atomics: results are bitwise reproducible. All launches go
 * to `stream`. Refused before any launch: null pointers, non-positive extents, 2^31 or more workgroups (one per 4 x 8 x 8
 * box), a sample of 2^31 or more voxels. */
/* out = [N, 27, D, H, W] features */
int gs_mind3d_descriptor(const float* x, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W, int32_t nl_size,
                         int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* stream);
/* out[0] = L(x, y); x has Cx channels, y has Cy. No 27-channel volume is written to memory. scratch =
 * gs_mind3d_scratch_bytes(N, D, H, W, 0) bytes. */
int gs_mind3d_l1(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t D, int32_t H, int32_t W,
                 int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma, float* out, void* scratch,
                 void* stream);
/* gradient of gs_mind3d_l1 w.r.t. y (the loss is symmetric: swap x and y for the other one), [N, Cy, D, H, W], scaled by
 * the upstream scalar grad_scale[0] (device pointer, NULL = 1). scratch = gs_mind3d_scratch_bytes(N, D, H, W, 1) bytes. */
int gs_mind3d_l1_backward(const float* x, const float* y, int32_t N, int32_t Cx, int32_t Cy, int32_t D, int32_t H, int32_t W,
                          int32_t nl_size, int32_t patch_size, int32_t neighbor_size, float sigma, const float* grad_scale,
                          float* grad_y, void* scratch, void* stream);
/* bytes of scratch for gs_mind3d_l1 (backward = 0: one partial per box) or gs_mind3d_l1_backward (backward = 1: 81 volumes
 * per sample) */
int64_t gs_mind3d_scratch_bytes(int32_t N, int32_t D, int32_t H, int32_t W, int32_t backward);

/* ---- validation / test image metrics (ganslate/utils/metrics/val_test_metrics.py:37-166, valmetrics.hip) ----
 * t (target) and p (prediction): N samples of P planes of H x W fp32, contiguous. table = device [N][7] fp64, one row per
 * sample: mae, mse, nmse (:37-53), psnr = 10 log10(max(t)^2 / mse) (:56-59), ssim = mean over the P planes of skimage
 * structural_similarity with defaults (7x7 uniform window, sample covariance, K1 0.01, K2 0.03, data range max(t) of the
 * sample; :62-87), nmi (:90-107) and histogram_chi2 (:110-131) from 100-bin histograms with numpy's float32 edges.
 * mae..psnr are always computed; GS_VM_SSIM adds ssim (needs H, W >= 7), GS_VM_HIST adds nmi and histogram_chi2 and needs
 * counts = device [N][2*100 + 100*100] uint32 (t bins, p bins, joint [t bin][p bin]), which it leaves holding the raw
 * bin counts. Columns not computed hold NaN. No float atomics: results are bitwise reproducible. At most four launches.
 * Inputs must be finite: where numpy raises ValueError on an inf / NaN histogram range, inf / NaN values are binned here
 * without an error. */
enum { GS_VM_SSIM = 1, GS_VM_HIST = 2 };
int gs_valmetrics(const float* t, const float* p, int32_t N, int32_t P, int32_t H, int32_t W, int32_t flags,
                  double* table, uint32_t* counts, void* scratch, void* stream);
int64_t gs_valmetric_scratch_bytes(int32_t N, int32_t P, int32_t H, int32_t W);

/* ---- the same metrics inside region masks (ganslate/engines/validator_tester.py:78-98,
 *      utils/metrics/val_test_metrics.py:19-29 create_masked_array, :141-149 get_metrics(mask=...)) ----
 * The reference scores np.ma.masked_array(x * m, mask=~m) with m = mask.astype(bool); some of the numpy / scipy /
 * scikit-image calls behind the seven metrics honour the mask and others strip it (np.asarray). Per sample, with m in
 * {0, 1}, n = sum(m), S = P*H*W, tm = t*m, pm = p*m and Rm = the maximum of t over the elements with m != 0 (not max(tm):
 * they differ when every target value inside the mask is negative):
 *   mae  = sum_m |t-p| / n          mse = sum_m (t-p)^2 / n          nmse = sum_m (t-p)^2 / sum_m t^2
 *          (np.mean, np.linalg.norm and .max() run over the unmasked elements; checked against numpy)
 *   psnr = 10 log10(Rm^2 / (sum_m (t-p)^2 / S)): divisor S, not n, because scikit-image converts with np.asarray and
 *          averages over every element
 *   ssim = the plane-wise 7x7 SSIM of gs_valmetrics of tm against pm over all planes, data range Rm
 *          (scipy.ndimage.uniform_filter sees x*m)
 *   nmi, histogram_chi2 = from the 100-bin histograms of tm and pm over all S elements: masked-out elements count as
 *          zeros, so the ranges are those of tm / pm (np.histogram and np.histogramdd see x*m; checked against numpy)
 * The psnr and ssim rows are read from scikit-image's source (_as_floats, mean_squared_error, structural_similarity) and
 * are not pinned against an installed scikit-image, as the unmasked ssim is not.
 * Definitions of this library: n == 0 gives NaN in every column of that row (the reference yields numpy's masked
 * constant); a mask has exactly the shape of the sample batch (the reference raises MaskError otherwise); any non-zero
 * mask byte means "inside".
 * masks = host array of L (1..GS_VM_MAX_LABELS) device pointers, each to N*P*H*W bytes laid out like t. table = device
 * [N][L][7] fp64 in the column order of gs_valmetrics; counts (needed with GS_VM_HIST) = device [N][L][2*100 + 100*100]
 * uint32, left holding the raw bin counts of tm and pm. t*m and p*m are never written to memory: one launch packs the
 * masks into a bit per label and the passes apply them on load. At most five launches whatever L is; t and p are read
 * once for all labels by the moments pass. No float atomics: tables are bitwise reproducible. */
#define GS_VM_MAX_LABELS 8
int gs_valmetrics_masked(const float* t, const float* p, const uint8_t* const* masks, int32_t L, int32_t N, int32_t P,
                         int32_t H, int32_t W, int32_t flags, double* table, uint32_t* counts, void* scratch,
                         void* stream);
int64_t gs_valmetric_masked_scratch_bytes(int32_t N, int32_t L, int32_t P, int32_t H, int32_t W);

/* ---- sliding-window (patch-wise) inference (ganslate/utils/sliding_window_inferer.py:8-52 -> monai/inferers/utils.py
 *      sliding_window_inference; slidewin.hip) ----
 * The stitching around a predictor that sees sw_batch_size windows at a time. Dense fp32 NCDHW tensors; an image is the
 * D == 1 case. roi = host {rd, rh, rw}, every entry >= 1. An input of D x H x W is, in the algorithm, padded symmetrically
 * with cval to the padded size max(size, roi) per axis; pad_before = host {z, y, x}, the part in front (the reference puts
 * (roi - size) / 2, rounded down, there), 0 <= pad_before[k] <= max(size, roi)[k] - size[k]. table = device int32 [n][4],
 * 16-byte aligned, one row (batch item, z, y, x) per window with the starts in padded coordinates; n >= 1. A padded sample
 * (all channels) and a window batch item hold fewer than 2^31 elements. imap = the importance map, device [rd][rh][rw].
 * Whatever the rows hold, no kernel writes outside the tensor it is given.
 *
 * gs_sw_gather: out [n][C][rd][rh][rw] = the windows of rows 0..n-1 cut from the padded input; in = the UNPADDED
 * [B][C][D][H][W], the padded copy is never built: a coordinate in the padding (or a row whose batch item is not in
 * [0, B)) reads cval. Every element of out is written.
 *
 * gs_sw_accumulate: acc[b][c][window of row i] += imap * pred[i][c] for the n rows of one chunk, in increasing i; per
 * element one rounded multiply, then one rounded add (no fma), so acc holds the bits of the sequential host loop
 * `for i: acc[window_i] += imap * pred[i]`. acc = [B][C][Dp][Hp][Wp] at the PADDED size (the caller zeroes it before the
 * first chunk), pred = [n][C][rd][rh][rw]. table_host = the same n rows in host memory: they are checked against the
 * accumulator (error code, nothing launched) and give the largest per-sample bounding box of the chunk's windows, over
 * which the launch runs. One thread owns an accumulator element and walks the rows in order: windows of a chunk may
 * overlap, and no atomics are used. Bitwise reproducible.
 *
 * gs_sw_finalize: result [B][C][D][H][W] (original size) = acc[.., v + pad_before] / count(v + pad_before), correctly
 * rounded division, where count(q) = the sum of imap over ALL n windows of the call that cover q, added in increasing
 * row index from zero — the bits of the host's `count[window_i] += imap`; no count buffer exists. A voxel no window covers
 * gives 0 / 0 = NaN, as on the host. */
int gs_sw_gather(const float* in, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, const int32_t* table, int32_t n,
                 const int32_t* roi, const int32_t* pad_before, float cval, float* out, void* stream);
int gs_sw_accumulate(float* acc, int32_t B, int32_t C, int32_t Dp, int32_t Hp, int32_t Wp, const int32_t* table,
                     const int32_t* table_host, int32_t n, const int32_t* roi, const float* imap, const float* pred,
                     void* stream);
int gs_sw_finalize(const float* acc, int32_t B, int32_t C, int32_t D, int32_t H, int32_t W, const int32_t* table,
                   int32_t n, const int32_t* roi, const int32_t* pad_before, const float* imap, float* result,
                   void* stream);

/* ---- the logged image grid (ganslate/utils/trackers/utils.py process_visuals_for_logging followed by
 *      torchvision.utils.save_image; visgrid.hip) ----
 * One kernel, one launch: K visuals side by side along the width, HWC bytes ready for a PNG encoder.
 * src = host array of K (1..GS_VIS_MAX_SRCS) device pointers to dense fp32 [N][ctot[k]][D][H][W] tensors (an image is the
 * D == 1 case); visual k shows the c[k] (1 or 3) channels from c0[k] on of its tensor, so a channel-wise modality split is
 * two entries with the same pointer and no copy. ctot, c0, c = host arrays of K; all four arrays reach the kernel by value
 * in its argument struct: the call allocates nothing on the device and uploads no table. The first n (1..N) samples are
 * written. slice == -1 stacks all D slices along the height, slice 0 on top; slice in [0, D) shows that slice only.
 * out = device [n][Hout][K * W][3] bytes, Hout = (slice < 0 ? D : 1) * H:
 *   out[s][row][k * W + x][ch] = byte(src[k][s][c0[k] + (c[k] == 3 ? ch : 0)][z][y][x]), row = z * H + y or y
 *   byte(v) = (uint8) clamp(((v + 1) / 2) * 255 + 0.5, 0, 255), every operation rounded to fp32 on its own (no fma, not
 *   re-associated), then truncated: the bits of the separate torch ops. NaN gives 0, +inf 255, -inf 0.
 * Every source element that appears in the image is read once (float4 where W % 4 == 0 and the line is 16-byte aligned),
 * every output byte is written once, there is no scratch buffer; out needs no alignment. H * W, D * H and K * W must be
 * < 2^31, D and n * K <= 65535; offsets into the tensors are 64-bit. What does not fit is rejected with a non-zero
 * return and nothing is launched. No thread writes outside out. */
#define GS_VIS_MAX_SRCS 16
int gs_visuals_grid_u8(const float* const* src, const int32_t* ctot, const int32_t* c0, const int32_t* c, int32_t K,
                       int32_t n, int32_t N, int32_t D, int32_t H, int32_t W, int32_t slice, uint8_t* out, void* stream);

/* ---- PatchNCE + patch MLP of CUT (ganslate/nn/gans/unpaired/cut.py:229-294, ganslate/nn/losses/cut_losses.py:14-43) ----
 * For every feature level l: sampled patches xq[l], xk[l] are [batch*patches][channels[l]] fp32 (target = query, source =
 * key, row = image * patches + patch); FeaturePatchMLP level l = Linear(C_l, nc) - ReLU - Linear(nc, nc) - x/(||x||+1e-7);
 * PatchNCE: logits [q.k+ , q.k_j over the other patches of the same image, diagonal -> -10] / nce_T, cross-entropy vs 0,
 * keys detached. params / grads: one flat fp32 buffer, per level W1 [nc][C_l], b1 [nc], W2 [nc][nc], b2 [nc]
 * (gs_patchnce_param_floats). loss[l] = lambda_nce / (levels * batch * patches) * sum over rows of the row loss, so that
 * sum_l loss[l] is what CUT._calculate_nce_loss returns (cut.py:218-226).
 * forward leaves what backward needs in `work` (gs_patchnce_work_bytes, caller-owned, same buffer for both calls);
 * backward: dxq[l] = d(sum_l loss[l]) / d xq[l] * grad_scale[0], grads += parameter gradients * grad_scale[0]
 * (grad_scale: device scalar, NULL = 1). nc must be 256 and patches <= 256 (the reference's defaults, cut.py:16-20). */
#define GS_PATCHNCE_MAX_LEVELS 8
typedef struct gs_patchnce_desc {
  int32_t levels, batch, patches, nc;
  int32_t channels[GS_PATCHNCE_MAX_LEVELS];
  float nce_T, lambda_nce;
} gs_patchnce_desc;
int64_t gs_patchnce_param_floats(const gs_patchnce_desc* d);
int64_t gs_patchnce_work_bytes(const gs_patchnce_desc* d);
int gs_patchnce_forward(const gs_patchnce_desc* d, const float* const* xq, const float* const* xk, const float* params,
                        void* work, float* loss, void* stream);
int gs_patchnce_backward(const gs_patchnce_desc* d, const float* const* xq, float* const* dxq, const float* params,
                         float* grads, void* work, const float* grad_scale, void* stream);

/* ---- SelfAttentionBlock (ganslate/nn/attention.py:12-47; selfattention_patchgan3d.py:58,73, selfattention_vnet3d.py:97-104) ----
 * x, out, dout, dx: NDHWC bf16 [B][N][C] (N = D*H*W voxels of the map, C a multiple of 8). q / k = 1x1x1 convs to C/8 channels,
 * v to C channels; A = softmax over keys of q_i . k_j; out = gamma * (A v) + x. Parameters in torch layout, fp32:
 * wq, wk [C/8][C], bq, bk [C/8], wv [C][C], bv [C], gamma [1] (device pointers). forward leaves q / k / v, the bf16 attention
 * matrix [B][N][N] and A v in `work` (gs_attn_work_bytes, caller-owned, the same buffer for both calls); backward writes
 * dx = d loss / d x and ADDS the parameter gradients into the tensors of `grads` (NULL members / NULL grads: skipped). */
typedef struct gs_attn_desc { int32_t B, N, C; } gs_attn_desc;
typedef struct gs_attn_params { float *gamma, *wq, *bq, *wk, *bk, *wv, *bv; } gs_attn_params;
int64_t gs_attn_work_bytes(const gs_attn_desc* d);
/* ... and for a forward pass whose state is never handed to gs_attn_backward (inference, attention.py:26-47 under no_grad):
 * without the backward's buffers */
int64_t gs_attn_forward_work_bytes(const gs_attn_desc* d);
int gs_attn_forward(const gs_attn_desc* d, const void* x, const gs_attn_params* params, void* out, void* work, void* stream);
int gs_attn_backward(const gs_attn_desc* d, const void* x, const void* dout, const gs_attn_params* params,
                     const gs_attn_params* grads, void* work, void* dx, void* stream);

/* ---- optimiser (torch.optim.Adam betas=(0.5,0.999) eps=1e-8, cyclegan.py:81-82) ------------------ */
/* hyper (host pointer to 6 floats): lr, beta1, beta2, eps, bias_correction1, sqrt(bias_correction2).
 * grad_scale multiplies the gradient (1/world_size after an all-reduce SUM). zero_grad != 0 clears g. */
int gs_adam_step(float* p, float* g, float* m, float* v, int64_t n, const float* hyper_host,
                 float grad_scale, int32_t zero_grad, void* stream);
/* Same update with `hyper` (same 6 floats) in DEVICE memory, so a captured hipGraph of the step can be replayed while
 * the host refreshes the learning rate and bias corrections between replays. */
int gs_adam_step_dev(float* p, float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                     float grad_scale, int32_t zero_grad, void* stream);
/* gs_adam_step_dev that also refreshes the bf16 weight packs where 8 consecutive pack elements are 8 consecutive, 8-aligned
 * master elements (row-major packs: a conv's forward pack, a transposed conv's data-gradient pack; nn/native/net.py builds
 * the tables): inv_x[i] = pack group (of 8 elements) holding master elements 8 i .. 8 i + 7, or -1; tables of ceil(n / 8)
 * int32. Either table / pack pair may be NULL. The transposed packs keep gs_repack_bf16_tiled_groups. Buffers 16-byte
 * aligned. (torch.optim.Adam.step + the weight cast a bf16 autocast run would do per use, pix2pix.py:61-66) */
int gs_adam_step_dev_packs(float* p, float* g, float* m, float* v, int64_t n, const float* hyper_dev, float grad_scale,
                           int32_t zero_grad, const int32_t* inv_f, void* fpack, const int32_t* inv_d, void* dpack,
                           void* stream);
/* gs_adam_step_dev_packs over several ranges [start, end) of the flat buffers in ONE launch (ranges_dev: device int64 [n_ranges][2],
 * elements, starts multiples of 8; max_len = the longest range; inv_f / inv_d index the WHOLE buffers): what gs_wgrad_adam leaves of
 * a network — biases and small layers between the layers it updated itself */
int gs_adam_step_dev_packs_ranges(float* p, float* g, float* m, float* v, const int64_t* ranges_dev, int32_t n_ranges,
                                  int64_t max_len, const float* hyper_dev, float grad_scale, int32_t zero_grad,
                                  const int32_t* inv_f, void* fpack, const int32_t* inv_d, void* dpack, void* stream);
/* ---- the PatchGAN's last layer: Conv2d(8 ndf, 1, k4, s1, p1) (patchgan2d.py:62) — one output channel -------------------------
 * A dot product per pixel: on the vector ALUs (v_dot2c_f32_bf16) with the filter in registers and a sliding 4 x 4 window of
 * input pixels, instead of an eighth of an MFMA tile behind a 16-fold im2col gather (csrc/cout1.hip). Same descriptors,
 * packs (row 0 is the filter; the other rows of the 8-row pack are zero) and results as gs_gconv_forward / gs_wgrad_ws for
 * this layer: out channel 0 = conv + bias, channels 1..7 = 0; dw row 0 += the gradient (rows 1..7 belong to channels whose
 * output gradient is zero). _eligible: 2-D, 16 taps forming a 4 x 4 grid, stride 1, zero border, Co = 8, Ci <= 512, no
 * statistics / accumulate. tw may be NULL. Workspace of the weight gradient: gs_wgrad_cout1_ws_floats (-1: not eligible);
 * partial sums per workgroup are added in a fixed order. */
int gs_conv_cout1_eligible(const gs_gconv_desc* d);
int gs_conv_cout1_forward(const gs_gconv_desc* d, const void* in, const void* w_pack, const float* bias, void* out,
                          const gs_twin* tw, void* stream);
int gs_wgrad_cout1_eligible(const gs_wgrad_desc* d);
int64_t gs_wgrad_cout1_ws_floats(const gs_wgrad_desc* d);
int gs_wgrad_cout1_ws(const gs_wgrad_desc* d, const void* a, const void* g, float* dw, float* ws, int64_t ws_floats,
                      const gs_twin* tw, void* stream);

/* ---- feature taps of CUT's PatchNCE loss (ganslate/nn/gans/unpaired/cut.py:229-312; FeaturePatchMLP.forward :262-277 reads
 * `feat.permute(0, 2, 3, 1).flatten(1, 2)[:, patch_id, :]` per level) ------------------------------------------------------------
 * ids_dev: int64 device array of P DISTINCT flat pixel indices (the head of a torch.randperm), shared by the n images.
 * gs_tap_gather: out[n][p][ch] = src[n][ids[p]][ch] as fp32, ch < c; src = n images of `pixels` NHWC bf16 pixels, cs channels.
 * gs_tap_scatter_add: the backward of it into a gradient buffer on a domain padded by f0: with (y, x) = divmod(ids[p], W),
 *   dst[n][(y + f0) * Wp + x + f0][ch] += g[n][p][ch] (bf16 storage, fp32 add); `pixels` = pixels per image of dst.
 * gs_tap_rows_sum: db[ch] += sum over rows of g[rows][c] in a fixed order (bias gradient seen by a tap of a raw conv output).
 * gs_zero_bytes: zero a 16-byte aligned buffer (the start of a gradient that only taps feed).
 * gs_image_tap_gather / _scatter: nce layer 0 is the ReflectionPad2d(pad) output of the fp32 NCHW image (resnet2d.py:24):
 *   out[n][p][ch] = x[n][ch][r(yp - pad)][r(xp - pad)], (yp, xp) = divmod(ids[p], W + 2 pad), r = reflection; the scatter
 *   zeroes gx [N][C][H][W] and adds g through the same map, colliding samples (reflected onto one pixel) in sample order:
 *   deterministic, at the price of an O(P^2) scan of the ids in LDS — P <= 16384 samples per image (the reference draws
 *   256, cut.py:46), larger P is refused with an error. */
int gs_tap_gather(const void* src, int32_t n, int64_t pixels, int32_t cs, const int64_t* ids_dev, int32_t P, int32_t c, float* out,
                  void* stream);
int gs_tap_scatter_add(void* dst, int32_t n, int64_t pixels, int32_t cs, const int64_t* ids_dev, int32_t P, int32_t c, int32_t W,
                       int32_t Wp, int32_t f0, const float* g, void* stream);
int gs_tap_rows_sum(const float* g, int64_t rows, int32_t c, float* db, void* stream);
int gs_zero_bytes(void* p, int64_t bytes, void* stream);
int gs_image_tap_gather(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t pad, const int64_t* ids_dev, int32_t P,
                        float* out, void* stream);
int gs_image_tap_scatter(const float* g, int32_t N, int32_t C, int32_t H, int32_t W, int32_t pad, const int64_t* ids_dev,
                         int32_t P, float* gx, void* stream);
/* FastCUT's flip-equivariance coin (cut.py:146-152: `real_A.flip(-1)` on a host coin): out = flag_dev[0] ? x.flip(-1) : x over
 * [rows][W] fp32, the flag in device memory so that a captured step replays either way. Not in place. */
int gs_flip_w_if(const float* x, float* out, int64_t rows, int32_t W, const int32_t* flag_dev, void* stream);

/* ImagePool.query (ganslate/data/utils/image_pool.py:31-60) with the host's coin flips uploaded as code_dev[B]:
 * < 0 pass image b through; slot: store image b in `slot`, return it (pool filling); slot | 0x40000000: return the
 * image stored in `slot`, store image b there. Images of a batch are handled in order (same-slot draws chain like the
 * reference's loop). pool = [slots][image_bytes], images/out = [B][image_bytes], image_bytes % 16 == 0. */
int gs_pool_query(void* pool, const void* images, void* out, const int32_t* code_dev, int32_t B,
                  int64_t image_bytes, void* stream);
/* pack[e] = bf16(master[index[e]]) (index < 0 -> 0): refresh the bf16 forward/dgrad weight packs */
int gs_repack_bf16(const float* master, const int32_t* index, void* pack, int64_t n, void* stream);

/* Same refresh for one [rows][kp] pack segment whose master indices run along the rows (transposed packs): 64 x 64
 * tiles through LDS so that both the master reads and the pack writes are contiguous. Results are identical. */
int gs_repack_bf16_tiled(const float* master, const int32_t* index, void* pack, int32_t rows, int32_t kp, void* stream);
/* Group-indexed forms of the two refreshes (round 3): one base index per 8 pack elements whose sources are 8 consecutive
 * master elements. Same call sites as gs_repack_bf16 (optimizer.step() -> weights the next forward reads,
 * cyclegan.py:107,123); an eighth of the index traffic; two launches per pack of a network.
 * gs_repack_bf16_groups, along k over the WHOLE pack: pack[8 g + j] = master[gindex[g] + j]; gindex[g] = -1 -> zeros,
 *   -2 -> the group's eight own entries of the element-wise table `index` (null if no group is marked), -3 -> not written
 *   (the group belongs to a transposed segment); n8 groups.
 * gs_repack_bf16_tiled_groups, along the rows of ALL transposed segments of the pack: seg_dev[5 i ..] = {pack offset in
 *   elements, gindex offset, rows (multiple of 8), kp (multiple of 64), first tile}, tiles = sum of ceil(rows / 64) * kp / 64;
 *   pack[off + (8 G + j) * kp + k] = master[gindex[goff + G * kp + k] + j], negative -> zeros.
 * master 16-byte aligned, pack 16-byte (8-byte for the segments) aligned. */
int gs_repack_bf16_groups(const float* master, const int32_t* gindex, const int32_t* index, void* pack, int64_t n8,
                          void* stream);
int gs_repack_bf16_tiled_groups(const float* master, const int32_t* gindex, void* pack, const int64_t* seg_dev,
                                int32_t nseg, int64_t tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANSLATE_HIP_H */
