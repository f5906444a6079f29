/*
 * dvs_train.h — C-ABI of the two streaming ops that sit immediately before / after the rasterizer in
 * train_step(): image loss + its gradient, and the fused Adam update of
 * the 59-float splat rows. They exist so that libgstrain's train_step() is a real training iteration;
 * the reference's own implementations live in the closed `gstrain` plugin (README.md:46). Flags that
 * select them in the reference: --ssim (application/diverseshot-cli/source/main.cpp:24-25), learning
 * rates (main.cpp:31, gs_train.cpp:52-57).
 */
#ifndef DVS_TRAIN_H
#define DVS_TRAIN_H
#include <stddef.h>
#include <stdint.h>
#include "dvs_raster.h"   /* dvs_camera (the 3D smoothing filter's camera rows) */
#ifdef __cplusplus
extern "C" {
#endif

/* Mean-L1 image loss over count floats: dL[i] = sign(rgb[i]-target[i]) / count; *loss_accum += sum|rgb-target| / count.
 * rgb, target, dL, loss_accum are DEVICE pointers; loss_accum (1 float) must be zeroed by the caller. Asynchronous. */
int dvs_l1_loss_grad(void* stream, const float* rgb, const float* target, size_t count, float* dL, float* loss_accum);
/* Weighted form for the mixed loss (1-w) L1 + w (1-SSIM): dL[i] = weight * sign(..)/count; *loss_accum += weight * mean|..|. */
int dvs_l1_loss_grad_w(void* stream, const float* rgb, const float* target, size_t count, float weight, float* dL, float* loss_accum);
/* Mean-squared-error variant (the upstream gradient bench.py uses): dL = (rgb-target) * (2/count)... scaled by `scale`. */
int dvs_l2_loss_grad(void* stream, const float* rgb, const float* target, size_t count, float scale, float* dL, float* loss_accum);

/* D-SSIM term of the photometric loss (reference flag --ssim, default weight 0.2: main.cpp:24-25; loss = (1-w) L1 + w (1 - SSIM)).
 * SSIM with the standard 11x11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2, per channel, mean over
 * all 3*H*W values. Two fused passes over LDS-staged 16x16 tiles with a 5-pixel halo:
 *   dvs_ssim_forward : img, target [3,H,W] -> per-pixel partial derivative maps (3 x [3,H,W], caller-provided scratch) and
 *                      ssim_sum[0..DVS_SSIM_SLOTS) += partial sums of the SSIM map (add the slots, divide by 3*H*W for the mean;
 *                      several slots because tens of thousands of same-address atomics would serialise);
 *   dvs_ssim_backward: dL_dimg[3,H,W] (+)= scale * d(mean SSIM)/d(img)   (scale = -w to minimise 1 - SSIM; accumulate = add).
 * All pointers DEVICE; asynchronous on `stream`. */
#define DVS_SSIM_SLOTS 4096          /* (64 slots made the 24 k per-workgroup atomics of a 1080p image the bottleneck of both loss kernels: 0.17 vs 0.06 ms) */
int dvs_ssim_forward(void* stream, const float* img, const float* target, int width, int height, float* dm_dmu1,
                     float* dm_dsigma1_sq, float* dm_dsigma12, float* ssim_sum);
int dvs_ssim_backward(void* stream, const float* img, const float* target, int width, int height, const float* dm_dmu1,
                      const float* dm_dsigma1_sq, const float* dm_dsigma12, float scale, float* dL_dimg, int accumulate);
/* The whole photometric gradient of L = (1-w) mean|x-y| + w (1 - mean SSIM) in one pass after dvs_ssim_forward:
 *   dL_dimg = (1-w)/(3HW) sign(x-y) - w/(3HW) dSSIM/dx   (overwritten),   l1_sum[0..DVS_SSIM_SLOTS) += (1-w)/(3HW) sum|x-y| (nullable).
 * Equivalent to dvs_l1_loss_grad_w(weight 1-w) followed by dvs_ssim_backward(scale -w, accumulate). */
int dvs_loss_l1_ssim_backward(void* stream, const float* img, const float* target, int width, int height, const float* dm_dmu1,
                              const float* dm_dsigma1_sq, const float* dm_dsigma12, float ssim_weight, float* dL_dimg, float* l1_sum);

/* ---- image metrics of a batch of views (held-out evaluation) ---------------------------------------------------------------------
 * out[v] = {mse, l1, ssim, psnr} of view v, with m = the pixel's mask value (1 when mask is NULL),
 *   x = min(1, max(0, img)) * m,   y = target * m   (an 8-bit target is expanded as (float)u * (1.0f/255.0f), the operation of the
 *   trainer's packLevel PackF32ToU8 views),
 *   mse = sum (x-y)^2 / (3HW),   l1 = sum |x-y| / (3HW),   ssim = the mean SSIM of x and y exactly as the loss kernels above define it,
 *   psnr = -10 log10(max(mse, 1e-10)) in fp64 (100 dB for identical images).
 * ONE launch over the tiles of all views plus a small finalising launch; no per-pixel output, 8-bit targets are read as bytes. Every
 * workgroup writes its fp32 partial sums to its own slot of `scratch` and the finalising kernel adds a view's slots in a fixed order
 * in fp64: no atomics, so two calls on the same inputs return bit-identical rows and a view's row does not depend on which other views
 * share the call.
 *   views     HOST array [n_views] (1..DVS_METRICS_MAX_VIEWS) of DEVICE pointers, all views width x height; copied before the call returns
 *   alignment img / target / mask need only the natural alignment of their element (4 bytes for fp32, 1 for uint8) — NOT the 16 bytes
 *             of the rasterizer's interface: the kernel reads scalars (rows of an odd width cannot be 16-byte aligned anyway)
 *   scratch   DEVICE, dvs_image_metrics_scratch_bytes(width, height, n_views) bytes, 4-byte aligned, no initialisation needed
 *   out       DEVICE double [n_views][4]
 * DVS_ERR_INVALID for n_views outside 1..16, a NULL img / target / scratch / out, non-positive sizes. Asynchronous on `stream`. */
#define DVS_METRICS_MAX_VIEWS 16
typedef struct dvs_metrics_view {   /* DEVICE pointers */
    const float* img;      /* [3,H,W] planar fp32, the rendered view */
    const void*  target;   /* [3,H,W] planar: fp32, or uint8 when target_u8 */
    const float* mask;     /* [H,W] or NULL */
} dvs_metrics_view;
size_t dvs_image_metrics_scratch_bytes(int width, int height, int n_views);
int dvs_image_metrics_views(void* stream, const dvs_metrics_view* views /* HOST [n_views] */, int n_views,
                            int width, int height, int target_u8, void* scratch, double* out /* DEVICE [n_views][4] */);

/* ---- box downsample of a batch of views (coarse-to-fine training: the level targets and masks of resolutionSchedule) -----------------
 * dst(x, y) = mean of the source block [x f, x f + f) x [y f, y f + f), per plane; dst is [planes, height/f, width/f] (floor): the
 * width - (width/f) f rightmost columns and the matching bottom rows of the source are not used. ALL views in ONE launch; no atomics,
 * no scratch. The result is defined bit for bit, whatever path the kernel takes for a view:
 *   uint8 source   ((float)S * (1.0f/255.0f)) * (1.0f/(f*f)), S the exact integer sum of the block (f = 1: the trainer's 8-bit expansion)
 *   fp32 source    the block's values added in fp32 in row-major order, starting from the first one, then * (1.0f/(f*f))
 *   views     HOST array [n_views] (1..DVS_DOWNSAMPLE_MAX_VIEWS) of DEVICE pointers, all views the same size; copied before the call returns
 *   planes    3 for images, 1 for masks;  factor 1, 2, 4 or 8;  src_u8: the sources are uint8, not fp32
 *   alignment only the natural alignment of the element (4 bytes for fp32, 1 for uint8). A view whose src and dst are 16-byte aligned
 *             and whose widths allow it (width % 16 == 0 for uint8, % 4 for fp32; (width/f) % 4 == 0) is moved as 16-byte words.
 * DVS_ERR_INVALID for NULL views / src / dst, n_views outside 1..16, planes < 1, another factor, width/f == 0 or height/f == 0.
 * Asynchronous on `stream`. */
#define DVS_DOWNSAMPLE_MAX_VIEWS 16
typedef struct dvs_downsample_view { const void* src; float* dst; } dvs_downsample_view;   /* DEVICE pointers */
int dvs_downsample_views(void* stream, const dvs_downsample_view* views /* HOST [n_views] */, int n_views,
                         int planes, int width, int height, int factor, int src_u8);

/* Fused Adam over one parameter array (count floats): m, v are the moment arrays (same size, DEVICE).
 * step is 1-based. Asynchronous. */
int dvs_adam_step(void* stream, float* param, const float* grad, float* m, float* v, size_t count, float lr, float beta1,
                  float beta2, float eps, int step);

/* All parameter groups of one optimizer step in ONE launch (the trainer has six: pos, sh0, shN, opacity, scale, rot).
 *   width        floats per splat of the group (3, 45, 1, 4 ...); only used to find the splat of an element when `visible` is given.
 *   layout       DVS_SHN_ROWS: element e belongs to splat e / width.  DVS_SHN_TILED (width 45 only): the [ceil(n/64)][12][64][4] layout.
 *   active_chunks  DVS_SHN_TILED only: update just the first active_chunks (1..12) float4 chunks of every splat, 0 = all. While the
 *                progressive SH degree is below 3 the higher coefficients have g = m = v = 0 and Adam is the identity on them, so
 *                skipping them is exact (chunks needed for degree d: ceil(3*((d+1)^2-1)/4)).
 *   visible      nullable int32[n_splats] (dvs_fwd_state.radii of this view): when given, only splats with visible[i] > 0 are updated and
 *                the moments of the others do not decay — the reference's `visibleAdam` option (gs_train.cpp:87; the "sparse Adam"
 *                of Taming-3DGS). NULL = dense Adam, identical to dvs_adam_step per group.
 *   alignment    param / grad / m / v of every group must be 16-byte aligned (moved as float4); DVS_ERR_INVALID otherwise. */
typedef struct dvs_adam_group {
    float* param;
    const float* grad;
    float* m;
    float* v;
    uint64_t count;       /* floats in the arrays (tiled: padded to whole 64-splat tiles) */
    float lr;
    int32_t width;
    int32_t layout;
    int32_t active_chunks;
} dvs_adam_group;
#define DVS_ADAM_MAX_GROUPS 8
int dvs_adam_step_groups(void* stream, const dvs_adam_group* groups, int n_groups, float beta1, float beta2, float eps, int step,
                         const int32_t* visible, int32_t n_splats);

/* ---- adaptive density control: clone / split / prune, the "ADC" strategy of --densifyStrategy -------------
 * (flags application/diverseshot-cli/source/main.cpp:20,29,46-65: growGrad2d 2e-4, warmupLength 500, refineEvery 100, resetAlphaEvery
 * 3000, refineStopIter 15000, minOpacity 0.005, capMax gs_train.cpp:89). The reference's own densifier is in the closed plugin; this
 * is the public ADC rule it names, operating in place on HBM-resident arrays with no host round trip except the new count.
 *
 * Per refinement interval:
 *   dvs_densify_accumulate after every backward: for visible splats  grad_accum += |g| (g = abs-grad of the 2D mean in NDC units:
 *                          pixel-unit gradient x 0.5*(W,H)),  denom += 1,  max_radii = max(max_radii, radius).
 *   dvs_densify_plan       action per splat from avg = grad_accum/denom:   PRUNE  sigmoid(opacity) < min_opacity, or world/screen size
 *                          above the limits (max exp(scale) > max_world_scale, max_radii > max_screen_radius, both strict; a splat that
 *                          was never visible has max_radii 0 and stays), or an opacity or scale that is NaN or +-inf (no forward
 *                          renders such a splat, so nothing else would ever remove it) — every prune rule is decided before any
 *                          growth, whatever avg;  SPLIT  avg >= grad_threshold and max exp(scale) > scale_threshold (replaced by 2
 *                          samples, scale / 1.6);  CLONE  avg >= grad_threshold otherwise (kept + 1 copy);  KEEP.
 *                          Writes action[n], the exclusive scan of the output counts offsets[n] and the new count (device + pinned host
 *                          copy is the caller's business). Growth is cut off deterministically (by splat index) at cap_max:
 *                          with S surviving (non-PRUNE) splats, only the first max(0, cap_max - S) CLONE / SPLIT candidates in
 *                          splat order keep their action, the others are demoted to KEEP in action[], and
 *                          new_count = min(uncapped count, max(cap_max, S)). PRUNE is never changed by the cap. When S alone exceeds
 *                          cap_max, new_count = S (> cap_max): what to do then (prune harder, or grow the arrays) is the caller's
 *                          decision. cap_max <= 0 = no cap.
 *   dvs_densify_apply      scatters ONE attribute set old -> new at the planned offsets. mode 0 = parameters (split samples drawn
 *                          from the splat's own Gaussian with a counter-based hash RNG), mode 1 = optimizer moments (kept rows copied,
 *                          rows of new splats zero). shN arrays may be in either layout (shn_layout).
 */
enum { DVS_DENSIFY_KEEP = 0, DVS_DENSIFY_CLONE = 1, DVS_DENSIFY_SPLIT = 2, DVS_DENSIFY_PRUNE = 3 };
typedef struct dvs_densify_params {
    float grad_threshold;      /* growGrad2d */
    float scale_threshold;     /* world units: percent_dense * scene extent */
    float min_opacity;         /* prune below (activated opacity) */
    float max_world_scale;     /* prune if max exp(scale) exceeds it; 0 = off */
    int32_t max_screen_radius; /* prune if max_radii exceeds it; 0 = off */
    int32_t cap_max;           /* cap on the new count (growth only, see dvs_densify_plan); <= 0 = no cap */
    uint32_t seed;             /* RNG stream for split samples (use the step number) */
    int32_t shn_layout;        /* DVS_SHN_ROWS / DVS_SHN_TILED for the shN arrays passed to dvs_densify_apply */
    int32_t revised_opacity;   /* config `revisedOpacity`: both results of a clone / split take opacity 1 - sqrt(1 - o), so that
                                  the pair composites to the opacity of the splat it replaces ("Revising Densification in GS") */
} dvs_densify_params;

int dvs_densify_accumulate(void* stream, int n, const int32_t* radii, const float* absgrad2d, int width, int height,
                           float* grad_accum, float* denom, int32_t* max_radii);
/* The same rule for every view of a multi-view pass (dvs_raster_forward_views), exactly as if the views had been accumulated one by
 * one: radii [n_views][n] (dvs_fwd_state.radii of the batch), rows = the composite backward's intermediate rows [n_views][n][12]
 * (dvs_get_bwd_intermediates) — call it between dvs_raster_backward_composite and dvs_raster_backward_project (which consumes them). */
int dvs_densify_accumulate_rows(void* stream, int n, int n_views, const int32_t* radii, const float* rows, int width, int height,
                                float* grad_accum, float* denom, int32_t* max_radii);
/* out[i] = max over the views of radii[v][i] (> 0: visible in at least one view of the pass; the visible-only Adam step's gate) */
int dvs_any_view_radius(void* stream, int n, int n_views, const int32_t* radii, int32_t* out);
/* scratch: at least (n/256 + 2) uint32; new_count: DEVICE uint64. */
int dvs_densify_plan(void* stream, int n, const float* opacity, const float* scale, const float* grad_accum, const float* denom,
                     const int32_t* max_radii, const dvs_densify_params* prm, uint8_t* action, uint32_t* offsets, uint32_t* scratch,
                     uint64_t* new_count);
/* src/dst: six DEVICE arrays in A0 order (pos, sh0, shN, opacity, scale, rot); dst sized for the new count. */
int dvs_densify_apply(void* stream, int n, const uint8_t* action, const uint32_t* offsets, const dvs_densify_params* prm, int mode,
                      const float* const src[6], float* const dst[6], int new_n);
/* Importance prune: keeps the `keep` splats with the largest score (dvs_raster_importance_views' score_sum summed over the training views,
 * dvs_raster.h) and leaves the plan in the form dvs_densify_plan does, so that dvs_densify_apply (modes 0 and 1) compacts from it.
 * Exactly n - min(keep, n) splats are marked DVS_DENSIFY_PRUNE, the rest DVS_DENSIFY_KEEP: the pruned ones are the smallest in the total
 * order (score, then larger index first) — the result is unique, ties included. offsets[n] = the exclusive scan of the kept splats,
 * *new_count (DEVICE uint64) = min(keep, n). Exact and on the device: a most-significant-byte-first radix select over the 64-bit score
 * (eight histogram + pick rounds), then one marking pass that resolves the ties by index; no host round trip. Asynchronous on `stream`.
 * scratch: dvs_importance_scratch_bytes(n) bytes, 16-byte aligned, contents irrelevant. DVS_ERR_INVALID for n <= 0, keep == 0, NULL or
 * misaligned pointers. */
size_t dvs_importance_scratch_bytes(int n);
int dvs_importance_plan(void* stream, int n, const uint64_t* score, uint32_t keep, uint8_t* action, uint32_t* offsets, void* scratch,
                        uint64_t* new_count);
/* Mask carve: which splats the foreground voted for, from the two sums of dvs_raster_foreground_views (dvs_raster.h) accumulated over the
 * training views, in the form dvs_region_plan leaves, so that dvs_densify_apply (modes 0 and 1) compacts from it:
 *   action[i]   DVS_DENSIFY_KEEP iff fg[i] > 0 and fg[i] * (100 - percent) >= bg[i] * percent, else DVS_DENSIFY_PRUNE. The products are
 *               formed in 128 bits: the rule holds for every 64-bit input. A splat that no valid pixel of any view took (fg = bg = 0)
 *               goes: it is in no training view. percent = 100 keeps only the splats that never landed on a background pixel.
 *   offsets[i]  the exclusive scan of the kept splats;  *new_count (DEVICE uint64) = their number (0 when none stays)
 * Three launches (flags + block sums | one workgroup scans the block sums, with a running carry | offsets); no host round trip.
 * Integers only, no atomics: two calls on the same inputs return identical bytes. Asynchronous on `stream`.
 *   scratch  at least (n / 256 + 2) uint32, contents irrelevant (as dvs_densify_plan's)
 * DVS_ERR_INVALID, before anything touches the device, for n <= 0, a percent outside 1..100, a NULL pointer, or a new_count that is
 * not 8-byte aligned; dvs_last_error() names the call. */
int dvs_foreground_plan(void* stream, int n, const uint64_t* fg, const uint64_t* bg, int percent /*1..100*/, uint8_t* action,
                        uint32_t* offsets, uint32_t* scratch, uint64_t* new_count);
/* opacity reset (--resetAlphaEvery): opacity = min(opacity, logit(max_opacity)); zeroes the matching Adam moments if given. */
int dvs_reset_opacity(void* stream, int n, float* opacity, float max_opacity, float* adam_m, float* adam_v);

/* ---- MCMC densification strategy (--densifyStrategy 1, main.cpp:20,29; `noiselr` gs_train.cpp:97) ---------------------------------------
 * The published rule the reference names ("3D Gaussian Splatting as Markov Chain Monte Carlo"); its own code is in the closed plugin.
 * All arrays DEVICE, in A0 order (pos, sh0, shN, opacity, scale, rot), sized for `capacity` splats; m / v = Adam moments (entries may
 * be NULL). Asynchronous on `stream`, no host round trip (the dead count is optional, read back asynchronously).
 *   dvs_mcmc_relocate : every dead splat (sigmoid(opacity) <= min_opacity) becomes a copy of a live splat drawn with probability
 *                       ~ opacity; a splat drawn c times and its c copies take opacity 1-(1-o)^(1/(c+1)) and the scale factor that
 *                       preserves the rendered contribution; moments of everything touched are zeroed.
 *   dvs_mcmc_grow     : n_new more copies drawn the same way are appended at [n, n+n_new) (caller: 5 % growth up to capMax).
 *   dvs_mcmc_add_noise: after each optimizer step  pos += Sigma z gate(o) lr,  z ~ N(0,I), gate = sigmoid(-100 (o - 0.005));
 *                       lr = noiselr * position learning rate.
 *   dvs_mcmc_regularize: adds the gradients of  opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scale)).
 * scratch: dvs_mcmc_scratch_bytes(capacity) bytes, zeroed once with dvs_mcmc_init_scratch (the draw counters live there). */
typedef struct dvs_mcmc_sets { float* param[6]; float* m[6]; float* v[6]; } dvs_mcmc_sets;
size_t dvs_mcmc_scratch_bytes(int capacity);
int dvs_mcmc_init_scratch(void* stream, void* scratch, int capacity);
int dvs_mcmc_relocate(void* stream, int n, const dvs_mcmc_sets* sets, float min_opacity, uint32_t seed, int shn_layout, void* scratch,
                      int capacity, uint32_t* n_dead_out /* host (pinned), may be NULL */);
int dvs_mcmc_grow(void* stream, int n, int n_new, const dvs_mcmc_sets* sets, float min_opacity, uint32_t seed, int shn_layout, void* scratch,
                  int capacity);
int dvs_mcmc_add_noise(void* stream, int n, float* pos, const float* scale, const float* rot, const float* opacity, float lr, uint32_t seed);
int dvs_mcmc_regularize(void* stream, int n, const float* opacity, const float* scale, float* g_opacity, float* g_scale, float opacity_reg,
                        float scale_reg);
/* the same two for the splats [first, first + count) of the n (full-array pointers): bit-identical to the whole-array calls — the noise is a
 * function of the global splat index, the regularisers' means are over n. For a data-parallel step that updates its parameters chunk by chunk. */
int dvs_mcmc_add_noise_range(void* stream, int n, int first, int count, float* pos, const float* scale, const float* rot, const float* opacity, float lr,
                             uint32_t seed);
int dvs_mcmc_regularize_range(void* stream, int n, int first, int count, const float* opacity, const float* scale, float* g_opacity, float* g_scale,
                              float opacity_reg, float scale_reg);

/* ---- 3D smoothing filter (the world-space half of Mip-Splatting, arXiv 2311.16493; the screen-space half is dvs_opts.antialias) -----------
 * Every splat is convolved with an isotropic Gaussian of standard deviation filter[i] (world units): the highest rate at which a
 * training camera samples it, so that no view can see detail finer than any training pixel did. Element-wise kernels AROUND the
 * rasterizer: it reads the effective scale and opacity that apply writes, and chain takes its gradients back to the trained values.
 * All arrays DEVICE, fp32, 16-byte aligned; asynchronous on `stream`; DVS_ERR_INVALID for NULL or misaligned pointers, negative counts,
 * n_cams < 1 or a range outside [0, n).
 *
 * pack_cameras (HOST only): host_rows[16 c ..] = the three rows of camera c's world-to-camera transform (from `view`), then focal_x,
 *   width, height and one pad float. The caller copies the rows to the device.
 * compute: for camera c and splat i with camera-space (x, y, z), the camera SEES the splat iff z > 0.2, |x/z focal_x| <= 0.65 width and
 *   |y/z focal_x| <= 0.65 height (the paper code's near bound and 15 % margin; focal_x on both axes, as there). The principal point is
 *   taken as the image centre: off-centre intrinsics are not modelled, the margin absorbs them.
 *     filter[i] = sqrt(0.2) min over the seeing cameras of z / focal_x
 *   A splat no camera sees (a non-finite position never is) takes the maximum filter of the seen splats; 0 everywhere when none is seen.
 *   scratch: 16 bytes; afterwards scratch[0] = the bits of that maximum, scratch[1] = the number of seen splats.
 * apply_range: with s_k = exp(scale_k), f = filter[i], r_k = s_k^2 / (s_k^2 + f^2), c = sqrt(r_0 r_1 r_2), for the splats [first, first+count):
 *     scale_eff_k = 0.5 log(s_k^2 + f^2),   opacity_eff = logit(sigmoid(a) c),
 *   the logit formed from 1 - o' = sigmoid(-a) + sigmoid(a) (1 - c), finite for a in [-20, 20]. f == 0: bit-for-bit copies.
 * chain_range: in place, gradients with respect to the effective values -> with respect to the trained ones (scale, opacity: the trained):
 *     g_scale_k <- g_scale_k r_k + g_opacity (1 - r_k) / (1 - o'),   g_opacity <- g_opacity sigmoid(-a) / (1 - o').   f == 0: the identity.
 * The forms without _range are the same calls on (0, n); a range is bit-identical to those rows of the whole-array call. */
int dvs_filter3d_pack_cameras(const dvs_camera* cams, int n_cams, float* host_rows /* HOST [n_cams][16] */);
int dvs_filter3d_compute(void* stream, int n, const float* pos, const float* dev_cam_rows, int n_cams, float* filter, uint32_t* scratch);
int dvs_filter3d_apply_range(void* stream, int n, int first, int count, const float* scale, const float* opacity, const float* filter,
                             float* scale_eff, float* opacity_eff);
int dvs_filter3d_apply(void* stream, int n, const float* scale, const float* opacity, const float* filter, float* scale_eff, float* opacity_eff);
int dvs_filter3d_chain_range(void* stream, int n, int first, int count, const float* scale, const float* opacity, const float* filter,
                             float* g_scale, float* g_opacity);
int dvs_filter3d_chain(void* stream, int n, const float* scale, const float* opacity, const float* filter, float* g_scale, float* g_opacity);

#ifdef __cplusplus
}
#endif
#endif
