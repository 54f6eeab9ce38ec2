/*
 * va.h -- C ABI of the MI355X-native two-stream inference hot path
 *         (libva_hip.so, built from video_analytics_amd/csrc/ with hipcc for gfx950).
 *
 * The reference (arindamrc/video_analytics, Sheet03) has no FFI of its own: its hot path
 * is reached through three Python call surfaces.  Each entry point
 * below names the reference interface it stands behind:
 *
 *   va_vgg16_*        self.features(ip) (forward with only `feat` requested) + the classifierList
 *                     traversal (va_vgg16_classify) inside validate():
 *                     Sheet03/spatialModel.py:110-113,127-129,136-152,212-218 and the
 *                     temporal twin Sheet03/temporalModel.py:122-126,140-142,165-181,241-247.
 *   va_copy_first_layer   TemporalNetwork.__copyFirstLayer__: Sheet03/temporalModel.py:149-162.
 *   va_tvl1_flow      the upstream tool that wrote the flow_x_%04d.jpg / flow_y_%04d.jpg files
 *                     TemporalDataset reads: Sheet03/temporalModel.py:76-81,
 *                     Sheet03/parameters.py:27,38-39 (no reference function exists; the
 *                     algorithm is the published TV-L1).
 *   va_flow_to_stack  the 8-bit flow image + getTransforms' ToTensor/Normalize + the x/y
 *                     interleave of TemporalDataset.__getitem__: Sheet03/temporalModel.py:83-90,
 *                     Sheet03/utils.py:148-150.
 *   va_flow_to_stack_crop   va_flow_to_stack for full-size flow (UCF-101's 320x240) with getTransforms'
 *                     RandomCrop(224) / RandomHorizontalFlip() applied to each of the 2L flow images:
 *                     Sheet03/temporalModel.py:76-90, Sheet03/utils.py:143,145.
 *   va_crop_images_u8 the same crop and flip of the RGB frame SpatialDataset loads:
 *                     Sheet03/spatialModel.py:64-81, Sheet03/utils.py:143,145.
 *   va_flow_to_stack_views, va_crop_images_u8_views, va_view_mean   ten-crop evaluation (the test protocol of the
 *                     two-stream paper; no reference counterpart): V crop-and-flip views of every clip and the mean of
 *                     the per-view outputs.
 *   va_flow_to_stack_snippets, va_score_consensus, va_fuse_scores   whole-video evaluation (the test protocols the
 *                     reference's notes state, Sheet03/notes.txt:113-116 and 225-230: 25 snippets of a video, ten crops
 *                     of each, class scores averaged; fusion by averaging, notes.txt:121-124; no reference code):
 *                     DESIGN.md S14-S16.
 *   va_flow_field_means, va_flow_motion   mean flow subtraction and trajectory stacking, two of the temporal-ConvNet
 *                     inputs of the two-stream paper (no reference counterpart).
 *   va_flow_homography, va_flow_compensate   warped optical flow, TSN's camera-compensated temporal input
 *                     (Sheet03/notes.txt:187-194; no reference code): DESIGN.md S21, S22.
 *   va_frames_warp_pairs   the same in TSN's own two-pass form: the second frame of every pair warped by the fitted
 *                     homography for a second va_tvl1_flow (no reference code): DESIGN.md S53, S54.
 *   va_flow_quantize_u8, va_flowq_to_stack_snippets, va_flowq_to_stack_resize   stored optical flow: the flow images the
 *                     reference reads are computed once (Sheet03/temporalModel.py:76-81, Sheet03/parameters.py:27), as
 *                     TSN's are (Sheet03/notes.txt:196-199, 245-250); these keep them on the device: DESIGN.md S39-S41.
 *   va_validate_batch the loss / argmax / correct-count lines of validate():
 *                     Sheet03/spatialModel.py:219-221.
 *   va_meter_*        the per-video AverageMeter collation of validate():
 *                     Sheet03/utils.py:154-171, Sheet03/spatialModel.py:223-228.
 *   va_linear_svm_predict   LinearSVC.predict on the joined descriptors:
 *                     Sheet03/combinedModel.py:38.
 *   va_linear_svm_fit*      LinearSVC().fit on the same descriptors: Sheet03/combinedModel.py:34-35.
 *   va_pca_*, va_gmm_*, va_fisher_encode   PCA, the diagonal Gaussian mixture and the Fisher vector on the trajectory
 *                     descriptors: Sheet02/Sheet02.py:568-617.
 *   va_stip_*         the space-time interest points and HOG / HOF cuboids of findSTIPs(): Sheet01/Sheet01.py:129-256.
 *   va_kmeans_*, va_bow_*   makeCodebook() and makeVideoHistogram(): Sheet01/Sheet01.py:259-277.
 *   va_vgg16_train_*  the batch-loop body of train(): Sheet03/spatialModel.py:165-182;
 *   va_vgg16_export/import_state   checkpoint contents: Sheet03/spatialModel.py:234-260.
 *
 * Conventions
 *   - return 0 (VA_OK) or an error code; va_last_error() returns a thread-local message.
 *   - every data pointer is a DEVICE pointer (hipMalloc'ed; torch tensor.data_ptr()) unless
 *     a parameter comment says "host".  The caller owns all inputs, outputs and workspaces;
 *     the library owns only va_ctx and the packed-weight handle.  No hidden allocation and
 *     no host synchronisation inside va_vgg16_forward / va_tvl1_flow / va_flow_to_stack:
 *     all work is enqueued on `stream` (a hipStream_t; NULL = the null stream).
 *   - a handle may be used by one thread at a time; one process per GPU.  Every entry point selects its
 *     context's device itself (hipSetDevice); `stream` and all pointers must belong to that device.
 *   - the library reads NO environment variable and keeps no process-global switch: every tuning or test
 *     knob is a field of va_tvl1_params or a va_vgg16_set_option value of one handle.
 *   - there is NO CPU fallback in this library.
 */
#ifndef VA_H
#define VA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VA_OK 0
#define VA_ERR_INVALID 1   /* bad argument / shape: Python wrapper raises ValueError */
#define VA_ERR_HIP 2       /* HIP runtime failure: RuntimeError */
#define VA_ERR_WORKSPACE 3 /* workspace too small: ValueError */
#define VA_ERR_STOPPED 4   /* a test switch cut the call short (VA_OPT_TRAIN_STOP_AT): RuntimeError in production code */

#define VA_DTYPE_F32 0
#define VA_DTYPE_BF16 1

typedef struct va_ctx va_ctx;
typedef struct va_vgg16 va_vgg16;

/* version number (currently 6; bit 0x10000, which marked a build flavour that no longer exists, is never set) */
int va_version(void);
const char* va_last_error(void);
int va_ctx_create(int device, va_ctx** out);
void va_ctx_destroy(va_ctx* ctx);

/* ------------------------------------------------------------------ VGG-16 streams --- */

/*
 * Pack weights once.  conv_w[13]: f32 OIHW [Cout][Cin][3][3]; conv_b[13]: f32 [Cout];
 * fc_w[4]: f32 [out][in] with FC1's input index in the reference's flatten order
 * c*49 + h*7 + w (Sheet03/spatialModel.py:213); fc_b[4]: f32 [out].
 * c_in is 3 (spatial) or 2L (temporal, 20).  in_mean/in_std: HOST arrays of c_in floats used
 * only when va_vgg16_forward is given u8 input (ToTensor+Normalize, Sheet03/utils.py:148-150);
 * may be NULL.  dtype: VA_DTYPE_F32 (fp32 in, fp32 MFMA accumulate: the parity configuration) or
 * VA_DTYPE_BF16 (bf16 activations and conv weights on the bf16 MFMA, fp32 accumulate, fp32 classifier:
 * the throughput configuration of BASELINE config 5; class scores deviate at the 1e-2 level).
 * The call synchronises `stream` before returning (the source tensors may be freed).
 */
int va_vgg16_create(va_ctx* ctx, int c_in, int n_classes, int desc_dim, int dtype,
                    const void* const* conv_w, const void* const* conv_b,
                    const void* const* fc_w, const void* const* fc_b,
                    const float* in_mean, const float* in_std,
                    void* stream, va_vgg16** out);
void va_vgg16_destroy(va_vgg16* model);
size_t va_vgg16_workspace_bytes(const va_vgg16* model, int batch);

/*
 * A/B and test switches of ONE model handle (defaults are the measured choices of DESIGN.md; results of the
 * fp32 path do not depend on VA_OPT_F32_CONV_KERNEL):
 *   VA_OPT_BF16_VARIANT     0 (default) kernel, tile and staging scheme chosen per layer (measured); 1 = 64-channel
 *                           tiles with one LDS buffer on every layer; 2 = the LDS-DMA ring on every layer; 5 = the
 *                           two-group kernel (k_conv3x3_pp_bf16) on every layer with >= 128 output channels and >= 28x28
 *                           pixels (the default uses it on the 28x28 layers); 0, 1, 2, 5 and 7 add the same products in the
 *                           same order and agree bit for bit.  6 (a halo-brick form of the two-group kernel that
 *                           measured no faster and was removed: DESIGN.md section 7) is refused with VA_ERR_INVALID.
 *                           7 = the weights-resident kernel (k_conv3x3_ws_bf16) on
 *                           both layers with 64 input channels (the default uses it on conv1_2 only); bit-equal to 0, 1, 2, 5.
 *                           (3 and 4, round 2's first halo-brick kernel, are gone.)
 *   VA_OPT_BF16_FIRST_LAYER 1 (default) the first layer reads the NCHW input itself (k_conv1_fused_bf16); 0 = the input is
 *                           first staged as a 64-channel NHWC tensor and convolved in three K steps (the round-1 path;
 *                           another fp32 summation order: bf16-level agreement).  Independent of VA_OPT_BF16_VARIANT
 *   VA_OPT_F32_CONV_KERNEL  1 (default) LDS-DMA staged fp32 kernel where Cin % 32 == 0; 0 = register-staged kernel
 *   VA_OPT_TRAIN_STOP_AT    -1 (default) full training step; i in [0,12]: va_vgg16_train_step returns
 *                           VA_ERR_STOPPED after the backward pass of conv layer i, leaving the gradient buffers
 *                           as that layer left them and the layers below WITHOUT their update (tests only)
 */
#define VA_OPT_BF16_VARIANT 1
#define VA_OPT_F32_CONV_KERNEL 2
#define VA_OPT_TRAIN_STOP_AT 3
#define VA_OPT_BF16_FIRST_LAYER 4
int va_vgg16_set_option(va_vgg16* model, int option, int value);

/*
 * x: f32 (x_is_u8 = 0) or u8 (x_is_u8 = 1) [batch][c_in][224][224] NCHW.
 * feat: f32 [batch][512][7][7] NCHW or NULL; desc: f32 [batch][desc_dim] (post-ReLU output of
 * classifier index 8) or NULL; logits: f32 [batch][n_classes] (no softmax) or NULL.
 * VA_DTYPE_BF16 models: batch <= 334 (a layer's activations are addressed with 32-bit byte offsets; VA_ERR_INVALID
 * beyond that: split the batch).
 */
int va_vgg16_forward(va_vgg16* model, const void* x, int x_is_u8, int batch,
                     void* feat, void* desc, void* logits,
                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * The classifier traversal alone (Sheet03/spatialModel.py:213-218): feat f32 [batch][512][7][7]
 * NCHW (as returned through `feat` above; flattened CHW-major) -> desc / logits (either may be
 * NULL).  va_vgg16_forward(x) == va_vgg16_classify(features(x)).
 */
int va_vgg16_classify(va_vgg16* model, const void* feat, int batch, void* desc, void* logits,
                      void* workspace, size_t workspace_bytes, void* stream);

/* w_rgb f32 [cout][3][3][3] -> w_out f32 [cout][n_in][3][3]: mean over the 3 input channels,
 * accumulated in channel order then divided by 3, replicated n_in times. */
int va_copy_first_layer(va_ctx* ctx, const void* w_rgb, int cout, int n_in, void* w_out, void* stream);

/* logits f32 [batch][n_classes], labels i64 [batch] -> out f32[2] (device):
 * out[0] = mean cross-entropy over the batch, out[1] = number of argmax(first max)==label. */
int va_validate_batch(va_ctx* ctx, const void* logits, const void* labels, int batch, int n_classes,
                      void* out, void* stream);

/* ------------------------------------------------------------------ TV-L1 flow ------- */

typedef struct va_tvl1_params {
    float tau;        /* 0.25 */
    float lambda;     /* 0.15 */
    float theta;      /* 0.3  */
    int nscales;      /* 5; pyramid levels wanted: fewer are used where the next level would be under 16 pixels wide or
                         high, and never more than 16 (a larger value is read as 16, not rejected) */
    int warps;        /* 5    */
    float epsilon;    /* 0.01; <= 0: run exactly `iters` inner iterations per warp */
    int iters;        /* 300  */
    float scale_step; /* 0.8; in (0,1).  The zoom-out Gaussian (sigma = 0.6 sqrt(1/step^2 - 1)) has radius
                         min((int)(3 sigma) + 1, 8): the clamp to 8 applies for scale_step <= 0.2195 */
    int block_iters;  /* inner iterations fused per launch (register-resident temporal
                         blocking); 0 = library default.  Results do not depend on it.
                         Forced to 1 when epsilon > 0. */
    int fast_math;    /* 0 (default): the exact arithmetic contract of DESIGN.md (correctly rounded
                         sqrt and division): results bit-identical to the CPU oracle.
                         1: the two special functions of the dual update use the 1-ulp hardware
                         v_sqrt_f32 / v_rcp_f32 (measured: 11 % more clips/s; flow within 7e-6 px on average
                         of the exact mode, 99.9 % of the pixels within 1e-3 px). */
    int tile_mask;    /* tuning/testing: bit i allows register-tile candidate i of the inner-iteration
                         kernel (bits 0-3: 256x32, 128x64, 84x96, 64x128 pixels, one 8-wave workgroup
                         per CU; bits 4-7: 256x16, 128x32, 84x48, 64x64, two 4-wave workgroups per
                         CU).  Bit 8 (256): iterate every level with the streaming kernel (a wave carries a
                         128-column strip row by row through 10 iterations per pass) instead of the
                         register tiles; fixed-iteration mode only.  Bit 9 (512): reserved, must be 0 (it selected a
                         kernel that was removed; refused with VA_ERR_INVALID).  Bit 10 (1024): the streaming kernel never lets the narrow last strips of two
                         pairs share a wave (A/B switch).  0 (default) = library choice per level.  Results do not depend on it. */
    int tuning[8];    /* the library's own tuning switches (which kernel iterates which pyramid level, chunking of
                         rows, pipeline shapes: named in csrc/va_internal.h, VA_TUNE_*); va_tvl1_default_params fills in the
                         defaults (-1, 0, 0, 0, -1, 0, 0, 0) and callers leave them alone.  Results do not depend on any
                         of them; the library reads no environment variable.  Slots 4, 6 and 7 are reserved, must be 0 (or
                         -1 for slot 4).  Values that selected a kernel family since removed (measured slower: DESIGN.md
                         section 7) are rejected with VA_ERR_INVALID. */
} va_tvl1_params;

void va_tvl1_default_params(va_tvl1_params* p);

/* Number of pyramid levels actually used and their sizes (ws/hs: HOST arrays of >= 16 ints). */
int va_tvl1_pyramid_sizes(int w, int h, const va_tvl1_params* p, int* ws, int* hs);

/* The register tiling va_tvl1_flow will use, level by level (host logic; HOST array of >= 6*16 ints): per level
 * { tile width, tile height, waves per workgroup, block depth K, tiles in x, tiles in y }; a level that streams
 * reports { strip width (64 x pixels per lane: 128 or 192), 0 (rows stream through), waves of the row pipeline (2 or 1), iterations per pass
 * (16 with two waves, 10 with one), strips in x, 0 (chunks of rows: chosen per call from the number of pairs) }.
 * Returns the number of levels (0 on bad arguments). */
int va_tvl1_tile_plan(int w, int h, const va_tvl1_params* p, int* out);

size_t va_tvl1_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p);

/*
 * frames: u8 (frames_are_u8 = 1) or f32 in [0,255] [n_seq][frames_per_seq][h][w] gray.
 * flow:   f32 [n_seq*(frames_per_seq-1)][2][h][w]; plane 0 = x flow, plane 1 = y flow of the
 *         pair (frame k, frame k+1) of each sequence.
 */
int va_tvl1_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq,
                 int w, int h, const va_tvl1_params* p, void* flow,
                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * Options carried beside va_tvl1_params (which keeps its size).  DESIGN.md S55: the flow is median filtered between
 * blocks of inner iterations, as the TV-L1 of OpenCV's CPU class does (median 5, median_every 30 with iters 300 are its
 * defaults; OpenCV's CUDA class, and this library without the option, do not filter).
 *   struct_bytes  sizeof(va_tvl1_options) of the caller; a smaller value is refused.
 *   median        0 (off), 3 or 5: at the head of inner iteration `it` of every warp, for every it with
 *                 it % median_every == 0, u1 and u2 are each replaced by their median x median median (window centred on
 *                 the pixel, coordinates clamped to the level's frame, exact selection; the dual variables stay).  With
 *                 epsilon > 0 a pair that has met the stopping rule in a warp is not filtered again in it.
 *   median_every  >= 0 inner iterations between two filters; 0 = iters: once per warp.
 * opt = NULL or median = 0: va_tvl1_flow's result and va_tvl1_workspace_bytes' count, bit for bit.  Values out of range
 * give VA_ERR_INVALID (a byte count of 0) and a message naming the field before anything is launched.  Results do not
 * depend on block_iters, tile_mask or tuning with the option either; fast_math is independent of it.
 */
typedef struct va_tvl1_options { int struct_bytes; int median; int median_every; } va_tvl1_options;
size_t va_tvl1_workspace_bytes_opt(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p, const va_tvl1_options* opt);
int va_tvl1_flow_opt(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                     const va_tvl1_params* p, const va_tvl1_options* opt, void* flow, void* workspace, size_t workspace_bytes,
                     void* stream);

/*
 * The launches va_tvl1_flow_opt makes for a call of this shape, from the code that makes them (the level, chunk, warp and
 * iteration loop runs dry: nothing is launched and no device is needed).  One record per inner-iteration launch and per
 * median launch, in launch order:
 *   level, warp     pyramid level (0 = the frame) and warp of the level
 *   pair0, npairs   the chunk of pairs the launch covers (a register-tile level whose pairs exceed the cache runs them
 *                   chunk by chunk: all warps of chunk 0, then chunk 1, ...)
 *   w, h, pitch     the level's size and its row pitch in floats
 *   family          VA_TVL1_LAUNCH_TILE (k_iter_tile), _STREAM (k_iter_stream) or _MEDIAN (k_median)
 *   cfg             tile: the candidate (bit of tile_mask) 0..7; otherwise -1
 *   waves, levels   tile: waves per workgroup, 0; stream: waves x levels per wave of the pipeline; median: 0, 0
 *   eps, fast       the EPS and FAST template arguments (median: eps = the stopping rule is on, fast = 0)
 *   median          median: the window (3 or 5); otherwise 0
 *   K, it0          iterations the launch runs and the first of them within the warp (median: 0 and the iteration at whose
 *                   head it filters)
 *   grid_x, grid_y  the launch grid
 *   strips, row_chunks, rows_per_chunk, halo_x
 *                   stream: strips in x, chunks of rows, rows per chunk, x halo; tile: tiles in x, tiles in y, tile height,
 *                   x halo; median: tiles in x, tiles in y, tile height, window radius
 *   narrow, rev     stream: the last strips of two pairs share a wave; the workgroup order is reversed (tile and stream)
 * records: HOST array of `capacity` records (NULL with capacity 0 to count).  Returns the number of launches of the call
 * (only the first `capacity` are written), or -1 on bad arguments (va_last_error names the parameter).
 */
enum { VA_TVL1_LAUNCH_TILE = 0, VA_TVL1_LAUNCH_STREAM = 1, VA_TVL1_LAUNCH_MEDIAN = 2 };
typedef struct va_tvl1_launch {
    int level, warp, pair0, npairs;
    int w, h, pitch;
    int family, cfg, waves, levels;
    int eps, fast, median;
    int K, it0;
    int grid_x, grid_y;
    int strips, row_chunks, rows_per_chunk, halo_x;
    int narrow, rev;
} va_tvl1_launch;
int va_tvl1_launch_plan(int w, int h, int n_seq, int frames_per_seq, const va_tvl1_params* p, const va_tvl1_options* opt,
                        va_tvl1_launch* records, int capacity);

/*
 * The filter of S55 on stored flow: flow f32 [n_fields][2][h][w] -> out of the same shape, every plane replaced by its
 * ksize x ksize median (ksize 3 or 5; any w, h >= 1: a plane narrower than the window is legal).  Only finite values
 * are specified; -0.0 and +0.0 compare equal.  out must not overlap flow (VA_ERR_INVALID).
 */
int va_flow_median(va_ctx* ctx, const void* flow, int n_fields, int w, int h, int ksize, void* out, void* stream);

/* ------------------------------------------------------------------ Brox flow -------- */

/*
 * The flow method of the two-stream paper (Sheet03/notes.txt:11-16): Brox, Bruhn, Papenberg, Weickert, "High accuracy
 * optical flow estimation based on a theory for warping", ECCV 2004, in the form of IPOL's "Robust Optical Flow
 * Estimation" (Sanchez, Monzon, Salgado 2013).  DESIGN.md S57-S62 are the specification: constancy of the intensity and
 * of its gradient, a robust smoothness term, lagged nonlinearities, red-black SOR.  Values out of range (alpha <= 0,
 * gamma < 0, scale_step outside (0,1), omega outside (0,2), epsilon <= 0, a count < 1, a tuning value with no kernel
 * shape) give VA_ERR_INVALID, or a byte count of 0, and a message naming the field before anything is launched.
 */
typedef struct va_brox_params {
    int struct_bytes;  /* sizeof(va_brox_params) of the caller; a smaller value is refused */
    float alpha;       /* 0.197; weight of the smoothness term (frames are scaled to [0,1]) */
    float gamma;       /* 50; weight of the gradient-constancy term; 0 turns it off */
    float scale_step;  /* 0.8; in (0,1): the pyramid of S1 */
    float omega;       /* 1.9; SOR relaxation, in (0,2) */
    float epsilon;     /* 1e-3; the regulariser under every square root, > 0 */
    int nscales;       /* 16: as deep as S1 allows (levels stop before min(w,h) < 16; a larger value is read as 16) */
    int warps;         /* 1; warps (outer iterations) per level */
    int inner_iters;   /* 10; lagged-nonlinearity steps per warp */
    int solver_iters;  /* 10; red-black SOR sweeps per step */
    int tuning[8];     /* shapes of the inner-step kernel (csrc/va_internal.h, VA_BROX_TUNE_*); va_brox_default_params fills
                          in (-1, 0, 0, 0, 0, 0, 0, 0).  Results do not depend on any of them. */
} va_brox_params;

void va_brox_default_params(va_brox_params* p);

/* Needs no device.  0 and a va_last_error text on bad parameters or sizes (w, h in [16,16384]). */
size_t va_brox_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_brox_params* p);

/* va_tvl1_flow's arguments and output layout: frames u8 or f32 in [0,255] [n_seq][frames_per_seq][h][w] gray ->
 * flow f32 [n_seq*(frames_per_seq-1)][2][h][w]. */
int va_brox_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                 const va_brox_params* p, void* flow, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test entry: exactly one inner step of S60-S61 (the coefficients from du, dv as they come in, then solver_iters red-black
 * SOR sweeps) on n fields of w x h dense f32 device arrays [n][h][w], in place on du, dv.  The step reads I1wx .. I1wyy,
 * Iz, Ixz, Iyz, u, v; I0x, I0y and I1w enter only through the differences and are not read.  scratch: 256-byte aligned,
 * >= 4*n*w*h floats (the ping-pong fields of the tiled launches).  w, h in [16,16384].
 */
int va_brox_inner_step(va_ctx* ctx, const void* I0x, const void* I0y, const void* I1w, const void* I1wx, const void* I1wy,
                       const void* I1wxx, const void* I1wxy, const void* I1wyy, const void* Iz, const void* Ixz,
                       const void* Iyz, const void* u, const void* v, void* du, void* dv, int n, int w, int h,
                       const va_brox_params* p, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ Farneback flow --- */

/*
 * The third dense flow method: G. Farneback, "Two-frame motion estimation based on polynomial expansion", SCIA 2003, in
 * the structure of OpenCV's calcOpticalFlowFarneback (the one flow method the modelled project calls by name:
 * Sheet01.py:79, Sheet02.py:191; the defaults below are that call's arguments).  DESIGN.md S63-S67 are the specification:
 * S1's pyramid, a quadratic fitted around every pixel, `iterations` passes per level of matrix update, window sum and 2x2
 * solve.  It is the build's own specification, not OpenCV's arithmetic: no bit parity with OpenCV is claimed.  Values out of
 * range (pyr_scale outside (0,1), winsize even or < 3 or > 63, poly_n not 5 or 7, poly_sigma <= 0, gaussian not 0 or 1, a
 * count < 1, a tuning value with no kernel shape) give VA_ERR_INVALID, or a byte count of 0, and a message naming the field
 * before anything is launched.
 */
typedef struct va_farneback_params {
    int struct_bytes;  /* sizeof(va_farneback_params) of the caller; a smaller value is refused */
    float pyr_scale;   /* 0.5; in (0,1): S1's scale_step */
    float poly_sigma;  /* 1.2; standard deviation of the Gaussian applicability of the polynomial expansion, > 0 */
    int levels;        /* 3; S1's nscales: levels stop before min(w,h) < 16, a larger value is read as the deepest S1 allows */
    int winsize;       /* 15; side of the averaging window, odd, in [3,63] */
    int iterations;    /* 3; passes per level */
    int poly_n;        /* 5; radius of the applicability: 5 or 7 */
    int gaussian;      /* 0: box window; 1: Gaussian window of the same support (OPTFLOW_FARNEBACK_GAUSSIAN) */
    int tuning[8];     /* tile shapes of the two kernels (csrc/va_internal.h, VA_FARNEBACK_TUNE_*); 0 = the library's choice.
                          Results do not depend on any of them. */
} va_farneback_params;

void va_farneback_default_params(va_farneback_params* p);

/* Needs no device.  0 and a va_last_error text on bad parameters or sizes (w, h in [16,16384]). */
size_t va_farneback_workspace_bytes(int w, int h, int n_seq, int frames_per_seq, const va_farneback_params* p);

/* va_tvl1_flow's arguments and output layout: frames u8 or f32 in [0,255] [n_seq][frames_per_seq][h][w] gray ->
 * flow f32 [n_seq*(frames_per_seq-1)][2][h][w]. */
int va_farneback_flow(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                      const va_farneback_params* p, void* flow, void* workspace, size_t workspace_bytes, void* stream);

/* Test entry: S64 alone.  fields f32 [n][h][w] -> coef f32 [n][5][h][w]: (b_x, b_y, a_xx, a_yy, a_xy).  w, h in [16,16384]. */
int va_farneback_polyexp(va_ctx* ctx, const void* fields, int n, int w, int h, const va_farneback_params* p, void* coef,
                         void* stream);

/*
 * Test entry: exactly one pass of S65-S67 on n pairs.  coef0, coef1 f32 [n][5][h][w] (the first and the second frame's
 * coefficients), flow_in f32 [n][2][h][w] -> flow_out of the same shape, which must not be flow_in.  w, h in [16,16384].
 */
int va_farneback_pass(va_ctx* ctx, const void* coef0, const void* coef1, const void* flow_in, void* flow_out, int n, int w,
                      int h, const va_farneback_params* p, void* stream);

/* ------------------------------------------------------------------ Dense trajectories */

/*
 * Dense trajectories (Wang, Klaeser, Schmid, Liu, CVPR 2011) with the constants of the modelled project's Sheet02.py:26-38:
 * points sampled on a grid where the gray frame has structure, followed through the 3x3-median-filtered flow for `length`
 * frames, and HOG / HOF / MBHx / MBHy histograms collected in a patch x patch x length tube of nxy x nxy x nt cells around
 * each track.  DESIGN.md S69-S76 are the specification; it is the build's own (no parity with OpenCV or with Sheet02's
 * arithmetic is claimed).  Orientation votes are quantised to fixed point, every later sum is an integer sum: no result
 * depends on a reduction order or on a tuning value.  Values out of range (length not a multiple of nt, patch not a multiple
 * of nxy, patch / nxy > 64, step < 2, quality outside (0,1), a threshold <= 0, a tuning value with no kernel shape) give
 * VA_ERR_INVALID, or a byte count of 0, and a message naming the field before anything is launched.
 */
typedef struct va_dtraj_params {
    int struct_bytes;     /* sizeof(va_dtraj_params) of the caller; a smaller value is refused */
    int step;             /* 5; side of a sampling grid cell in pixels, >= 2 */
    int length;           /* 15; steps of a trajectory (it has length + 1 points), a multiple of nt */
    int patch;            /* 32; side of the tube in pixels, a multiple of nxy, patch / nxy <= 64 */
    int nxy;              /* 2; cells across and down the tube */
    int nt;               /* 3; cells along the tube */
    float quality;        /* 0.001; a point starts where the corner response exceeds quality * the frame's maximum */
    float min_flow;       /* 0.4; HOF: a flow vector no longer than this votes into the ninth bin */
    float min_std;        /* 1.7320508; standard deviation (pixels) of x and of y below which a trajectory is static */
    float max_std;        /* 30; standard deviation of x or of y above which it is erratic */
    float max_dis;        /* 20; longest step in pixels above which it is a jump */
    float max_dis_share;  /* 0.7; share of the whole length one step may have */
    int tuning[8];        /* chunk length and tile shape (csrc/va_internal.h, VA_DTRAJ_TUNE_*); 0 = the library's choice.
                             Results do not depend on any of them. */
} va_dtraj_params;

void va_dtraj_default_params(va_dtraj_params* p);

/* Needs no device.  0 and a va_last_error text on bad parameters or sizes (w, h in [16,16384], n_frames in [2,65536],
 * capacity >= 1).  The bytes hold the track table of (w/step)(h/step) * length slots and one chunk of frames: 33 planes of
 * votes and 33 integral planes each. */
size_t va_dtraj_workspace_bytes(int w, int h, int n_frames, int capacity, const va_dtraj_params* p);

/*
 * gray u8 or f32 in [0,255] [n_frames][h][w]; flow f32 [n_frames-1][2][h][w] and flow_median, the same flow after
 * va_flow_median with ksize 3 -> desc f32 [capacity][2*length + 33*nt*nxy*nxy] (shape | HOG | HOF | MBHx | MBHy; 426 values
 * at the defaults), points f32 [capacity][length+1][2] (x, y), starts i32 [capacity] (first frame), in order of the last
 * frame, then of the track.  *count (host) is the number of trajectories FOUND: when it exceeds capacity only the first
 * `capacity` were written and the caller must say so.  rejected (host, 5 ints): left the frame, static, erratic, jump,
 * still unfinished behind the last frame.  The call synchronises the stream once, at its end, to read these counts.
 * workspace: 256-byte aligned, >= va_dtraj_workspace_bytes (VA_ERR_WORKSPACE otherwise).
 */
int va_dtraj_extract(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, const void* flow_median, int n_frames,
                     int w, int h, const va_dtraj_params* p, void* desc, void* points, void* starts, int capacity, int* count,
                     int* rejected, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test entries, one per stage.  The track table is one device buffer, `state`, of va_dtraj_state_layout bytes (needs no
 * device; 0 on bad values); offsets receives up to 8 byte offsets of its regions:
 *   0 counts  i32 [16]: live tracks, current list (0 or 1), trajectories found, found before the last finish, rejected
 *             [4..7] (left, static, erratic, jump)
 *   1 lists   i32 [2][slots]: the slots of the live tracks in track order; slots = (w/step)(h/step) * length
 *   2 status  i32 [slots] by list position, left by a step: 0 alive, 1 left the frame, 2 has `length` steps
 *   3 start   i32 [slots]: first frame of the slot's track; a track that starts at frame t in grid cell c owns slot
 *             (t mod length) * cells + c
 *   4 points  f32 [slots][length+1][2]
 *   5 sums    u64 [slots][nt][nxy*nxy][33]
 *   6 occupancy i32 [cells], all 0 between calls        7 i32 [slots]: the slots the last finish wrote out
 */
size_t va_dtraj_state_layout(int w, int h, const va_dtraj_params* p, size_t* offsets, int capacity);

/* S69-S71: gray [n][h][w], unfiltered flow f32 [n][2][h][w] -> votes u32 [n][33][h][w]
 * (planes: HOG 0-7, HOF 8-16, MBHx 17-24, MBHy 25-32). */
int va_dtraj_votes(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, int n, int w, int h,
                   const va_dtraj_params* p, void* votes, void* stream);

/* S72: u32 [planes][h][w] -> u32 [planes][h+1][w+1], sums mod 2^32; w, h in [1,16384]. */
int va_dtraj_integral(va_ctx* ctx, const void* votes, int planes, int w, int h, void* integral, void* stream);

/* S73: gray [n][h][w] -> response f32 [n][h][w] and max_bits u32 [n], the bit pattern of each frame's largest response. */
int va_dtraj_corner(va_ctx* ctx, const void* gray, int gray_is_u8, int n, int w, int h, void* response, void* max_bits,
                    void* stream);

/* S74: one frame's response [h][w] and max_bits [1]; appends the tracks that start at `frame` to the state. */
int va_dtraj_sample(va_ctx* ctx, const void* response, const void* max_bits, int w, int h, int frame,
                    const va_dtraj_params* p, void* state, void* stream);

/* S75: one frame's integral planes u32 [33][h+1][w+1] and median-filtered flow f32 [2][h][w]; every live track adds its
 * slice, moves, and gets its status. */
int va_dtraj_step(va_ctx* ctx, const void* integral, const void* flow_median, int w, int h, int frame,
                  const va_dtraj_params* p, void* state, void* stream);

/* S76: the tracks with `length` steps are tested and written out (as va_dtraj_extract writes them, from index counts[2]
 * on), the alive ones go to the other list, the counts are updated. */
int va_dtraj_finish(va_ctx* ctx, int w, int h, const va_dtraj_params* p, void* state, void* desc, void* points, void* starts,
                    int capacity, void* stream);

/* ------------------------------------------------------------------ Space-time interest points */

/*
 * Space-time interest points (Laptev, "On space-time interest points", IJCV 2005) with HOG / HOF cuboid descriptors, with
 * the constants of the modelled project's Sheet01.py:13-23.  DESIGN.md S83-S90 are the specification; it is the build's own
 * (no parity with Sheet01's arithmetic is claimed; S90 lists what Sheet01 does by accident and this library does not).  The
 * volume is [T][h][w].  Per scale pair (sigma, tau): L = g(sigma, sigma, tau) * f, np.gradient's derivatives, the six
 * products smoothed with (s sigma, s sigma, s tau), H = det - k trace^3, strict local maxima above min_response, and around
 * each a cuboid of nx x ny x nt cells of `bins` orientation bins of (Lx, Ly) and of the flow.  Smoothing is float32 in one
 * written order (the same bits under every tile shape); votes are fixed point and every later sum an integer sum.
 * Values out of range give VA_ERR_INVALID, or a byte count of 0, and a message naming the field before anything is launched.
 */
#define VA_STIP_MAX_SIGMAS 8
#define VA_STIP_MAX_TAUS 4
#define VA_STIP_MAX_RADIUS 512
typedef struct va_stip_params {
    int struct_bytes;      /* sizeof(va_stip_params) of the caller; a smaller value is refused */
    int n_sigmas;          /* 6; spatial scales in use, 1..8 */
    int n_taus;            /* 2; temporal scales in use, 1..4 */
    float sigmas[VA_STIP_MAX_SIGMAS]; /* 2^((1+i)/2), i = 1..6; each > 0 with int(4 s sigma + 0.5) <= 512 */
    float taus[VA_STIP_MAX_TAUS];     /* 2^(j/2), j = 1, 2; likewise */
    float integration;     /* 2.0; s: the products are smoothed with (s sigma, s sigma, s tau) */
    float k;               /* 0.005; H = det - k trace^3 */
    float min_response;    /* 0; a point has H > min_response (finite) */
    float cuboid;          /* 9; the cuboid's sides are 2 cuboid sigma (x, y) and 2 cuboid tau (t) */
    int neighbours;        /* 6 (the axes, Sheet01's rule) or 26 (Laptev's full neighbourhood) */
    int nx, ny, nt;        /* 3, 3, 2; cells of a cuboid, each 1..8 */
    int bins;              /* 4; orientation bins of 360 / bins degrees, 2..16; 2 nx ny nt bins <= 512 */
    int tuning[8];         /* tile shapes of the smoothing passes (csrc/va_internal.h, VA_STIP_TUNE_*); 0 = the library's
                              choice.  Results do not depend on any of them. */
} va_stip_params;

void va_stip_default_params(va_stip_params* p);

/* Needs no device.  0 and a va_last_error text on bad parameters or sizes (w, h in [1,16384], n_frames in [2,65535],
 * w h n_frames < 2^31, capacity >= 1).  The bytes hold ten float volumes (L, six products, two pass buffers, H), one volume
 * of `bins` vote planes and two of integral planes, the row counts and the taps: one scale pair's worth, reused by all. */
size_t va_stip_workspace_bytes(int w, int h, int n_frames, int capacity, const va_stip_params* p);

/*
 * gray u8 or f32 in [0,255] [n_frames][h][w]; flow f32 [n_frames-1][2][h][w] (the field of the last pair stands in for the
 * last frame) -> points i32 [capacity][5] (x, y, t, sigma index, tau index), response f32 [capacity] (H there), desc f32
 * [capacity][2 nx ny nt bins] (HOG | HOF, cells in (t, y, x) order, divided by the L2 norm of the whole; a zero norm gives
 * zeros), in the order scale pair (sigma outer, tau inner), t, y, x.  *count (host) is the number of points FOUND: when it
 * exceeds capacity only the first `capacity` were written and the caller must say so.  The call synchronises the stream
 * twice: after the taps are uploaded, and at its end to read the count.
 * workspace: 256-byte aligned, >= va_stip_workspace_bytes (VA_ERR_WORKSPACE otherwise).
 */
int va_stip_extract(va_ctx* ctx, const void* gray, int gray_is_u8, const void* flow, int n_frames, int w, int h,
                    const va_stip_params* p, void* points, void* response, void* desc, int capacity, int* count,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Test entries, one per stage. */

/* S83: the taps g[0..r] of sigma as the device uses them; returns r = int(4 sigma + 0.5), or -1 (sigma <= 0, r > 512 or
 * capacity < r + 1).  Needs no device. */
int va_stip_taps(double sigma, float* taps, int capacity);

/* S84: src u8 or f32 [n_frames][h][w] -> dst f32, smoothed with sigma along x and y and tau along t (reflected borders).
 * tmp: device scratch of tmp_floats >= 2 n_frames h w + 2048 floats, 256-byte aligned.  p supplies the tuning only.
 * n_frames, w, h >= 1 here.  dst may not alias src or tmp. */
int va_stip_smooth(va_ctx* ctx, const void* src, int src_is_u8, int n_frames, int w, int h, double sigma, double tau,
                   const va_stip_params* p, void* dst, void* tmp, size_t tmp_floats, void* stream);

/* S85: L f32 [n_frames][h][w] -> products f32 [6][n_frames][h][w]: LxLx, LyLy, LtLt, LxLy, LxLt, LyLt. */
int va_stip_gradient_products(va_ctx* ctx, const void* L, int n_frames, int w, int h, void* products, void* stream);

/* S86: the six smoothed products -> H f32 [n_frames][h][w]. */
int va_stip_response(va_ctx* ctx, const void* products, int n_frames, int w, int h, float k, void* H, void* stream);

/* S87: H -> the maxima appended to points / response from index counts[0] on (never past capacity), tagged with the two
 * scale indices.  counts: device i32 [16]; [0] points found so far (in and out), [1] its value before this call.
 * scratch: device i32 [2 n_frames h + 256]. */
int va_stip_maxima(va_ctx* ctx, const void* H, int n_frames, int w, int h, float min_response, int neighbours, int sigma_index,
                   int tau_index, void* points, void* response, int capacity, void* counts, void* scratch, void* stream);

/* S88: L f32 [n_frames][h][w] and flow f32 [n_frames-1][2][h][w] -> hog, hof u32 [n_frames][bins][h][w]; either output
 * (with its input) may be NULL.  n_frames >= 2. */
int va_stip_votes(va_ctx* ctx, const void* L, const void* flow, int n_frames, int w, int h, const va_stip_params* p, void* hog,
                  void* hof, void* stream);

/* S89: points i32 [n][5] and the integral planes u32 [n_frames][bins][h+1][w+1] of both groups (va_dtraj_integral of the
 * votes) -> desc f32 [n][2 nx ny nt bins]. */
int va_stip_describe(va_ctx* ctx, const void* points, int n, const void* hog_integral, const void* hof_integral, int n_frames,
                     int w, int h, const va_stip_params* p, void* desc, void* stream);

/*
 * flow f32 [n_pairs][2][h][w] -> stack f32 [2*n_pairs][h][w]: channel 2k = x flow of pair k,
 * 2k+1 = y flow (Sheet03/temporalModel.py:83).  Each value is quantised to the 8-bit flow
 * image convention q = rint(clamp(255*(v+bound)/(2*bound), 0, 255)) and then normalised as
 * (q/255 - mean)/std (Sheet03/utils.py:148-150; single-channel rule: mean 0.485, std 0.229).
 */
int va_flow_to_stack(va_ctx* ctx, const void* flow, int n_pairs, int w, int h,
                     float bound, float mean, float stdv, void* stack, void* stream);

/*
 * va_flow_to_stack with a crop and flip per output channel (DESIGN.md S10 then S9; Sheet03/temporalModel.py:76-90, the
 * transform applied to each flow image independently at :86; Sheet03/utils.py:143,145,148-150).
 * flow f32 [n_pairs][2][h][w] -> stack f32 [2*n_pairs][out_h][out_w].
 * crops: DEVICE int32 [2*n_pairs][3] = {top, left, flip}, one per output channel (channel 2k = x flow of pair k).
 * Output pixel (y, x) of channel ch reads source (top + y, left + (flip ? out_w-1-x : x)) of its plane, then quantises and
 * normalises it exactly as va_flow_to_stack does.  A flip mirrors the quantised image and does not negate the x flow.
 * top and left are clamped to [0, h-out_h] x [0, w-out_w] on the device; callers validate them on the host.
 */
int va_flow_to_stack_crop(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean, float stdv,
                          const void* crops, int out_w, int out_h, void* stack, void* stream);

/*
 * The crop and flip of getTransforms() on u8 frames (Sheet03/spatialModel.py:64-81, Sheet03/utils.py:143,145):
 * src u8 [n][c][h][w] (src_nhwc = 0) or [n][h][w][c] (src_nhwc = 1, the decode order of PIL and JPEG);
 * crops: DEVICE int32 [n][3] = {top, left, flip}, one per image, shared by its channels (clamped like
 * va_flow_to_stack_crop's); dst u8 [n][c][out_h][out_w] NCHW: the u8 input of va_vgg16_forward, which applies
 * ToTensor + Normalize (Sheet03/utils.py:148-150).
 */
int va_crop_images_u8(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc,
                      const void* crops, int out_w, int out_h, void* dst, void* stream);

/*
 * V views of every clip (ten-crop evaluation): flow f32 [n_clips*flow_count][2][h][w] -> stack f32
 * [n_clips][n_views][2*flow_count][out_h][out_w].  Output plane o = (b*n_views + v)*2L + c (L = flow_count; c = 2k is the
 * x flow of pair k, 2k+1 its y flow) reads source plane b*2L + c through crops row o, then quantises and normalises it as
 * va_flow_to_stack_crop does.  crops: DEVICE int32 [n_clips*n_views*2L][3] = {top, left, flip}, one row per output plane
 * (clamped on the device like va_flow_to_stack_crop's).  invert_x_on_flip = 1: a flipped x-flow plane (c even) is also
 * inverted, q -> 255 - q, before the normalisation (the TSN convention: mirroring reverses horizontal motion); 0: the
 * reference's mirror without inversion.  n_views = 1 with per-plane crops gives the reference's random crops with TSN
 * flips.  At most 65535 output planes per call.
 */
int va_flow_to_stack_views(va_ctx* ctx, const void* flow, int n_clips, int flow_count, int n_views, int w, int h,
                           float bound, float mean, float stdv, const void* crops, int invert_x_on_flip, int out_w,
                           int out_h, void* stack, void* stream);

/*
 * V views of every image: src u8 [n][c][h][w] (src_nhwc = 0) or [n][h][w][c] (src_nhwc = 1) -> dst u8
 * [n][n_views][c][out_h][out_w]; output image i reads source image i / n_views through crops row i.
 * crops: DEVICE int32 [n*n_views][3] = {top, left, flip}.  At most 65535 output planes (n*n_views*c) per call.
 */
int va_crop_images_u8_views(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, int n_views,
                            const void* crops, int out_w, int out_h, void* dst, void* stream);

/*
 * The mean over views: x f32 [n][n_views][d] -> out f32 [n][d],
 * out[b][j] = (((x[b][0][j] + x[b][1][j]) + ...) + x[b][n_views-1][j]) / (float)n_views, summed in view order with one
 * division at the end (no atomics: the result does not depend on scheduling).
 */
int va_view_mean(va_ctx* ctx, const void* x, int n, int n_views, int d, void* out, void* stream);

/*
 * The flow volumes of the snippets of ONE video (the 25 equally spaced flow stacks of
 * Sheet03/notes.txt:113-116,225-230): flow f32 [n_pairs][2][h][w], the video's flow fields, each computed once ->
 * stack f32 [n_snippets][n_views][2*flow_count][out_h][out_w].  Snippet s is the window of L = flow_count fields that
 * starts at field starts[s]; windows may overlap and repeat.  Output plane o = (s*n_views + v)*2L + c reads source plane
 * 2*(starts[s] + c/2) + c%2 through crops row o, with the quantisation, normalisation, flip and inversion of
 * va_flow_to_stack_views: with starts[s] = s*L the two entry points give the same bits.  starts: DEVICE int32
 * [n_snippets], clamped to [0, n_pairs - L] on the device (callers validate it on the host); crops: DEVICE int32
 * [n_snippets*n_views*2L][3].  n_pairs >= flow_count; the other limits are va_flow_to_stack_views'.
 */
int va_flow_to_stack_snippets(va_ctx* ctx, const void* flow, int n_pairs, const void* starts, int n_snippets,
                              int flow_count, int n_views, int w, int h, float bound, float mean, float stdv,
                              const void* crops, int invert_x_on_flip, int out_w, int out_h, void* stack, void* stream);

/*
 * Crop-resize gathers: scale jittering, the one input transform that resamples.  table: DEVICE i32
 * [n_out][6] rows {src, top, left, ch, cw, flip}, 1 <= ch <= h, 1 <= cw <= w, the rectangle inside the frame; the output is
 * always 224 x 224.  Output pixel (y, x), x' = flip ? 223 - x : x, plain f32 without fmaf: s = (float)cw / 224.0f,
 * u = ((float)x' + 0.5f) * s - 0.5f clamped to [0, cw - 1], x0 = floor(u), ax = u - x0, x1 = min(x0 + 1, cw - 1); rows
 * likewise from y, ch, top (no vertical flip); val = t + ay*(b - t), t = A + ax*(B - A), b = C + ax*(D - C): bilinear
 * with half-pixel centres, no antialiasing, confined to the crop.  ch = cw = 224: the plain crop, bit for bit.
 *   va_flow_to_stack_resize  flow f32 [n_pairs][2][h][w]; src indexes its 2*n_pairs planes (even: x flow); stack f32
 *                            [n_out][224][224] = va_flow_to_stack's quantisation and normalisation of val (the FLOAT field
 *                            is resampled, then quantised once); invert_x_on_flip as va_flow_to_stack_views
 *   va_resize_images_u8      src u8 [n][c][h][w] or (src_nhwc) [n][h][w][c]; src indexes images; dst u8 NCHW
 *                            [n_out][c][224][224] = (u8) rintf(clamp(val, 0, 255)) of the u8 values as floats
 * Rows are validated by the host wrappers and clamped into range on the device.  n_out (x c) <= 65535 per call.
 */
int va_flow_to_stack_resize(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, float mean, float stdv,
                            const void* table, int n_out, int invert_x_on_flip, void* stack, void* stream);
int va_resize_images_u8(va_ctx* ctx, const void* src, int n, int c, int w, int h, int src_nhwc, const void* table, int n_out,
                        void* dst, void* stream);

/*
 * Stored optical flow: the flow of a video is computed once and kept, as float32 (the TV-L1 output
 * itself) or as the 8-bit flow images TSN and the reference's flow JPEGs hold, flowq u8 [n_pairs][2][h][w].
 *   va_flow_quantize_u8         S39: flow f32 [n_pairs][2][h][w] -> out u8 of the same shape,
 *                               t = (255.0f*(v + bound)) / (2.0f*bound), q = rintf(fminf(fmaxf(t, 0), 255)): the q of
 *                               va_flow_to_stack and every flow gather, in their order (a NaN becomes 0).  Any width; flow
 *                               4-byte aligned, out any alignment (16-byte loads and 4-byte stores where the pointers allow).
 *   va_flowq_to_stack_snippets  S40: va_flow_to_stack_snippets with flowq as the source: output
 *                               ((float)q' / 255.0f - mean) / stdv, q' = 255 - q for a flipped x-flow plane under
 *                               invert_x_on_flip and q otherwise.  Plane addressing, clamping of starts and crops and limits
 *                               as there; on flowq = va_flow_quantize_u8(flow) the result equals
 *                               va_flow_to_stack_snippets(flow) bit for bit.  With starts[s] = s*L it covers the views and
 *                               crop forms as well.
 *   va_flowq_to_stack_resize    S41: the crop-resize gather in TSN's order, the IMAGE is resampled, not the float field: with
 *                               the table rows, taps and bilinear form of va_flow_to_stack_resize on the u8 values as floats,
 *                               qr = rintf(clamp(val, 0, 255)) -- what va_resize_images_u8 writes for the plane, bit for bit
 *                               -- then q' = 255 - qr under the inversion, then the normalisation.  At ch = cw = 224 it is
 *                               va_flowq_to_stack_snippets' crop bit for bit; at other sizes it differs from
 *                               va_flow_to_stack_resize of the float field (which quantises after resampling).
 * Bad arguments: VA_ERR_INVALID before anything is enqueued.  No allocation, no synchronisation, no atomics.
 */
int va_flow_quantize_u8(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, float bound, void* out, void* stream);
int va_flowq_to_stack_snippets(va_ctx* ctx, const void* flowq, int n_pairs, const void* starts, int n_snippets, int flow_count,
                               int n_views, int w, int h, float mean, float stdv, const void* crops, int invert_x_on_flip,
                               int out_w, int out_h, void* stack, void* stream);
int va_flowq_to_stack_resize(va_ctx* ctx, const void* flowq, int n_pairs, int w, int h, float mean, float stdv,
                             const void* table, int n_out, int invert_x_on_flip, void* stack, void* stream);

/*
 * The RGB-difference volume, TSN's third input modality (Sheet03/notes.txt:187-191): frames u8
 * [n_frames][3][h][w] or (src_nhwc) [n_frames][h][w][3] -> stack f32 [n_out][3*n_diff][224][224].  n_diff = D, 1 <= D,
 * 3*D <= 64.  table: DEVICE i32 [n_out][6] rows {src, top, left, ch, cw, flip} in the crop-resize gathers' format; src is
 * the FIRST frame of the item's window of D + 1 frames, src + D <= n_frames - 1 (validated by the host wrapper; the device
 * clamps src to [0, n_frames - 1 - D] and the rectangle as the crop-resize gathers do).  den: HOST float[3],
 * den[c] = 255.0f * std[c] rounded to f32 once on the host, finite and > 0.
 * For frame src + j (j = 0..D) and channel c let r_j,c(y, x) be the u8 value va_resize_images_u8 gives for that frame,
 * channel and table row (S17's val, clamped, rintf; same taps, same order, no fmaf; at ch = cw = 224 the plain crop).
 * Plane 3j + c of item o holds (float)((int)r_{j+1},c - (int)r_j,c) / den[c], one IEEE f32 division: every frame is
 * transformed identically and normalised, then neighbours are subtracted (TSN's order), so the mean cancels exactly and the
 * integer difference is exact in f32; a horizontal flip mirrors the images and changes no sign; resampling before
 * differencing makes the result equal to differences of va_resize_images_u8 outputs bit for bit.
 * n_out <= 65535 per call; n_frames > D.  Bad arguments: VA_ERR_INVALID.
 */
int va_rgbdiff_to_stack(va_ctx* ctx, const void* frames, int n_frames, int w, int h, int src_nhwc, int n_diff,
                        const float* den, const void* table, int n_out, void* stack, void* stream);

/*
 * Colour jitter and PCA lighting on u8 images, in place or not: torchvision's ColorJitter in PIL's
 * arithmetic, value for value.  src, dst u8 [n][3][h][w], any h, w >= 1 with w*h < 2^30; dst may equal src and must not
 * overlap it otherwise.  table: DEVICE f32 [n][8], one row per image = {op0, op1, op2, op3, f_brightness, f_contrast,
 * f_saturation, hue_shift}: the op codes in application order (0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue), the
 * three blend factors (>= 0) and the hue shift, an integer in 0..255.  Rows are validated by the host wrapper and clamped
 * on the device (codes to 0..4, a repeated code to none, factors to [0, 1e30], the shift to 0..255).  With
 * B(d, v, f) = d + f*(v - d) in f32 (multiply, then add), the result 0 if <= 0, 255 if >= 255, else truncated:
 *   brightness  v <- B(0, v, f) per channel
 *   saturation  v <- B(L, v, f) per channel, L = (19595 R + 38470 G + 7471 B + 32768) >> 16 of the pixel
 *   contrast    v <- B(m, v, f) per channel, m = (2 S + N) / (2 N) in integers, S the sum of L over the image as it is when
 *               contrast's turn comes (after the ops before it in the row), N = w*h
 *   hue         RGB -> HSV, h <- (h + hue_shift) & 255, HSV -> RGB, both conversions as PIL's (S32 gives the widths)
 * lighting: DEVICE f32 [n][3] or NULL; applied last, v <- (u8) rintf(clamp((float)v + lighting[i][c], 0, 255)).
 * workspace: DEVICE, n * VA_COLOR_JITTER_PARTIALS uint32, owned by the caller until the call has run: launch one writes
 * per-workgroup integer sums of L there for the images whose row has contrast, launch two adds them (integers: the result
 * does not depend on scheduling; no atomics).  NULL: the caller states that no row has contrast; launch one is skipped and
 * a contrast code counts as none.  table, lighting and workspace 4-byte aligned.  n <= 65535 per call.  Bad arguments:
 * VA_ERR_INVALID before anything is enqueued.
 */
#define VA_COLOR_JITTER_PARTIALS 256
int va_color_jitter_u8(va_ctx* ctx, const void* src, int n, int w, int h, const void* table, const void* lighting, void* dst,
                       void* workspace, void* stream);

/*
 * Decoded frames -> the pipeline's inputs: PIL's Image.resize((out_w, out_h), BILINEAR) of every RGB
 * frame and its convert('L'), bit for bit.  src u8 [n][3][h][w] (src_nhwc: [n][h][w][3]) -> rgb_out u8 [n][3][out_h][out_w],
 * always planar, and gray_out u8 [n][out_h][out_w], gray = (19595 R + 38470 G + 7471 B + 32768) >> 16 of rgb_out.  The
 * resize is PIL's 8-bit two-pass resample: the horizontal pass into a u8 intermediate, then the vertical pass, a pass whose
 * length does not change being skipped; out = clamp((2^21 + sum_j p[lo + j] k_j) >> 22, 0, 255) in int32.
 *   x_bounds, y_bounds: DEVICE i32 [out][2] = {lo, count} per output sample of the axis; x_taps, y_taps: DEVICE i32
 *   [out][ksize], ksize = 2 ceil(max(in / out, 1)) + 1, the taps k_j in units of 2^-22 (built on the host in float64:
 *   video_analytics_amd/frames.py, resample_table).  The tables of a skipped pass are NULL.  The kernels keep every read
 *   inside the input whatever a table holds.
 *   rgb_out may be NULL only when the size is unchanged and src is planar (the frames are their own result); non-NULL
 *   there, it receives a copy.  No buffer needs more than byte alignment; the tables are 4-byte aligned.
 *   workspace: DEVICE, va_frames_prepare_workspace_bytes(...) bytes, the [n][3][h][out_w] intermediate when both passes run
 *   (0 otherwise); too small: VA_ERR_WORKSPACE.
 * Any n that one launch holds (n is folded into the grid's x dimension); every plane below 2^31 / 3 pixels.  A downscale
 * factor above 16 on either axis (ksize > 33), a side below 1, a NULL required buffer: VA_ERR_INVALID before anything is
 * enqueued.  No allocation, no synchronisation; two launches at most, on the caller's stream.
 */
size_t va_frames_prepare_workspace_bytes(int n, int w, int h, int out_w, int out_h);
int va_frames_prepare(va_ctx* ctx, const void* src, int n, int w, int h, int src_nhwc, int out_w, int out_h,
                      const void* x_bounds, const void* x_taps, const void* y_bounds, const void* y_taps, void* rgb_out,
                      void* gray_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Baseline JPEG decoding: n images of one size, component count and sampling, value for value what
 * libjpeg's default decompressor gives (Huffman decode, the "islow" integer IDCT, "fancy" chroma upsampling, fixed-point
 * YCbCr -> RGB).  The host parses the headers (video_analytics_amd/jpeg.py).  ncomp 1 (gray; hs = vs = 1) or 3 (YCbCr; luma
 * sampling hs x vs of 1x1, 2x1 or 2x2, chroma 1x1); w, h in 3..65535 and the MCU-padded samples of one image, all components
 * together (64 per 8x8 block), below 2^31 -- 4:2:0 up to about 37800 x 37800; anything else is VA_ERR_INVALID (a workspace of 0 bytes).
 *   packed: DEVICE, 16-byte aligned, one upload:
 *     image table    i32 [n][4]            {table set, first segment, segments, 0}
 *     segment table  i32 [n_segments][8]   {image, byte offset into the data, bytes, first MCU, MCUs, 0, 0, 0}
 *     table sets     [n_sets][8928 bytes]  quant u16 [3][64] in natural order, one table per component; then the Huffman tables
 *                                          (DC, AC) of component 0, 1, 2, each 1424 bytes: look u16 [512] (length << 8 | symbol
 *                                          for codes of up to 9 bits, 0 otherwise), maxcode i32 [18] (per length l the
 *                                          largest l-bit value that is a code of length l or starts with a shorter code, so it
 *                                          grows with l; -1 before the first code), valoff i32 [18] (index of a length's first
 *                                          symbol minus its first code), vals u8 [256]
 *     data           the segments' entropy-coded bytes, FF 00 un-stuffed, every segment from a multiple of 4
 *   A segment is a restart interval, or a whole scan: DC prediction starts at 0 in each.
 *   out: u8 [n][3][h][w] planar RGB, or u8 [n][h][w] for gray files; any alignment.
 *   status: i32 [n], zeroed by the call; afterwards 0 for an image that decoded, else bits 1 (a code that is in no table), 2 (a
 *   run past coefficient 63), 4 (the segment's bits ran out), 8 (a bad segment-table row).  A lane never reads outside its
 *   segment nor writes outside its own blocks, whatever the bytes hold; the pixels of a failed image are unspecified.
 *   workspace: DEVICE, 16-byte aligned, va_jpeg_decode_workspace_bytes(...) bytes (0: bad shape): the coefficients i16
 *   [n][blocks][64] and, for colour files, the MCU-padded component planes; too small: VA_ERR_WORKSPACE.
 * No allocation, no synchronisation; two memsets and three launches (two for gray files) on the caller's stream.
 *   va_jpeg_idct      (testing entry point) the second launch alone: coef i16 [n][blocks][64], the blocks of an image per component
 *                     in raster order (Y, Cb, Cr), times quant u16 [ncomp][64] -> dst: the planes u8 [n][blocks * 64] (Y, Cb, Cr, each
 *                     MCU-padded), or u8 [n][h][w] for ncomp = 1.  32-bit arithmetic that wraps.
 *   va_jpeg_upsample  (testing entry point) the third launch alone: such planes -> out u8 [n][3][h][w].
 */
size_t va_jpeg_decode_workspace_bytes(int n, int w, int h, int ncomp, int hs, int vs);
int va_jpeg_decode(va_ctx* ctx, const void* packed, size_t packed_bytes, int n, int w, int h, int ncomp, int hs, int vs,
                   int n_segments, int n_sets, void* out, void* status, void* workspace, size_t workspace_bytes, void* stream);
int va_jpeg_idct(va_ctx* ctx, const void* coef, const void* quant, int n, int w, int h, int ncomp, int hs, int vs, void* dst,
                 void* stream);
int va_jpeg_upsample(va_ctx* ctx, const void* planes, int n, int w, int h, int hs, int vs, void* out, void* stream);

/*
 * Baseline JPEG encoding: n images of one size -> the entropy-coded scan of each, byte for byte what libjpeg's
 * default compressor writes between SOS and EOI (jccolor's fixed-point RGB -> YCbCr, h2v1 / h2v2 downsampling without smoothing,
 * the "islow" integer forward DCT, quantisation rounding half away from zero, Huffman coding, restart markers).  The host writes
 * the headers around it (video_analytics_amd/jpeg.py).  Shapes as va_jpeg_decode; restart: the restart interval in MCUs, 0 for
 * none, at most 65535; the bound below of one image stays below 2^31.  Anything else is VA_ERR_INVALID (a workspace of 0 bytes).
 *   images: DEVICE, u8 [n][h][w] (ncomp = 1) or planar RGB u8 [n][3][h][w]; any alignment.
 *   tables: DEVICE, 16-byte aligned, 2560 bytes, one upload: quant u16 [3][64] in natural order, one table per component; then
 *           the Huffman codes of luma and of chroma, each DC u32 [16] and AC u32 [256] indexed by symbol: length << 16 | code,
 *           0 for a symbol the table does not hold.
 *   out: DEVICE, out_bytes bytes: the scans back to back, image i from the sum of lengths[0..i).  One image takes at most
 *        2 U + 2 (intervals - 1) bytes with U = ceil(blocks * 1658 / 8) + intervals: a block codes to at most 20 bits of DC and
 *        63 x 26 bits of AC, every interval ends with up to 7 fill bits, stuffing at most doubles it, and an RSTm of two bytes
 *        stands between intervals.  With n times that nothing is ever cut short; an image that would end behind out_bytes is
 *        not written at all and gets status bit 2.
 *   lengths: i32 [n], the bytes of every scan.  status: i32 [n], zeroed by the call; bit 1: a coefficient outside the baseline
 *        categories (a DC difference above 11 bits, an AC value above 10) or a symbol without a code, which is left out of the
 *        scan (the image's bytes are then no valid file; its neighbours' are untouched); bit 2: the image did not fit.
 *   workspace: DEVICE, 16-byte aligned, va_jpeg_encode_workspace_bytes(...) bytes (0: bad shape): the un-stuffed scans and
 *        the interval marks (U rounded up to 16, each), and the coefficients i16 [n][blocks][64]; too small: VA_ERR_WORKSPACE.
 * No allocation, no synchronisation; two memsets and four launches on the caller's stream; one workgroup per image in the
 * entropy stage, none waiting for another, and bytes that depend on no launch shape or timing.
 *   va_jpeg_fdct            (testing entry point) the first launch alone: images -> coef i16 [n][blocks][64], the decoder's
 *                           layout (va_jpeg_idct); coef 16-byte aligned.  Only the quant part of tables is read.
 *   va_jpeg_entropy_encode  (testing entry point) the other three: any coef of that layout -> out, lengths, status; the
 *                           workspace as above (its front part is used).  Only the Huffman part of tables is read.
 */
size_t va_jpeg_encode_workspace_bytes(int n, int w, int h, int ncomp, int hs, int vs, int restart);
int va_jpeg_encode(va_ctx* ctx, const void* images, int n, int w, int h, int ncomp, int hs, int vs, int restart, const void* tables,
                   void* out, size_t out_bytes, void* lengths, void* status, void* workspace, size_t workspace_bytes, void* stream);
int va_jpeg_fdct(va_ctx* ctx, const void* images, const void* tables, int n, int w, int h, int ncomp, int hs, int vs, void* coef,
                 void* stream);
int va_jpeg_entropy_encode(va_ctx* ctx, const void* coef, const void* tables, int n, int w, int h, int ncomp, int hs, int vs, int restart,
                           void* out, size_t out_bytes, void* lengths, void* status, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * Mean flow subtraction, step one: flow f32 [n_pairs][2][h][w] -> means f32 [n_pairs][2], the mean of
 * every displacement field's component over the full frame.  Each value is clamped to [-32768, 32768] (a NaN becomes
 * -32768) and summed as the exact integer rint(a * 65536) in int64, so the result does not depend on the reduction
 * order: means[n][c] = (float)((double)S / ((double)(w*h) * 65536.0)).
 */
int va_flow_field_means(va_ctx* ctx, const void* flow, int n_pairs, int w, int h, void* means, void* stream);

/*
 * The motion field: flow f32 [n_chains*chain_len][2][h][w] -> out f32 of the same shape and pair order,
 * so that va_flow_to_stack / _crop / _views apply to it unchanged.  trajectory = 1: trajectory stacking, every pixel
 * (x, y) of chain b starts at p_0 = (x, y); pair n = b*chain_len + k is sampled bilinearly at p_k (clamped into the
 * frame) and p_{k+1} = p_k + that raw sample.  trajectory = 0: the flow itself.  means (DEVICE f32 [n_pairs][2], from
 * va_flow_field_means; NULL = none) is subtracted from every output value of its pair and component.  trajectory = 0
 * with means = NULL is rejected (nothing to do).  out must not overlap flow.  At most 65535 chains per call.
 */
int va_flow_motion(va_ctx* ctx, const void* flow, int n_chains, int chain_len, int trajectory, int w, int h,
                   const void* means, void* out, void* stream);

/*
 * Warped optical flow, step one: the homography that explains most of each dense flow field, the camera's
 * motion.  flow f32 [n_fields][2][h][w] -> H f64 [n_fields][3][3] (pixel coordinates, H[2][2] = 1) and stats f64
 * [n_fields][2] = {share of the frame the last solve trusted (sum of its weights / (w*h)), status}.  Reweighted least
 * squares in float64 over every pixel's correspondence (x, y) -> (x + dx, y + dy) in normalised coordinates: iters
 * solves (1..1024), the first with unit weights, the others with Tukey's biweight of the last solution's transfer error
 * at the squared scale max(cmin_sq, c0_sq * 2^-k) px^2 (0 < cmin_sq <= c0_sq).  A pixel whose flow is not finite has
 * weight 0.  A field whose 8x8 system has no Cholesky factor (a pivot not above 2^-40 x its largest diagonal entry: too
 * few pixels, all on a line, none valid) gets H = I and status 1.  The summation order is fixed: a call repeats its bits.
 */
int va_flow_homography(va_ctx* ctx, const void* flow, int n_fields, int w, int h, int iters, double c0_sq, double cmin_sq,
                       void* H, void* stats, void* stream);

/*
 * Warped optical flow, step two: out = flow minus the camera's displacement field,
 *   out[n][0](y, x) = flow[n][0](y, x) - (float)(X/D - x), out[n][1](y, x) = flow[n][1](y, x) - (float)(Y/D - y),
 *   (X, Y, D) = H[n] (x, y, 1)^T in float64, left to right, no fused multiply-add.
 * H: DEVICE f64 [n_fields][3][3].  out has the flow's shape and pair order (every va_flow_to_stack* and va_flow_motion
 * applies to it unchanged); it may be the flow buffer itself (in place) or must not overlap it.  H = I returns the flow's
 * bits.  At most 65535 fields per call.
 */
int va_flow_compensate(va_ctx* ctx, const void* flow, int n_fields, int w, int h, const void* H, void* out, void* stream);

/*
 * Warped optical flow in TSN's two-pass form, the warp: the frame pairs of TV-L1's input with every
 * second frame resampled under the pair's homography, so that a second va_tvl1_flow finds the motion that is left when
 * the camera's is gone.  frames: u8 or f32 [n_seq][frames_per_seq][h][w] (frames_per_seq >= 2), va_tvl1_flow's own input;
 * H: DEVICE f64 [N][3][3], N = n_seq * (frames_per_seq - 1), H[n] mapping the coordinates of frame k to those of frame
 * k + 1 for pair n = s * (frames_per_seq - 1) + k (va_tvl1_flow's pair order; what va_flow_homography fits);
 * pairs: f32 [N][2][h][w], va_tvl1_flow input again: N sequences of two frames.
 *   pairs[n][0] = (float) frame k.
 *   pairs[n][1](y, x): (X, Y, D) = H[n] (x, y, 1)^T in float64, left to right, no fused multiply-add; px = X/D, py = Y/D.
 *   Inside (D > 0 and 0 <= px <= w-1 and 0 <= py <= h-1; a NaN is outside): x0 = floor(px), ax = (float)(px - x0),
 *   x1 = min(x0 + 1, w-1), rows likewise, and with the four values A B / C D of frame k + 1 as floats, in float32 without
 *   fused multiply-add: t = A + ax*(B-A), b = C + ax*(D-C), value = t + ay*(b-t).  It is not rounded to 8 bits.
 *   Outside: frame k's own pixel (no evidence: no residual motion).
 * H = I gives pairs[n][1] the bits of (float) frame k + 1; a NaN H or D <= 0 everywhere gives the pair (f_k, f_k).
 * pairs must not overlap frames.  No workspace.  At most 65535 pairs per call.
 */
int va_frames_warp_pairs(va_ctx* ctx, const void* frames, int frames_are_u8, int n_seq, int frames_per_seq, int w, int h,
                         const void* H, void* pairs, void* stream);

/*
 * Self-test of the arithmetic contract: compares the kernel's packed correctly-rounded sqrt and
 * reciprocal sequences with IEEE sqrtf / division on EVERY float in [lo, hi] (within [2^-100, 1e30];
 * the reciprocal on the part >= 1).  mismatches: DEVICE u64[2] = {sqrt, reciprocal} counts.
 */
int va_selftest_exact_math(va_ctx* ctx, float lo, float hi, unsigned long long* mismatches, void* stream);

/* ------------------------------------------------------------ testing entry points --- */

/*
 * One 3x3 convolution layer (stride 1, zero padding 1) through exactly the dispatch the model uses (fp32: the forward pass's
 * and the training step's; bf16: the forward pass's), for layer-by-layer tests:
 *   out = maxpool2x2?(mask?(relu?(conv(in, w) + bias)))
 * in: NHWC [batch][hw][hw][cin_pad] of dtype; w_packed: [cout][9][cin_pad] of dtype (tap 3 ky + kx, channel innermost);
 * bias: f32 [cout]; out: NHWC [batch][hw'][hw'][cout] of dtype, or f32 when out_f32 (hw' = hw / 2 when pool, else hw);
 * mask: f32, same layout as out, or NULL (zero the output where mask <= 0: training dgrad); zeros: >= 256 zero bytes.
 * kernel_opt: fp32: VA_OPT_F32_CONV_KERNEL (0, 1); bf16: VA_OPT_BF16_VARIANT (0, 1, 2, 5, 7).
 * linear = 1: no ReLU (fp32 only).  out_f32: bf16 with pool only.  cin_pad: a multiple of 16 (fp32) / 64 (bf16);
 * cout: a multiple of 64; pool: even hw; mask: fp32 without pool.  Other shapes: VA_ERR_INVALID.
 * kernel_name: HOST buffer of name_len bytes or NULL; receives the kernel instantiation that was launched, with its
 * template arguments (e.g. "k_conv3x3_dma_f32<1,true,3>").  Pointers 16-byte aligned.
 */
int va_conv3x3_layer(va_ctx* ctx, int dtype, int kernel_opt, int hw, int cin_pad, int cout, int pool, int linear,
                     int out_f32, int batch, const void* in, const void* w_packed, const float* bias, const float* mask,
                     const void* zeros, void* out, char* kernel_name, int name_len, void* stream);

/*
 * The model's first stage alone -- the input conversion, where the path has one, then conv layer 0 -- through the very
 * function va_vgg16_forward runs first (same dispatch on the model's dtype, c_in, VA_OPT_BF16_FIRST_LAYER,
 * VA_OPT_BF16_VARIANT, VA_OPT_F32_CONV_KERNEL and the alignment of x), for tests of the layer against a reference.
 * x, x_is_u8, batch: as va_vgg16_forward's; x needs only the alignment of its element type (a bf16 model with
 * c_in <= 21 whose x is not 16-byte aligned takes the staged path, as in va_vgg16_forward).
 * out: NHWC [batch][224][224][64] of the model's dtype (f32 / bf16): relu(conv(x, w0) + b0), stored by the convolution
 * kernel itself.  staged: the converted input of the staging paths, written by the conversion kernel: fp32 models f32
 * [batch][224*224][c_in_pad] (c_in rounded up to 16; channels >= c_in zero); bf16 models bf16 [batch][224*224][64]:
 * c_in >= 22: the channels, zero from c_in on; c_in <= 21: channel kx*c_in + c = channel c of pixel x + kx - 1 (zero
 * outside the row), zero from 3*c_in on.  The fused bf16 first layer (k_conv1_fused_bf16) does not touch it.
 * info: HOST buffer of info_len bytes or NULL; receives what ran, e.g. "k_conv1_fused_bf16<u8>",
 * "k_nchw_to_nhwc_xcol<float>+k_conv3x3_mfma_bf16<1,false,false,3>", "k_nchw_to_nhwc_pad<u8,float>+k_conv3x3_mfma<2,2,2,1,false,16>".
 * VA_ERR_INVALID before anything is launched: NULL model/x/staged/out, batch < 1 (or beyond va_vgg16_forward's limits: 4096;
 * bf16 models 334), u8 input to a model created without in_mean/in_std, staged or out not 16-byte aligned.
 * Non-finite inputs: k_conv1_fused_bf16 turns a NaN or infinity in pixel (y, x) of one channel into NaN outputs at the
 * 3 x 3 pixels around it (its ReLU keeps a NaN).  It multiplies the tail of its 16-element K blocks -- the first
 * KROW - 3 Cp channels of the pixel after the three taps -- with zero weights, so the NaN also reaches column x - 2 of rows
 * y - 1 .. y + 1 and, when x % 16 == 15, column x + 16 of rows y - 2 .. y (the patch row of the brick to the right
 * wraps); every other output keeps its bits, and finite inputs are not affected.  Every other conv kernel, the staged
 * paths included, keeps a NaN through ReLU and the 2 x 2 max as well (IEEE maximum) and confines it to the 3 x 3 pixels.
 */
int va_vgg16_first_layer(va_vgg16* model, const void* x, int x_is_u8, int batch,
                         void* staged, void* out, char* info, int info_len, void* stream);

/*
 * The kernels of the training step (va_vgg16_train_step), one layer at a time, through the very functions the step
 * calls, for kernel-by-kernel tests.  fp32 throughout; every pointer 16-byte aligned; shapes the kernels do not take are
 * VA_ERR_INVALID before anything is launched.  `info`: HOST buffer of info_len bytes or NULL; receives what ran.
 *
 * va_train_conv_backward_layer: backward of one 3x3 conv layer.  dy: NHWC [batch][hw][hw][cout], the gradient at the
 * layer's post-ReLU, pre-pool output (ReLU mask applied); x: the layer's input, NHWC [batch][hw][hw][cin_pad] (channels
 * >= cin zero); w_packed / mom_w: [cout][9][cin_pad]; bias / mom_b: [cout]; cin: the real input channels.
 *   dx != NULL: dx = mask?(conv(dy, flip-transpose(w_packed))), NHWC [batch][hw][hw][cin], from the weights BEFORE the
 *     update (k_pack_dgrad_w into wt, then the forward dispatch, kernel_opt = VA_OPT_F32_CONV_KERNEL); mask: f32 shaped
 *     like dx or NULL (dx is zeroed where mask <= 0).  Needs cin == cin_pad, cin % 64 == 0.
 *   then, in place: g_w = sum over pixels of dy x (k_conv_wgrad into slab, k_wgrad_reduce_sgd), g_b = sum of dy
 *     (k_conv_bgrad_partial into bpart, k_conv_bgrad_sgd); V = momentum V + g; W -= lr V.
 * cin_pad and cout: multiples of 4 (16-byte loads); with dx: cout a multiple of 16, cin of 64; batch 1..64; 1 <= cin <= cin_pad.
 * Scratch: slab, wt (may be NULL when dx is), bpart; scratch_floats: HOST array of 3 = {slab, wt, bpart} in floats: on
 * entry the sizes given, on return the sizes needed (wt = cin 9 cout; bpart = blocks cout; slab = S Mpad Npad of the
 * reported plan).  slab == NULL: size query, nothing is launched.  Too small: VA_ERR_WORKSPACE.
 * info: "k_conv_wgrad<1,3> S=2 chunk=304 Mpad=64 Npad=192 bgrad_blocks=588 dgrad=k_conv3x3_dma_f32<1,false,3>"
 * (dgrad=none without dx).  zeros: >= max(512, cin) zero floats.
 */
int va_train_conv_backward_layer(va_ctx* ctx, int kernel_opt, int batch, int hw, int cin, int cin_pad, int cout,
                                 const float* dy, const float* x, float* w_packed, float* bias, float* mom_w, float* mom_b,
                                 float lr, float momentum, float* dx, const float* mask, const float* zeros, float* slab,
                                 float* wt, float* bpart, size_t* scratch_floats, char* info, int info_len, void* stream);
/*
 * Backward of one Linear layer (fc_backward_dispatch): dz f32 [batch][out_f], x f32 [batch][in_f] (the layer's input),
 * w / mom_w [out_f][in_f], bias / mom_b [out_f].  dx [batch][in_f] = dz W (weights before the update), times `scale`
 * where mask > 0 and 0 elsewhere (mask f32 [batch][in_f] or NULL: no mask, no scale); then in place
 * V = momentum V + dz^T x, W -= lr V, and the same for the bias.  batch 1..64, out_f, in_f >= 1.
 * info: "k_fc_dx<32>" (batch <= 32) or "k_fc_dx<64>": the instantiation of all three classifier kernels.
 */
int va_train_fc_backward_layer(va_ctx* ctx, int batch, int out_f, int in_f, const float* dz, const float* x, float* w,
                               float* bias, float* mom_w, float* mom_b, float lr, float momentum, float* dx,
                               const float* mask, float scale, char* info, int info_len, void* stream);
/*
 * The STORE and ADD forms of the two entry points above: the same launches with the finishing kernels in
 * the form va_vgg16_train_accumulate uses.  grad_w ([cout][9][cin_pad] / [out_f][in_f]) and grad_b receive the gradient
 * (add = 0: G = g) or have it added (add != 0: G = G + g, one rounding); the weights are only read (dx), no bias, momentum
 * buffer, lr or momentum takes part.  Everything else, scratch and info included, as above.
 */
int va_train_conv_backward_layer_grad(va_ctx* ctx, int kernel_opt, int batch, int hw, int cin, int cin_pad, int cout,
                                      const float* dy, const float* x, const float* w_packed, int add, float* grad_w,
                                      float* grad_b, float* dx, const float* mask, const float* zeros, float* slab,
                                      float* wt, float* bpart, size_t* scratch_floats, char* info, int info_len,
                                      void* stream);
int va_train_fc_backward_layer_grad(va_ctx* ctx, int batch, int out_f, int in_f, const float* dz, const float* x,
                                    const float* w, int add, float* grad_w, float* grad_b, float* dx, const float* mask,
                                    float scale, char* info, int info_len, void* stream);
/*
 * 2x2/2 max-pool of y NHWC [batch][hw][hw][c] into p [batch][hw/2][hw/2][c] (k_maxpool) and, when dp != NULL, its
 * backward fused with the ReLU mask of the pooled value (k_unpool): dy gets dp at the FIRST maximum of each window in
 * row-major order where p > 0, and 0 everywhere else.  hw even, c a multiple of 4.
 */
int va_train_pool_layer(va_ctx* ctx, int batch, int hw, int c, const float* y, float* p, const float* dp, float* dy,
                        void* stream);
/*
 * Loss of the step: k = 0: mean cross-entropy of logits [n][c] (k_ce_fwd_bwd); k >= 1: of the mean over the k snippets
 * of logits [n][k][c] (k_ce_consensus_fwd_bwd).  labels i64 [n]; dlogits like logits; out f32 [2] = loss, hits.
 * n >= 1, n * max(k, 1) <= 64, c >= 1.
 */
int va_train_loss(va_ctx* ctx, const float* logits, const void* labels, int n, int k, int c, float* dlogits, float* out,
                  void* stream);
/*
 * The multi-task form of the step's loss (k_ce_multitask_fwd_bwd), through the function
 * va_vgg16_train_step_multitask calls: logits [n][c] (k = 0) or [n][k][c] with c = the sum of head_sizes; labels i64 [n],
 * LOCAL to the video's head; tasks i32 [n]; head_sizes: HOST int[n_heads]; dlogits like logits; out f32 [2 + 2 n_heads] =
 * loss, hits, loss per head, hits per head.  n >= 1, n * max(k, 1) <= 64, 1 <= n_heads <= 8, every head >= 1 class, c <= 2^20;
 * anything else is VA_ERR_INVALID before a launch.
 */
int va_train_loss_multitask(va_ctx* ctx, const float* logits, const void* labels, const void* tasks, int n, int k,
                            int n_heads, const int* head_sizes, float* dlogits, float* out, void* stream);
/* Dropout(p = 0.5) of the step's classifier layer `layer` (0..2) in place on x f32 [n] (k_dropout, keys from
 * (dropout_seed, layer) as va_vgg16_train_step derives them). */
int va_train_dropout(va_ctx* ctx, float* x, size_t n, unsigned long long dropout_seed, int layer, void* stream);

/*
 * The stages of va_linear_svm_fit (below) one at a time, for stage-by-stage tests: the fit's own
 * loop is written over the same helpers, so a phase enqueues exactly the launches the fit enqueues for it.
 *
 * va_linear_svm_fit_layout (host only): offsets: HOST size_t[VA_SVM_FIT_FIELDS], the byte offsets into the workspace of
 *   W G S R P HP          f64 [rows][dim + 1]   iterate, gradient, Newton direction, CG residual, CG direction, H P
 *   M U Q                 f64 [n][rows]         margins Xh W, the active part of the last product's input, Xh S
 *   part                  f64 [ceil(n / 256)][rows][dim + 1]   Xh^T U per 256-row chunk
 *   losspart              f64 [ceil(n / 64)][rows]             squared hinge per 64-row block
 *   f gn g0 steps rr cgtol cgs   f64 [rows]     objective, |G|, |G(0)|, Newton steps, the CG's |R|^2 and stop threshold, CG steps
 *   live notdone          i32 [rows]            the row's CG is running; the row has not met the stop rule
 * in this order, each on a 256-byte boundary.  Returns the total, equal to va_linear_svm_fit_workspace_bytes; sizes out of
 * range, offsets == NULL or count != VA_SVM_FIT_FIELDS answer 0 and set va_last_error.
 *
 * va_linear_svm_fit_phase: x, y, n, dim, n_classes, C, intercept_scaling, tol, workspace, workspace_bytes, stream and their
 * checks as va_linear_svm_fit's.  It reads and writes the solver state in the workspace and nothing else:
 *   VA_SVM_PHASE_INIT         k_svm_init: the six vectors and seven scalars 0, live 0, notdone 1
 *   VA_SVM_PHASE_EVAL_FIRST   k_svm_fwd<EVAL>, k_svm_xtu, k_svm_cls_grad(first = 1): M, U, f, G, the stop rule with g0 = gn,
 *                             and the start of the CG (S = 0, R = P = -G, rr, cgtol, live)
 *   VA_SVM_PHASE_EVAL         the same with first = 0: g0 is kept
 *   VA_SVM_PHASE_CG           `count` (1 .. 100) rounds of k_svm_fwd<CG>, k_svm_xtu, k_svm_cls_cg
 *   VA_SVM_PHASE_LINE_SEARCH  k_svm_fwd<LS>, k_svm_cls_ls
 * `count` is read by the CG phase only.  An unknown phase or a CG count outside 1 .. 100: VA_ERR_INVALID before any launch.
 * One Newton step of the fit is CG with count 100, LINE_SEARCH, EVAL; restart = 1 is INIT, EVAL_FIRST.
 */
#define VA_SVM_FIT_FIELDS 20
#define VA_SVM_PHASE_INIT 0
#define VA_SVM_PHASE_EVAL_FIRST 1
#define VA_SVM_PHASE_EVAL 2
#define VA_SVM_PHASE_CG 3
#define VA_SVM_PHASE_LINE_SEARCH 4
size_t va_linear_svm_fit_layout(int n, int dim, int n_class_rows, size_t* offsets, int count);
int va_linear_svm_fit_phase(va_ctx* ctx, const void* x, const void* y, int n, int dim, int n_classes, double C,
                            double intercept_scaling, double tol, int phase, int count, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * Measurement hooks (bench.py): when enabled, va_tvl1_flow brackets every run of
 * inner-iteration launches with HIP events on `stream`.  va_tvl1_profile_read synchronises
 * those events and returns, summed over all va_tvl1_flow calls since the last reset:
 * out[0] = milliseconds inside the inner-iteration kernel, out[1] = its launches,
 * out[2] = pixel-iterations it performed (valid pixels x iterations; algorithmic bytes =
 * 64 B x out[2]), out[3] = pixel-warps (44 B each), out[4] = milliseconds during which at least one
 * run of inner-iteration launches was in flight (the union of the bracketed intervals: equals
 * out[0] on one stream, smaller when calls on several streams overlap) -- all as doubles (HOST
 * array of 5).  va_tvl1_profile_enable(1) synchronises the device and sets the time origin.
 */
int va_tvl1_profile_enable(va_ctx* ctx, int on);
int va_tvl1_profile_read(va_ctx* ctx, double* out, int reset);
/* The same measurement per pyramid level (0 = full resolution): out[3*s + 0] = summed per-call milliseconds of the
 * level's inner-iteration launches, out[3*s + 1] = its pixel-iterations, out[3*s + 2] = its launches (HOST array of
 * 3*n doubles, n <= 16).  Call va_tvl1_profile_read(reset = 0) first (it synchronises the events), then this. */
int va_tvl1_profile_levels(va_ctx* ctx, double* out, int n, int reset);

/* ------------------------------------------------ video-level aggregation and fusion --- */

/*
 * The AverageMeter bank of validate() (Sheet03/utils.py:154-171, Sheet03/spatialModel.py:223-228) kept
 * on the device: desc f32 [batch][dim] (the descriptors of one batch), slot i32 [batch] = index of each
 * clip's video in the caller's video list (a negative slot skips the row: padding);
 * sums f32 [n_slots][dim] += desc row, counts i32 [n_slots] += 1, rows applied in batch order (a video
 * occurring twice in a batch gets both adds in that order: bit-identical to update() row by row).
 * Replaces the per-batch device-to-host copy of the reference loop.
 */
int va_meter_update(va_ctx* ctx, const void* desc, const void* slot, int batch, int dim,
                    void* sums, void* counts, int n_slots, void* stream);
/* avg f32 [n_slots][dim] = sums / counts (AverageMeter.avg; 0 where counts == 0). */
int va_meter_average(va_ctx* ctx, const void* sums, const void* counts, int n_slots, int dim,
                     void* avg, void* stream);

/*
 * LinearSVC.predict of the fusion step (Sheet03/combinedModel.py:38): x f64 [n][dim] (the joined
 * descriptors of combineDescriptors, Sheet03/combinedModel.py:9-26), coef f64 [n_class_rows][dim],
 * intercept f64 [n_class_rows] (sklearn's coef_ / intercept_; n_class_rows == 1 for a binary problem)
 * -> scores f64 [n][n_class_rows] = x coef^T + intercept (sum over dim in ascending order, double
 * multiply then add), pred i32 [n] = index into classes_: arg-max (first maximum), or score > 0 for
 * the binary case.  The model is a fitted LinearSVC's or va_linear_svm_fit's; with x the test rows of a Gram matrix and coef
 * va_kernel_svm_fit's dual_coef it is the kernel SVM's prediction.  1 <= dim <= 65536 (up to 8192 the row of x is staged in
 * LDS, above that it is read in place: the same operations in the same order).
 */
int va_linear_svm_predict(va_ctx* ctx, const void* x, int n, int dim, const void* coef,
                          const void* intercept, int n_class_rows, void* scores, void* pred,
                          void* stream);

/*
 * LinearSVC().fit of the fusion step (Sheet03/combinedModel.py:34-35): liblinear's L2R_L2LOSS_SVC,
 * one-vs-rest.  Class row r minimises f_r(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i w.[x_i, s])^2 over w in R^(dim+1), with
 * y_i = +1 where y[i] is the row's class and -1 elsewhere and s = intercept_scaling (the bias is regularised, as in
 * liblinear; s = 0: no intercept); coef[r] = w[0..dim), intercept[r] = s w[dim].  rows = n_classes == 2 ? 1 : n_classes,
 * the single row of a binary problem being class 1's (sklearn's convention, which va_linear_svm_predict reads).
 *
 * x f64 [n][dim], y i32 [n] with values in [0, n_classes).  The solver is a primal Newton-CG in float64 over all rows at
 * once; a row stops, and is frozen, when |grad f_r(w)| <= tol |grad f_r(0)|.  The call enqueues newton_iters Newton steps
 * on the caller's stream and then writes coef f64 [rows][dim], intercept f64 [rows] and stats f64 [rows][4] = f_r,
 * |grad f_r|, |grad f_r(0)|, Newton steps taken so far; it allocates nothing and does not synchronise.  restart = 1 starts
 * from w = 0; restart = 0 continues from the state a previous call left in the workspace (same x, y, sizes and scalars), so
 * that a caller may enqueue a few steps, read stats, and go on until every row has stopped: the steps of one long call and
 * of several short ones are the same operations and give the same bits.  No atomics: two fits of the same input agree
 * bit for bit.  workspace: va_linear_svm_fit_workspace_bytes(n, dim, rows) bytes, 8-byte aligned (too small:
 * VA_ERR_WORKSPACE).  n >= 2, 1 <= dim <= 8192, 2 <= n_classes <= 4096, C > 0, tol > 0, intercept_scaling >= 0, all
 * finite, 0 <= newton_iters <= 1000, else VA_ERR_INVALID before anything is launched.  The size query answers 0 and sets
 * va_last_error for sizes out of range (n_class_rows is 1 or 3 .. 4096).
 */
size_t va_linear_svm_fit_workspace_bytes(int n, int dim, int n_class_rows);
int va_linear_svm_fit(va_ctx* ctx, const void* x, const void* y, int n, int dim, int n_classes, double C,
                      double intercept_scaling, double tol, int newton_iters, int restart, void* coef, void* intercept,
                      void* stats, void* workspace, size_t workspace_bytes, void* stream);
/* cg_steps f64 [n_class_rows]: the CG steps every row has taken since restart = 1, read from the workspace of a fit of the
 * same sizes (a measurement for tools/bench_svm_fit.py and the info of linear_svm_fit; asynchronous, on the stream). */
int va_linear_svm_fit_cg_steps(va_ctx* ctx, int n, int dim, int n_class_rows, const void* workspace,
                               size_t workspace_bytes, void* cg_steps, void* stream);

/*
 * The consensus over the k items (snippets x views, snippet-major) of each of n videos:
 * logits f32 [n][k][c] -> scores f32 [n][c], one launch for all videos.
 *   mode 0 ("softmax"; Simonyan and Zisserman's testing, Sheet03/notes.txt:113-116): per item
 *          p_j = exp(x_j - max_j x) / sum_j exp(x_j - max_j x) in f32, then ((p_0 + p_1) + ...) + p_{k-1} in item order
 *          and one division by (float)k, as va_view_mean.
 *   mode 1 ("logits"; TSN's H(G(...)), notes.txt:176-185): the mean of the logits in item order, then one softmax.
 * No atomics: the result does not depend on scheduling.  A NaN logit makes the scores of its video NaN.
 * k <= 4096, c <= 4096.
 */
int va_score_consensus(va_ctx* ctx, const void* logits, int n, int k, int c, int mode, void* scores, void* stream);

/*
 * Fusion of the two streams' scores by weighted averaging (Sheet03/notes.txt:121-124; TSN's weighting,
 * notes.txt:225-230): a, b f32 [n][c] -> fused f32 [n][c] = (wa*a + wb*b) / (wa + wb), every operation rounded to f32,
 * and pred i32 [n], the arg-max of fused with the first maximum winning (as va_validate_batch and
 * va_linear_svm_predict).  wa = wb = 1 is plain averaging, (1, 1.5) TSN's spatial : temporal weighting.
 * wa, wb >= 0 and wa + wb > 0, else VA_ERR_INVALID.  (Fusion by a linear SVM on the stacked scores [n][2c] or on the
 * joined descriptors [n][512] is va_linear_svm_predict.)
 */
int va_fuse_scores(va_ctx* ctx, const void* a, const void* b, int n, int c, float wa, float wb, void* fused, void* pred,
                   void* stream);

/*
 * Fusion of m streams' scores by weighted averaging: scores: HOST array of m DEVICE pointers to f32 [n][c];
 * weights: HOST float[m]; 2 <= m <= 8.  fused f32 [n][c] = (((w0*a0 + w1*a1) + w2*a2) + ...) / (((w0 + w1) + w2) + ...),
 * every operation rounded to f32, in stream order; pred i32 [n], the arg-max of fused with the first maximum winning.  Every
 * weight finite and >= 0 with a positive (finite) sum, else VA_ERR_INVALID.  m = 2 gives va_fuse_scores' bits.
 */
int va_fuse_scores_n(va_ctx* ctx, const void* const* scores, const float* weights, int m, int n, int c, void* fused,
                     void* pred, void* stream);

/* ------------------------------------------------------------------ training step --- */

/*
 * The body of the batch loop of SpatialNetwork.train() / TemporalNetwork.train()
 * (Sheet03/spatialModel.py:165-182, Sheet03/temporalModel.py:194-211), fp32 models only:
 * forward in train mode (Dropout(p=0.5) after the three hidden classifier ReLUs; element i of dropout
 * layer d is kept and doubled iff video_analytics_amd.synth.hash_uniform(dropout_seed, 100 + d)[i] >= 0.5),
 * mean cross-entropy (nn.CrossEntropyLoss, Sheet03/spatialModel.py:114), backward through the whole network
 * (max-pool gradient to the first maximum of each window, like torch), then torch.optim.SGD's update of every
 * parameter (Sheet03/spatialModel.py:116: buf = momentum*buf + grad; p -= lr*buf; no weight decay).  Weight decay, another
 * dropout ratio and frozen layers: va_vgg16_set_solver below; this paragraph describes its defaults.
 *   va_vgg16_train_init   allocates and zeroes the momentum buffers (the only allocation of the training path)
 *   x, labels (i64 [batch]): device; batch <= 64
 *   desc: device f32 [batch][desc_dim] or NULL: the train-mode descriptor tap (after the third Dropout:
 *         Sheet03/spatialModel.py:171-173, quirk 7 of SURVEY.md)
 *   loss_out: device f32[2] = { mean cross-entropy, number of arg-max hits }, both of the forward pass
 *             that preceded the update
 */
int va_vgg16_train_init(va_vgg16* model, void* stream);
size_t va_vgg16_train_workspace_bytes(const va_vgg16* model, int batch);
int va_vgg16_train_step(va_vgg16* model, const void* x, int x_is_u8, const void* labels, int batch,
                        float lr, float momentum, unsigned long long dropout_seed, void* desc,
                        void* loss_out, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same step with the loss on the consensus of each video's snippets (TSN, Sheet03/notes.txt:165-185):
 * x holds n*k images, video-major (n*k <= 64), labels i64 [n].  With logits z[n][k][c]: m[v][c] = (z[v][0][c] + ... +
 * z[v][k-1][c]) / (float)k, summed in snippet order; loss (mean over the n videos), hits (arg-max of m) and the gradient
 * g at m are va_vgg16_train_step's on m; every snippet receives g / (float)k.  Forward, backward and update are the same
 * code; k = 1 gives va_vgg16_train_step's bits.  desc: [n*k][desc_dim]; workspace: va_vgg16_train_workspace_bytes(n*k).
 */
int va_vgg16_train_step_consensus(va_vgg16* model, const void* x, int x_is_u8, const void* labels, int n, int k,
                                  float lr, float momentum, unsigned long long dropout_seed, void* desc,
                                  void* loss_out, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The same step with one loss per dataset (multi-task learning, Sheet03/notes.txt:88-96): the model's last
 * layer holds n_heads heads, head t the outputs [o_t, o_t + head_sizes[t]) with o_t = head_sizes[0] + ... + head_sizes[t-1];
 * the sum of head_sizes (HOST int[n_heads], 1 <= n_heads <= 8, each >= 1) must be the model's n_classes.  tasks i32 [n]
 * (device) names each video's head, labels i64 [n] are local to it.  Each head's loss is va_vgg16_train_step_consensus's
 * on the head's videos and outputs (its mean over that head's videos); the step descends the sum of the heads' losses; the
 * outputs of the other heads receive a zero gradient, so a head without a video in the batch moves by its momentum alone, as
 * the rows of one torch parameter do under torch.optim.SGD.  loss_out: device f32 [2 + 2 n_heads] = { loss, hits, loss of
 * every head, hits of every head }.  k >= 1, n*k <= 64; n_heads = 1 gives va_vgg16_train_step_consensus's bits.
 * workspace: va_vgg16_train_workspace_bytes(n*k).  A task outside [0, n_heads) or a label outside its head: NaN loss.
 */
int va_vgg16_train_step_multitask(va_vgg16* model, const void* x, int x_is_u8, const void* labels, const void* tasks,
                                  int n, int k, int n_heads, const int* head_sizes, float lr, float momentum,
                                  unsigned long long dropout_seed, void* desc, void* loss_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
/*
 * The step split into "produce the gradient" and "apply it" (DESIGN.md S29, S30): gradient accumulation over micro-batches,
 * torch.nn.utils.clip_grad_norm_ on the whole gradient, and a gradient to all-reduce for data-parallel training.
 *
 * The gradient buffer is the caller's: one flat device f32 buffer of va_vgg16_train_grad_floats(model) floats (about 135 M,
 * 540 MB), 16-byte aligned, holding the 34 parameter tensors in the order conv 0..12 as (weight, bias), then fc 0..3 as
 * (weight, bias), each in the layout of its parameter and momentum buffer (conv weights packed [cout][9][cin_pad], FC1 in
 * NHWC-flatten order).  va_vgg16_train_grad_layout: offsets / counts (HOST size_t[34], in floats) of the segments; every
 * segment starts on a multiple of 64 floats, and the storing call writes zeros into the gaps, which no norm ever reads.
 *
 * va_vgg16_train_accumulate: forward and backward of one micro-batch; weights and momentum buffers are left untouched.
 *   k = 0: va_vgg16_train_step's loss on n images; k >= 1, tasks == NULL (n_heads = 0, head_sizes ignored):
 *   va_vgg16_train_step_consensus's on n videos of k snippets; tasks != NULL: va_vgg16_train_step_multitask's.  Batch limits
 *   (n * max(k, 1) <= 64), workspace (va_vgg16_train_workspace_bytes), the dropout hash, desc and loss_out as there.
 *   scales: HOST f32 [max(n_heads, 1)], finite: after the loss launch the gradient at the logits is multiplied by its head's
 *   scale on that head's columns (one launch; none when every scale is exactly 1).  A ragged micro-batch gets its share of
 *   the full batch's mean with scale = n_micro / n_full (per head: that head's videos).  loss_out is NOT scaled.
 *   first != 0: G = g (and zeros into the gaps); first = 0: G = G + g, one rounding per element.
 *   Forward, data gradients, the weight-gradient slabs and every sum are the fused step's code: g has the bits of the
 *   gradient the fused step would have applied.
 * va_vgg16_train_apply: V = fmaf(momentum, V, c G), W = fmaf(-lr, V, W) over all 34 tensors in one launch, the fused step's
 *   two fused multiply-adds.  clip_norm <= 0: c is absent (G is used as it is).  clip_norm > 0: the norm of G first, a float64
 *   sum of squares in a fixed order (1024 partial sums in the workspace, one workgroup adds them; no atomics), then
 *   c = min(1, clip_norm / (norm + 1e-6)), torch's rule, read by the update on the device: the host never waits.
 *   norm_out: device f64 [1] or NULL (non-NULL with clip_norm <= 0: the norm is computed and reported, not used).
 *   workspace: va_vgg16_train_apply_workspace_bytes() bytes, 8-byte aligned, needed when the norm is (the training workspace
 *   serves); too small: VA_ERR_WORKSPACE.
 * va_vgg16_unpack_grad: the gradient in the reference's layouts (as va_vgg16_export_state): what p.grad holds.
 * Argument errors are VA_ERR_INVALID / VA_ERR_WORKSPACE before anything is written.
 */
size_t va_vgg16_train_grad_floats(const va_vgg16* model);
int va_vgg16_train_grad_layout(const va_vgg16* model, size_t* offsets, size_t* counts);
int va_vgg16_train_accumulate(va_vgg16* model, const void* x, int x_is_u8, const void* labels, const void* tasks, int n,
                              int k, int n_heads, const int* head_sizes, const float* scales, int first,
                              unsigned long long dropout_seed, void* desc, void* loss_out, void* grad, size_t grad_floats,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t va_vgg16_train_apply_workspace_bytes(void);
int va_vgg16_train_apply(va_vgg16* model, const void* grad, size_t grad_floats, float lr, float momentum, float clip_norm,
                         void* norm_out, void* workspace, size_t workspace_bytes, void* stream);
int va_vgg16_unpack_grad(va_vgg16* model, const void* grad, void* const* conv_w, void* const* conv_b, void* const* fc_w,
                         void* const* fc_b, void* stream);
/*
 * The solver: L2 weight decay, the ratio of the three Dropout layers and frozen layers, "as [15]" in both
 * papers (Sheet03/notes.txt:98-111, :196-210, :234-243).  The model carries ONE solver state; va_vgg16_train_step, _consensus,
 * _multitask, _accumulate and va_vgg16_train_apply read it.  A model whose solver was never set behaves bit for bit as one
 * with va_solver_default's values: V = mu V + g; W -= lr V, Dropout(0.5), nothing frozen.
 *
 * Update of one tensor.  lr_t = lr, wd_t = weight_decay for a weight; lr_t = (float)(lr * bias_lr_mult),
 * wd_t = (float)(weight_decay * bias_decay_mult) for a bias, both formed once on the host (a multiplier of 1 keeps the bits).
 * With g the completed gradient element (c g under clipping, as va_vgg16_train_apply forms it):
 *   wd_t == 0:  V = fmaf(mu, V, g);  W = fmaf(-lr_t, V, W)                       (today's two statements, a path of its own)
 *   otherwise:  d = fmaf(wd_t, W, g);  V = fmaf(mu, V, d);  W = fmaf(-lr_t, V, W)
 * torch.optim.SGD's order: clip the raw gradient, add the decay, then the momentum; the clip norm is the raw gradient's and
 * the decay never enters it.  (Caffe folds lr into the momentum buffer, V = mu V + lr d; W -= V: this library keeps torch's
 * form, the two differ when lr changes between steps.)  One stored micro-batch plus va_vgg16_train_apply is the fused step
 * bit for bit under any solver.  The padded input channels of the packed weights are zero and stay zero.
 *
 * Dropout with ratio p (float32): element i of layer d is kept iff synth.hash_uniform(dropout_seed, 100 + d)[i] >= p, i.e.
 * iff (h >> 8) >= T with T = ceil(p * 2^24), and multiplied by s = 1.0f / (1.0f - p); a dropped one by 0.  p = 0.5: T = 2^23,
 * s = 2, today's bits; p = 0 launches nothing.  The classifier backward multiplies by each layer's own s.
 *
 * frozen_layers = n: layers are numbered 0..12 (conv) and 13..16 (fc); the first n keep every bit of weight, bias and both
 * momentum buffers (no gradient, no decay, no momentum move: requires_grad = False under torch.optim.SGD).  The backward pass
 * stops above layer n-1 and layer n forms no input gradient; n >= 13 launches no un-pool and no conv backward.  Loss, hits,
 * descriptors and every other tensor keep the bits of the unfrozen step.  va_vgg16_train_accumulate with first != 0 writes
 * zeros into the frozen tensors' segments of the gradient buffer and leaves them alone otherwise; va_vgg16_train_apply and
 * its norm skip them.  n may change between steps.  A VA_OPT_TRAIN_STOP_AT layer that is frozen is never reached.
 *
 * va_vgg16_set_solver returns VA_ERR_INVALID, names the field in va_last_error() and
 * changes nothing for a negative or non-finite weight_decay or multiplier, a dropout ratio outside [0, 1) or NaN,
 * frozen_layers outside 0..16, or a bf16 model.
 * va_train_dropout_p: va_train_dropout (testing entry points) with the ratio p of [0, 1).
 */
typedef struct va_solver {
    float weight_decay;     /* L2 coefficient of the weights, torch.optim.SGD's weight_decay; default 0 */
    float bias_lr_mult;     /* bias lr = lr * this; default 1 (Caffe's VGG and TSN solvers: 2) */
    float bias_decay_mult;  /* bias decay = weight_decay * this; default 1 (torch); Caffe's: 0 */
    float dropout[3];       /* ratio of the classifier's three Dropout layers; default 0.5 each */
    int   frozen_layers;    /* 0..16: the first n of conv 0..12, fc 0..3 take no gradient and no update */
} va_solver;
void va_solver_default(va_solver* solver);
int va_vgg16_set_solver(va_vgg16* model, const va_solver* solver);
int va_vgg16_get_solver(const va_vgg16* model, va_solver* solver);
int va_train_dropout_p(va_ctx* ctx, float* x, size_t n, unsigned long long dropout_seed, int layer, float p, void* stream);
/*
 * Checkpoints (Sheet03/spatialModel.py:234-260, Sheet03/utils.py:29-35): copy the parameters (which = 0) or the
 * momentum buffers (which = 1) out to / in from device tensors in the reference's layouts -- conv OIHW
 * [cout][cin][3][3], fc [out][in] (FC1's input CHW-major), biases [out] -- i.e. what model.state_dict() and
 * optimizer.state_dict()['state'][..]['momentum_buffer'] hold.
 */
/* Debugging aid of the tests: byte offsets inside the training workspace -- out[0..12] the 13 conv outputs,
 * out[13..25] the pooled maps (0 where a layer has no pool), out[26], out[27] the two gradient buffers,
 * out[28] the gradient at the classifier input, out[29] the NHWC input (HOST array of 30).  With the
 * va_vgg16_set_option(model, VA_OPT_TRAIN_STOP_AT, i), va_vgg16_train_step stops after the backward pass of conv
 * layer i (return code VA_ERR_STOPPED), leaving the gradient buffers as that layer left them. */
int va_vgg16_train_plan(const va_vgg16* model, int batch, unsigned long long* out);
int va_vgg16_export_state(va_vgg16* model, int which, void* const* conv_w, void* const* conv_b,
                          void* const* fc_w, void* const* fc_b, void* stream);
int va_vgg16_import_state(va_vgg16* model, int which, const void* const* conv_w, const void* const* conv_b,
                          const void* const* fc_w, const void* const* fc_b, void* stream);

/*
 * Fisher vectors (csrc/fisher.hip): the part of the modelled project's Sheet02 between the trajectory
 * descriptors and the linear SVM (Sheet02.py:568-617) -- PCA to 64 dimensions (Sheet02.py:40), a 256-component
 * diagonal-covariance Gaussian mixture (Sheet02.py:41), one Fisher vector of length k + 2 k d per video.  All arithmetic is
 * float64 (the descriptors are float32 and widened exactly); every sum has a fixed order that depends on the inputs and the
 * parameters alone; there are no floating-point atomics.  The dense products run on v_mfma_f64_16x16x4_f64.
 *
 * va_pca_moments: x DEVICE float32 [n][d], 1 <= n, 1 <= d <= 2048.  sums: DEVICE float64 [1 + d + d*d]: the row count, the
 * column sums, and X^T X as [d][d] of which the upper triangle (column >= row) is filled and the rest is 0.  first = 1
 * stores, first = 0 adds to what sums holds: one call per video accumulates a training set that never sits in one tensor.
 * Rows are summed in chunks of va_pca_chunk_rows(n, d) rows, then the chunks in ascending order.  workspace:
 * va_pca_workspace_bytes(n, d) bytes (0 and va_last_error() for sizes out of range; never above 1 GiB), 8-byte aligned.
 */
size_t va_pca_workspace_bytes(int n, int d);
int va_pca_chunk_rows(int n, int d);
int va_pca_moments(va_ctx* ctx, const void* x, int n, int d, int first, void* sums, void* workspace, size_t workspace_bytes,
                   void* stream);
/* out float32 [n][m] = (x - mean) components^T: x float32 [n][d], mean float64 [d], components float64 [m][d],
 * 1 <= m <= d <= 2048; accumulated in float64 over the columns in ascending groups of four, stored as float32.  No
 * whitening (sklearn's PCA default, Sheet02.py:574). */
int va_pca_transform(va_ctx* ctx, const void* x, int n, int d, const void* mean, const void* components, int m, void* out,
                     void* stream);

/*
 * The statistics of a diagonal-covariance Gaussian mixture, the one hot path of fitting it and of encoding with it.
 * For every row x of x float32 [n][d]:
 *   log p_j = log w_j - 1/2 sum_c (x_c - mu_jc)^2 / var_jc - 1/2 sum_c log var_jc - d/2 log 2 pi   (evaluated expanded,
 *             [x^2, x] against [-1/(2 var), mu / var], plus a constant per component: DESIGN.md S78)
 *   gamma_j = exp(log p_j - logsumexp_j log p)              mode VA_GMM_SOFT
 *           = 1 for the lowest j that attains max_j log p_j, else 0   mode VA_GMM_HARD
 * and for every segment s (rows segments[s] .. segments[s+1]-1; segments: DEVICE int64 [n_segments + 1], ascending, from 0
 * to n; empty segments allowed):
 *   stats[s][j] = [ S0 = sum gamma_j | S1[d] = sum gamma_j x | S2[d] = sum gamma_j x^2 ]   float64 [n_segments][k][1 + 2d]
 *   loglik[s]   = sum logsumexp_j log p                                                    float64 [n_segments] (both modes)
 * weights [k], means [k][d], variances [k][d]: DEVICE float64.
 * Limits, checked by va_gmm_workspace_bytes (0 and the field's name in va_last_error()): 1 <= n, 1 <= d <= 512,
 * 1 <= k <= 256, 1 <= n_segments <= 65536, 16 <= chunk_rows <= 65536, chunk_rows <= batch_rows <= 65536.
 * Order of the sums: rows are cut into chunks at every multiple of chunk_rows and at every segment boundary; within a
 * chunk rows are added four at a time in ascending order, then the chunks of a segment in ascending order.  The
 * responsibilities exist only for one batch of batch_rows rows (rounded down to a multiple of chunk_rows) at a time, so the
 * workspace does not grow with n: gamma of one batch, the chunk sums of one batch, the expanded parameters.
 */
#define VA_GMM_SOFT 0
#define VA_GMM_HARD 1
typedef struct va_gmm_params {
    int struct_bytes; /* sizeof(va_gmm_params) of the caller; a smaller value is refused */
    int chunk_rows;   /* rows whose statistics are accumulated serially before the chunks are summed; default 1024 */
    int batch_rows;   /* rows whose responsibilities exist at once; default 65536 */
    int reserved[5];
} va_gmm_params;
void va_gmm_default_params(va_gmm_params* p);
size_t va_gmm_workspace_bytes(int n, int d, int k, int n_segments, const va_gmm_params* p);
int va_gmm_stats(va_ctx* ctx, const void* x, int n, int d, const void* segments, int n_segments, const void* weights,
                 const void* means, const void* variances, int k, int mode, const va_gmm_params* p, void* stats, void* loglik,
                 void* workspace, size_t workspace_bytes, void* stream);
/* The responsibilities themselves, for tests and small inputs: gamma float64 [n][k], lse float64 [n] (the row's
 * logsumexp), n <= 65536; the same kernel as va_gmm_stats'.  workspace: va_gmm_workspace_bytes(n, d, k, 1, NULL). */
int va_gmm_posteriors(va_ctx* ctx, const void* x, int n, int d, const void* weights, const void* means, const void* variances,
                      int k, int mode, void* gamma, void* lse, void* workspace, size_t workspace_bytes, void* stream);
/* sklearn's diagonal M-step from the ascending sum of stats over its n_segments segments: nk = S0 + 10 DBL_EPSILON,
 * mu = S1 / nk, var = S2 / nk - 2 (mu S1) / nk + mu^2 + reg_covar, w = nk / sum_j nk (j ascending).  One small kernel. */
int va_gmm_mstep(va_ctx* ctx, const void* stats, int n_segments, int k, int d, double reg_covar, void* weights, void* means,
                 void* variances, void* stream);
/* out float32 [n_segments][k + 2 k d] = [ G_alpha [k] | G_mu [k][d] | G_sigma [k][d] ] (Sheet02.py:611-615), with T =
 * counts[s] (DEVICE int64 [n_segments], the segment's rows) and sigma = sqrt(var):
 *   G_alpha = (S0 - T w) / sqrt(w),  G_mu = (S1 - mu S0) / (sigma sqrt(w)),
 *   G_sigma = ((S2 - 2 mu S1 + mu^2 S0) / var - S0) / sqrt(2 w),
 * all divided by T; power > 0: sign(v) |v|^power (0: none, Sheet02's; 0.5: the improved Fisher vector); then divided by the
 * L2 norm unless that is below 1e-6 (Sheet02.py:39, 112-115).  T = 0 gives zeros.  0 <= power <= 1. */
int va_fisher_encode(va_ctx* ctx, const void* stats, const void* counts, int n_segments, int k, int d, const void* weights,
                     const void* means, const void* variances, double power, void* out, void* stream);

/*
 * Bag of words (csrc/codebook.hip): the k-means codebook and the per-video histograms of the modelled
 * project's Sheet01 (Sheet01.py:259-277).  x: DEVICE float32 [n][d], widened exactly; centres: DEVICE float64 [k][d]; all
 * arithmetic is float64 in a fixed order, there are no floating-point atomics, and nothing of size n * k exists.
 * Limits, checked by va_kmeans_workspace_bytes (0 and the field's name in va_last_error()): 1 <= n <= 2^31 - 1,
 * 1 <= d <= 512, 1 <= k <= 4096, 1 <= n_segments <= 65536, 64 <= chunk_rows <= 2^20.  One workspace size serves every entry
 * point below (256-byte aligned): O(n) integers (labels and a permutation), n / 256 doubles and n k / chunk_rows integers.
 * chunk_rows is the chunk of the counting sort in va_kmeans_update; the sort is stable, so no result depends on it (it is
 * raised internally so that there are never more than 65536 chunks).
 */
#define VA_BOW_NONE 0
#define VA_BOW_L1 1
#define VA_BOW_L2 2
typedef struct va_kmeans_params {
    int struct_bytes; /* sizeof(va_kmeans_params) of the caller; a smaller value is refused */
    int chunk_rows;   /* rows per chunk of the counting sort; default 8192 */
    int reserved[6];
} va_kmeans_params;
void va_kmeans_default_params(va_kmeans_params* p);
size_t va_kmeans_workspace_bytes(int n, int d, int k, int n_segments, const va_kmeans_params* p);
/* The centres of one LDS tile of va_kmeans_assign (64): the sizes at which its tests walk one tile more. */
int va_kmeans_tile_centres(void);
/* labels int32 [n]: the lowest j that attains min_j s_ij, s_ij = 1/2 |c_j|^2 - x_i . c_j (|c_j|^2 summed over the columns in
 * ascending order, the products on the float64 MFMA, centres walked in LDS tiles with a running (min, index) per row; ties
 * go to the lower index).  d2 float64 [n] or NULL: sum_c (x_ic - c_{label,c})^2, columns ascending, computed directly after
 * the arg-min.  inertia float64 [1]: the sum of d2 (blocks of 256 rows by a fixed tree, then the blocks).  changed
 * uint64 [1]: the rows whose label differs from prev_labels (int32 [n], or NULL: every row). */
int va_kmeans_assign(va_ctx* ctx, const void* x, int n, int d, const void* centres, int k, const void* prev_labels, void* labels,
                     void* d2, void* inertia, void* changed, void* workspace, size_t workspace_bytes, void* stream);
/* counts int64 [k]; new_centres float64 [k][d]: the mean of the cluster's rows, added in the tree of DESIGN.md S92 over the
 * rows in ascending order; an empty cluster keeps its centre.  shift2 float64 [1] = sum_j |new_j - old_j|^2, j ascending.
 * Labels outside 0 .. k-1 are counted nowhere. */
int va_kmeans_update(va_ctx* ctx, const void* x, int n, int d, const void* labels, const void* centres, int k,
                     const va_kmeans_params* p, void* counts, void* new_centres, void* shift2, void* workspace,
                     size_t workspace_bytes, void* stream);
/* k-means++ (Arthur and Vassilvitskii; one trial per centre) from u float64 [k] in [0, 1): centre 0 is row floor(u_0 n);
 * for j >= 1, m_i = min(m_i, |x_i - c_{j-1}|^2) and the chosen row is the lowest i whose running sum of m
 * exceeds u_j total, the last row with m_i > 0 if there is none, floor(u_j n) when total = 0.  No host synchronisation.
 * centres float64 [k][d], rows int32 [k], m float64 [n] (as after the last step; +inf when k = 1). */
int va_kmeans_seed(va_ctx* ctx, const void* x, int n, int d, const void* u, int k, void* centres, void* rows, void* m,
                   void* workspace, size_t workspace_bytes, void* stream);
/* out float32 [n_segments][k]: the counts of the labels (int32 [n]) of the rows segments[s] .. segments[s+1]-1 (DEVICE
 * int64 [n_segments + 1], as va_gmm_stats'), counted in integers, then divided once by their L2 norm (VA_BOW_L2, Sheet01's
 * normalize), their sum (VA_BOW_L1) or nothing (VA_BOW_NONE); the norm is float64 over the words in ascending order.  An
 * empty segment gives zeros. */
int va_bow_histograms(va_ctx* ctx, const void* labels, int n, const void* segments, int n_segments, int k, int norm, void* out,
                      void* stream);
/* va_kmeans_assign's labels (kept in the workspace; no d2) followed by va_bow_histograms, in one call. */
int va_bow_encode(va_ctx* ctx, const void* x, int n, int d, const void* centres, int k, const void* segments, int n_segments,
                  int norm, void* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * HMM action segmentation (csrc/hmm.hip): the Gaussian emission table, batched Viterbi decoding and the
 * Baum-Welch statistics of the modelled project's Sheet04 (Kuehne, Arslan and Serre, CVPR 2014; Sheet04.py:242-252, :300-420
 * and :520-560).  All arithmetic is
 * float64 and there are no atomics.
 *
 * A model is flat, in CSR form by predecessor: emit int32 [N] (the state's Gaussian), pred_ptr int32 [N + 1], pred_idx
 * int32 [E] (ascending within a state), pred_logp float64 [E], log_pi and log_final float64 [N]; -inf is legal everywhere,
 * NaN nowhere.  1 <= N <= 1024, any in-degree.  The models of a call are concatenated: state_ptr int32 [n_models + 1] cuts
 * emit, log_pi and log_final, edge_ptr int32 [n_models + 1] cuts pred_idx and pred_logp, and the pred_ptr rows (N + 1 each,
 * counting from 0 within the model) follow one another, so model m's starts at state_ptr[m] + m.  The sequences are the
 * rows seq_ptr[s] .. seq_ptr[s + 1] - 1 of logb (seq_ptr: int32 [n_seqs + 1]).  Every array is a DEVICE array.
 *
 * va_hmm_wave_states, va_hmm_wave_edges: a model of at most that many states (64) and edges (512) runs in the single-wave
 * form of the kernel, every other one in the workgroup form.  va_hmm_backtrack_block: the frames of backpointers (16) that
 * pass through LDS per step of the backtrack.  The results do not depend on any of the three.
 */
int va_hmm_wave_states(void);
int va_hmm_wave_edges(void);
int va_hmm_backtrack_block(void);
/* logb float64 [t_total][g] = consts[g] - 0.5 q, q = the sum over the columns in ascending order of
 * ((x - mean) (x - mean)) inv_var, one rounding per operation.  x: float32 (x_is_f64 = 0, widened exactly) or float64
 * [t_total][d], 1 <= d <= 512; means, inv_var float64 [g][d]; consts float64 [g] (the host's
 * -0.5 (d log 2 pi + sum log var)). */
int va_hmm_emissions(va_ctx* ctx, const void* x, int x_is_f64, int t_total, int d, const void* means, const void* inv_var,
                     const void* consts, int g, void* logb, void* stream);
/* jobs int32 [n_jobs][3]: (sequence, model, want_path).  delta_0[j] = log_pi[j] + logb[0][emit j]; delta_t[j] = max_i
 * (delta_{t-1}[i] + pred_logp[i -> j]) + logb[t][emit j], a predecessor winning only by > over the running best in ascending
 * pred_idx; score float64 [n_jobs] = max_j (delta_{T-1}[j] + log_final[j]), the lowest j on ties.  status int32 [n_jobs]:
 * 0 ok; 1 no path of finite score (score -inf, path -1); 2 a NaN reached the recursion (score NaN, path -1); 3 the job's
 * indices leave the arrays of the call (score NaN, nothing else written).  A job with want_path = 1 writes its states to
 * path[path_off[job] ..] (int32, T entries; path_off, bp_off: int64 [n_jobs], read only for such jobs) and keeps its
 * backpointers, uint16 [T][N], at element bp_off[job] of the workspace; path_elems and bp_elems are the sizes the offsets
 * address, and a workspace below 2 bp_elems bytes is VA_ERR_WORKSPACE with nothing written.  A job with want_path = 0
 * needs no workspace. */
int va_hmm_viterbi(va_ctx* ctx, const void* logb, int t_total, int g, const void* seq_ptr, int n_seqs, const void* state_ptr,
                   const void* edge_ptr, int n_models, int n_states_total, int n_edges_total, const void* emit,
                   const void* pred_ptr, const void* pred_idx, const void* pred_logp, const void* log_pi, const void* log_final,
                   const void* jobs, int n_jobs, const void* path_off, const void* bp_off, void* score, void* status, void* path,
                   size_t path_elems, size_t bp_elems, void* workspace, size_t workspace_bytes, void* stream);
/*
 * The scaled forward-backward pass of the same jobs (the jobs' third column is not read).  With
 * b_t[j] = exp(logb[t][emit j] - m_t), m_t the maximum over the model's states, and a, pi, f the exponentials of pred_logp,
 * log_pi and log_final:
 *   alpha_0[j] = pi[j] b_0[j] / c_0,  alpha_t[j] = b_t[j] (sum_i alpha_{t-1}[i] a[i -> j]) / c_t   (predecessors ascending;
 *   c_t: the frame's sum of the numerators), c_T = sum_j alpha_{T-1}[j] f[j], beta_{T-1}[j] = f[j] / c_T,
 *   beta_t[i] = sum_j a[i -> j] ((b_{t+1}[j] beta_{t+1}[j]) / c_{t+1})   (successors ascending),
 *   gamma_t = alpha_t beta_t,  xi[e] = sum_t (alpha_t[i] a[e]) ((b_{t+1}[j] beta_{t+1}[j]) / c_{t+1})  (t descending),
 *   loglik = sum_t (log c_t + m_t) + log c_T   (t ascending).
 * A frame's sum runs over each wave's lanes as an xor butterfly (offsets 32 .. 1) and then over the waves in ascending
 * order.  succ_ptr (rows laid out like pred_ptr's), succ_idx and succ_edge int32 [E] list every state's successors in
 * ascending order and each edge's place in the model's pred_idx.  Job k writes gamma float64 [T][N] at gamma_off[k], xi
 * float64 [E] at xi_off[k] and uses 2 T doubles of the workspace at mc_off[k] (all int64 [n_jobs], in elements; gamma_elems,
 * xi_elems and mc_elems are the sizes they address).  status: 0 ok; 1 the likelihood is zero -- a frame whose states all
 * have logb -inf, or a c_t that is 0 -- with gamma and xi zeros and loglik -inf; 2 a NaN or +inf in the job's logb, or a
 * c_t that is not finite, with gamma and xi zeros and loglik NaN; 3 as va_hmm_viterbi's.  workspace:
 * va_hmm_fb_workspace_bytes (0 and va_last_error() for sizes out of range), 256-byte aligned; too small a one is
 * VA_ERR_WORKSPACE with nothing written.
 */
size_t va_hmm_fb_workspace_bytes(int n_states_total, int n_edges_total, size_t mc_elems);
int va_hmm_forward_backward(va_ctx* ctx, const void* logb, int t_total, int g, const void* seq_ptr, int n_seqs,
                            const void* state_ptr, const void* edge_ptr, int n_models, int n_states_total, int n_edges_total,
                            const void* emit, const void* pred_ptr, const void* pred_idx, const void* pred_logp, const void* log_pi,
                            const void* log_final, const void* succ_ptr, const void* succ_idx, const void* succ_edge,
                            const void* jobs, int n_jobs, const void* gamma_off, const void* xi_off, const void* mc_off, void* gamma,
                            size_t gamma_elems, void* xi, size_t xi_elems, size_t mc_elems, void* loglik, void* status,
                            void* workspace, size_t workspace_bytes, void* stream);
/* stats float64 [g][1 + 2 d] = [ sum w | sum w x | sum w (x x) ] per Gaussian, x as va_hmm_emissions'.  mode 0: w is gamma;
 * Gaussian k takes the contributions contrib_ptr[k] .. contrib_ptr[k + 1] - 1 (int32 [g + 1]), each a row (first frame,
 * frames T, states N, state j) of contrib int32 [n_contrib][4] whose weights are gamma[contrib_off[c] + t N + j] (int64
 * [n_contrib]).  mode 1: w = 1 on the frames t with align[t] = k (int32 [t_total]; -1 for none).  One wave of four adds the
 * frames t = v, v + 4, ... of each contribution in ascending order, the contributions in ascending order; the result is
 * ((p0 + p1) + p2) + p3.  A contribution that leaves the arrays turns its Gaussian's sum w into NaN. */
int va_hmm_gauss_stats(va_ctx* ctx, const void* x, int x_is_f64, int t_total, int d, int g, int mode, const void* gamma,
                       size_t gamma_elems, const void* contrib_ptr, const void* contrib, const void* contrib_off, int n_contrib,
                       const void* align, void* stats, void* stream);

/* --------------------------------------------------------------- kernel SVMs --- */

/*
 * Gram matrices for the kernel SVM.  x [m][d] and y [n][d] are DEVICE float32 (x_is_f64 = 0) or float64 (1) rows, widened as
 * they are read; out is float64 [m][n].  y == NULL is the symmetric form: n is ignored, out is [m][m], only the 64 x 64 tiles
 * on and above the diagonal are computed and every result is also written to its mirror place, so that out is bitwise
 * symmetric and equal to the call on (x, x).  1 <= m, n <= 2^20, 1 <= d <= 65536, else VA_ERR_INVALID before any launch.
 *
 * va_chi2_distance: out[i][j] = sum_k (x[i][k] - y[j][k])^2 / (x[i][k] + y[j][k]) over the columns c0 <= k < c1 in ascending
 * order (0 <= c0 < c1 <= d), one float64 accumulator per result, every operation IEEE (no contraction); a term whose
 * denominator is 0 counts 0 (sklearn's chi2_kernel convention, no factor 1/2).  The diagonal of the symmetric form is exactly
 * 0.  chunk: the columns staged in LDS at a time, 1 .. 32, 0 for the library's 16; no value changes a result.
 *
 * va_linear_gram: out[i][j] = sum_k x[i][k] y[j][k] on v_mfma_f64_16x16x4_f64, k in a fixed order.
 */
#define VA_CHI2_MAX_CHANNELS 16
int va_chi2_distance(va_ctx* ctx, const void* x, const void* y, int m, int n, int d, int c0, int c1, int x_is_f64, int chunk,
                     void* out, void* stream);
int va_linear_gram(va_ctx* ctx, const void* x, const void* y, int m, int n, int d, int x_is_f64, void* out, void* stream);
/* mean float64 [1] = the mean of the strict upper triangle of dist float64 [n][n], 2 <= n <= 2^20 (Laptev's and Wang's
 * normaliser A of a chi-square channel): rowsum float64 [n] (scratch) takes each row's sum over j > i, lane l of 256 adding
 * j = i + 1 + l, i + 1 + l + 256, ... in ascending order, then an xor butterfly; the rows are added the same way.  No atomics. */
int va_upper_mean(va_ctx* ctx, const void* dist, int n, void* rowsum, void* mean, void* stream);
/* out float64 [count] = exp(-(weights[0] dist[0] + weights[1] dist[1] + ...)), elementwise over n_channels (1 ..
 * VA_CHI2_MAX_CHANNELS) DEVICE float64 arrays of `count` elements, the products added in channel order; dist and weights are
 * HOST arrays, the weights finite and >= 0, 1 <= count <= 2^38.  Distances that are exactly 0 (a symmetric diagonal) give
 * exactly 1. */
int va_chi2_combine(va_ctx* ctx, const void* const* dist, const double* weights, int n_channels, size_t count, void* out,
                    void* stream);

/*
 * The one-vs-rest kernel SVM fit over a Gram matrix: va_linear_svm_fit's model, L2-regularised squared
 * hinge with the regularised bias s = intercept_scaling, posed in the dual.  With Kt = k + s^2 and H = Kt + I / (2C), class row
 * r (y_i = +1 where y[i] is the row's class, -1 elsewhere) solves
 *     min over alpha >= 0 of  1/2 alpha^T ((y y^T) o H) alpha - e^T alpha,
 * dual_coef[r][i] = y_i alpha_i, intercept[r] = s^2 sum_i dual_coef[r][i]; the score of a row x is sum_i dual_coef[r][i]
 * k(x_i, x) + intercept[r], which is va_linear_svm_predict on the test rows of the Gram matrix.  With k = X X^T the model
 * dual_coef [X, s] is va_linear_svm_fit's.  rows = n_classes == 2 ? 1 : n_classes, as there.
 *
 * k float64 [n][n] symmetric positive semi-definite (the caller's promise; only the finite, symmetric part is checked by the
 * Python layer), y i32 [n] with values in [0, n_classes).  The solver is a Newton-CG on the primal written in beta (S107):
 * every outer step judges the feasible candidate by the dual's projected gradient pg and a row stops, and is frozen, when
 * |pg|_2 <= tol sqrt(n).  The call enqueues outer_iters outer steps on the caller's stream and then writes dual_coef f64
 * [rows][n] (alpha >= 0 exactly, zeros exact), intercept f64 [rows] and stats f64 [rows][5] = the dual objective, |pg|, the
 * support vectors, the outer steps taken, the CG steps taken; it allocates nothing and does not synchronise.  restart as
 * va_linear_svm_fit's.  Every product H V serves all rows at once on the float64 MFMA; no atomics: two fits agree bit for bit.
 * workspace: va_kernel_svm_fit_workspace_bytes(n, rows) bytes, 8-byte aligned (too small: VA_ERR_WORKSPACE).  2 <= n <=
 * 16384, 2 <= n_classes <= 1024, C > 0, tol > 0, intercept_scaling >= 0, all finite, 0 <= outer_iters <= 1000, else
 * VA_ERR_INVALID before anything is launched.  The size query answers 0 and sets va_last_error for sizes out of range
 * (n_class_rows is 1 or 3 .. 1024).
 */
size_t va_kernel_svm_fit_workspace_bytes(int n, int n_class_rows);
int va_kernel_svm_fit(va_ctx* ctx, const void* k, const void* y, int n, int n_classes, double C, double intercept_scaling,
                      double tol, int outer_iters, int restart, void* dual_coef, void* intercept, void* stats,
                      void* workspace, size_t workspace_bytes, void* stream);
/*
 * The stages of va_kernel_svm_fit one at a time, for stage-by-stage tests; the fit's own loop is written over the same helpers.
 *
 * va_kernel_svm_fit_layout (host only): offsets: HOST size_t[VA_KSVM_FIT_FIELDS], the byte offsets into the workspace of
 *   B HB BC Z X R P HP Q   f64 [rows][n]   iterate beta, H B, the feasible candidate, H BC, the CG's solution (then the step
 *                                          S = X - B), CG residual, CG direction, H P on the face, H S
 *   free                   i32 [rows][n]   the row's face: 1 where 1 - y f > 0
 *   q pgn nsv steps rr cgtol cgs ref   f64 [rows]   dual objective, |pg|, support vectors, outer steps, the CG's |R|^2 and
 *                                          stop threshold, CG steps, the size of the Newton system's right-hand side
 *   live notdone tight     i32 [rows]      the row's CG is running; the row has not met the stop rule; its last step was refused
 * in this order, each on a 256-byte boundary.  Returns the total, equal to va_kernel_svm_fit_workspace_bytes; sizes out of
 * range, offsets == NULL or count != VA_KSVM_FIT_FIELDS answer 0 and set va_last_error.
 *
 * va_kernel_svm_fit_phase: the arguments and checks of va_kernel_svm_fit.  It reads and writes the state in the workspace:
 *   VA_KSVM_PHASE_INIT         k_ksvm_init: every vector and scalar 0, notdone 1
 *   VA_KSVM_PHASE_EVAL         k_ksvm_prod (HB = H B), k_ksvm_face, k_ksvm_prod (Z = H BC), k_ksvm_grad: the face, the
 *                              candidate, pg, the stop rule, and the start of the CG (X = BC, R = P = y - Z on the face)
 *   VA_KSVM_PHASE_CG           `count` (1 .. 100) rounds of k_ksvm_prod<masked> (HP = H P on the face) and k_ksvm_cg
 *   VA_KSVM_PHASE_LINE_SEARCH  k_ksvm_dir (S = X - B), k_ksvm_prod (Q = H S), k_ksvm_ls
 * `count` is read by the CG phase only.  One outer step of the fit is CG with count 100, LINE_SEARCH, EVAL; restart = 1 is
 * INIT, EVAL.
 */
#define VA_KSVM_FIT_FIELDS 21
#define VA_KSVM_PHASE_INIT 0
#define VA_KSVM_PHASE_EVAL 1
#define VA_KSVM_PHASE_CG 2
#define VA_KSVM_PHASE_LINE_SEARCH 3
size_t va_kernel_svm_fit_layout(int n, int n_class_rows, size_t* offsets, int count);
int va_kernel_svm_fit_phase(va_ctx* ctx, const void* k, const void* y, int n, int n_classes, double C,
                            double intercept_scaling, double tol, int phase, int count, void* workspace,
                            size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VA_H */
