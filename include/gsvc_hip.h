/*
 * include/gsvc_hip.h — C-ABI of libgsvc_hip.so, the MI355X (gfx950) hot path of GSVC.
 *
 * Drop-in boundary: these entry points are what a GSVC maintainer binds in place of the two native
 * extensions the renderer path imports (INTEGRATION.md shows the ctypes stubs):
 *
 *   diff_gaussian_rasterization.cuda_ortho_gaussian_rasterizer   (external pip dependency, reference README.md:52)
 *       GaussianRasterizer.visible_filter   call site reference ortho_gaussian_renderer/preprocess.py:99-104
 *       GaussianRasterizer.forward          call site reference ortho_gaussian_renderer/renderer.py:90-98
 *       GaussianRasterizer.backward         implicit via autograd, reference pipeline/train.py:462
 *   _gridencoder                                                  (reference submodules/gridencoder.zip)
 *       grid_encode_forward / grid_encode_backward   gridencoder.zip!gridencoder/src/gridencoder.h:12-36,
 *                                                    call sites reference utils/encodings.py:529-553,582-610
 *   utils/entropy_models.py EntropyGaussian (+Low_bound)           reference utils/entropy_models.py:32-68,159-175
 *
 * TWO KINDS OF ENTRY POINTS.  A maintainer who swaps GSVC's native extensions for this library binds the EIGHTEEN marked
 * [BOUNDARY] — they have the shape of the calls GSVC makes today — and can ignore the rest:
 *
 *   rasterizer   gsvc_raster_sizes_query, gsvc_raster_visible_filter, gsvc_raster_forward, gsvc_raster_backward_scratch_bytes,
 *                gsvc_raster_backward   (+ gsvc_raster_forward_pair: the decoder's two-view frame of report_utils.py:297-319 in one pass)
 *                (+ gsvc_raster_{visible_filter,forward,backward}_ex: SH colours / precomputed 3-D covariances)
 *   hash grid    gsvc_grid_forward, gsvc_grid_backward                      (= grid_encode_forward / grid_encode_backward)
 *   rate         gsvc_rate_forward, gsvc_rate_backward                      (= EntropyGaussian.forward + Low_bound's backward)
 *   codec        gsvc_ans_segments, gsvc_ans_scratch_bytes, gsvc_ans_encode, gsvc_ans_decode_scratch_bytes, gsvc_ans_decode
 *                                                                             (= gsvc_cuda_ans.ANSCoder behind encoder_gaussian / decoder_gaussian)
 *   init         gsvc_knn3_mean_dist2                                         (= simple_knn._C.distCUDA2)
 *   always       gsvc_last_error, gsvc_version
 *
 * Everything else is [INTERNAL]: fusion entries that gsvc_amd's own host code (gsvc_amd/ *.py) calls to run the fitting step and
 * the decoder loop in ~170 launches instead of ~2 000 — batched / un-compacted forms of the same arithmetic (several views, whole
 * MLPs, the step's loss terms, the optimizer, the step plan), each with a parity test against the tensor expression or reference
 * function it replaces (cited at the declaration).  They are exported because the host side is Python over ctypes; their
 * signatures follow gsvc_amd's needs, not GSVC's API, and may change between rounds.  INTEGRATION.md section 1 has the same map
 * with the reference call site of every [BOUNDARY] entry.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless its name ends in _host;
 *   - the caller owns every buffer (outputs, scratch blobs); nothing is allocated or freed inside, nothing
 *     synchronises the device, so every call may be captured into a hipGraph;
 *   - every call is enqueued on `stream` (a hipStream_t passed as void*): every kernel and helper kernel of it (buffers an entry
 *     zeroes are zeroed by a kernel, not by hipMemsetAsync: csrc/common.h, zero_words_async);
 *   - before a capture, make one eager call through each entry family the graph will hold: a process's first call through a family
 *     may set kernel attributes, and the entropy coder's first use uploads its Phi table with a synchronous copy (see
 *     gsvc_ans_table_checksum);
 *   - what is tested of this: tests/test_abi_contract_gpu.py captures and replays one case per entry family of the fitting step and
 *     the decoder, the rasterizer's forward and backward have their own graph test.  NOT established: capture of
 *     gsvc_generate_all_forward / _backward (the inference forward included), whose case stopped the device and was withdrawn, and
 *     of the front-end analysis entries (flow, detail, scene, tfilter, frames_from_*, frames_sse, msssim, grain_stats, block_sse,
 *     knn), which have no case;
 *   - return value: 0 = ok, negative = GSVC_E_*; gsvc_last_error() gives the message of the calling
 *     thread's last failure;
 *   - float = IEEE binary32, row-major, contiguous.
 */
#ifndef GSVC_HIP_H
#define GSVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSVC_OK 0
#define GSVC_E_INVALID (-1)   /* bad argument (null pointer, negative size, unsupported shape) */
#define GSVC_E_LAUNCH (-2)    /* HIP reported a launch error */
#define GSVC_E_UNSUPPORTED (-3)

const char *gsvc_last_error(void);
/* "gsvc_hip <version> gfx950" */
const char *gsvc_version(void);

/* Per-kernel timing for bench.py (not a drop-in entry point).  While enabled, every kernel launch made by
 * this library is bracketed by hipEvents on its own stream.  gsvc_profile_collect synchronises those events
 * and returns, per kernel name, the launch count and total milliseconds since the last collect/enable.
 * names_out: `max_kernels` slots of 64 bytes.  Returns the number of kernels written (<0 on error).
 * `on` is a bit set: 1 = the per-kernel timing; 2 = the compositing backward runs its diagnostic instantiation and adds, per
 * launch, three uint64 to bytes 64..87 of the render's counters block (the start of the binning blob): (entry, quadrant) replays,
 * lanes of those replays that held a contributing pixel, list entries replayed — bench.py's roofline_valu reads them. */
int gsvc_profile_enable(int on);
int gsvc_profile_collect(char *names_out_host, int32_t *launches_out_host, float *total_ms_out_host, int max_kernels);

/* ------------------------------------------------------------------------------------------------------
 * Orthographic sliding-window rasterizer   [BOUNDARY; gsvc_raster_visible_masks and the two *_layout queries are INTERNAL]
 * ---------------------------------------------------------------------------------------------------- */

/* Fields of GaussianRasterizationSettings the extension reads (reference renderer.py:63-83).
 * sh_degree / campos are read only when SH colours are given: they travel in gsvc_raster_sources, the argument of the
 * *_ex entry points, and are not part of this struct; prefiltered / debug carry no information and are not part of the ABI.  viewmatrix is the LOGICAL 4x4 the reference passes (`frame.view_matrix.permute(1,0)`),
 * row-major: p_view = M[:3,:3] p + M[:3,3]. */
typedef struct gsvc_raster_settings {
    int32_t image_height;
    int32_t image_width;
    float x_min;
    float y_min;
    float scale;
    float threshold;
    float scale_modifier;
    float bg[3];
    float viewmatrix[16];
    uint32_t flags;   /* GSVC_RASTER_* convention switches below; 0 = the conventions of DESIGN.md "Raster spec" */
    float low_pass;   /* added to the diagonal of the 2-D covariance, pixels^2; 0 = the default 0.3 (reference
                         arguments/__init__.py:55); GSVC_RASTER_NO_LOW_PASS for none */
} gsvc_raster_settings;

/* Convention switches.  The external CUDA rasterizer's source is not part of the reference tree (README.md:52), so the
 * conventions its call sites do not pin are kept switchable; INTEGRATION.md "Calibrating the rasterizer conventions" shows
 * how to find the combination that reproduces the real extension on one small scene.  Every combination is covered by the
 * oracle <-> dense-float64 cross-check and by HIP <-> oracle parity (tests/test_oracle_raster.py, tests/test_raster_gpu.py). */
#define GSVC_RASTER_SLAB_ONE_SIDED 1u        /* keep -threshold <= z_view <= 0 instead of |z_view| <= threshold (preprocess.py:108-112) */
#define GSVC_RASTER_PIXEL_CORNER 2u          /* u = (x_view - x_min) * scale, without the -0.5 that puts pixel centres on integers */
#define GSVC_RASTER_DEPTH_DESCENDING 4u      /* composite from the largest view-space z to the smallest (ties still by index) */
#define GSVC_RASTER_MEANS2D_PIXEL_UNITS 8u   /* dL_dmeans2D = (dL/du, dL/dv) in pixels instead of NDC units (x W/2, x H/2) */
#define GSVC_RASTER_CLAMP_STOPS_GRADIENT 16u /* no gradient to conic / mean / opacity where the alpha <= 0.99 clamp is active */
#define GSVC_RASTER_NO_LOW_PASS 32u          /* low_pass = 0 exactly */
#define GSVC_RASTER_TIGHT_BINNING 64u       /* a Gaussian is LISTED only in the tiles of its 3-sigma rectangle that its alpha >= 1/255 box
                                               touches (the other instances can contribute nothing: the compositing kernels skip them
                                               anyway): same image, radii, num_rendered (still the 3-sigma count) and gradients (up to
                                               the order large rectangles' rows are added in), shorter lists — late in a fit 40 % of the
                                               3-sigma instances are such.  The pair forward clamps both views' rectangles by the (shared) box */
#define GSVC_RASTER_SH_VIEW_AXIS 128u       /* SH colours (gsvc_raster_sources.shs) are evaluated at the view's constant axis
                                               dir = normalize(viewmatrix[2][0..2]) (world direction of view-space +z) instead of
                                               dir = normalize(p_world - campos); no gradient reaches means3D through dir then */

/* Byte sizes of the three opaque state blobs of one forward call (the 3DGS-lineage "geomBuffer /
 * binningBuffer / imgBuffer" the reference extension hands back to autograd). */
typedef struct gsvc_raster_sizes {
    uint64_t geom_bytes;
    uint64_t binning_bytes;
    uint64_t image_bytes;
} gsvc_raster_sizes;

/* counters written by forward into the first 32 bytes of the binning blob */
typedef struct gsvc_raster_counters {
    int32_t num_rendered; /* sum of the 3-sigma rectangles' tiles (true count even when it overflowed) = the lists' length, except under
                             GSVC_RASTER_TIGHT_BINNING, where the lists are shorter: their length is tile_offsets[T] (gsvc_raster_binning_layout) */
    int32_t overflow;     /* 1 when the lists' length (reserved[2]; = num_rendered except under GSVC_RASTER_TIGHT_BINNING) > max_instances:
                             image/state are NOT valid, retry with max_instances >= reserved[2] */
    int32_t num_visible;  /* Gaussians with radius > 0 */
    int32_t max_tile_len; /* longest per-tile list */
    int32_t num_big_tiles; /* tiles whose list is sorted by the workgroup kernel (internal) */
    int32_t reserved[3];  /* [0], [1]: internal cursors; [2]: after the forward, the tile lists' length = tile_offsets[T] (true length even
                             when it overflowed): point_list / inst_bbox / the backward's scratch rows are sized by THIS, not by num_rendered */
} gsvc_raster_counters;

int gsvc_raster_sizes_query(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                            gsvc_raster_sizes *sizes_host);

/* radii[P] (int32): >0 iff the Gaussian's 3-sigma ellipse intersects the z-slab and the screen. */
int gsvc_raster_visible_filter(const gsvc_raster_settings *settings, int64_t P, const float *means3D,
                               const float *scales, const float *rotations, int32_t *radii, void *stream);
/* The same test for 1..8 views over the same P Gaussians in one launch: masks[r P + i] = (radius under settings[r] > 0).
 * scales: rows scale_stride floats apart, the first three read; scale_exp != 0: they are logarithms (reference
 * scene/gaussian_model.py scaling_activation = exp); rot_normalise != 0: rotations are un-normalised quaternions (rotation_activation
 * = normalize, eps 1e-12) — the per-anchor activations of reference ortho_gaussian_renderer/preprocess.py:88-104 folded in. */
int gsvc_raster_visible_masks(const gsvc_raster_settings *const *settings, int32_t views, int64_t P, const float *means3D,
                              const float *scales, int32_t scale_stride, int32_t scale_exp, const float *rotations,
                              int32_t rot_normalise, uint8_t *masks, void *stream);

/* Forward: means3D[P,3] colors[P,3] opacities[P] scales[P,3] rotations[P,4]  ->  image[3,H,W], radii[P].
 * State blobs sized by gsvc_raster_sizes_query(settings, P, max_instances).  The counters struct sits at
 * byte 0 of `binning`; copy it to the host when num_rendered is needed (the reference API returns it as a
 * python int, reference renderer.py:90). */
int gsvc_raster_forward(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                        const float *means3D, const float *colors, const float *opacities, const float *scales,
                        const float *rotations, float *image, int32_t *radii, void *geom, void *binning,
                        void *image_state, void *stream);

/* Two-view frame in one pass (no backward): image_pair[3,H,W] = (render(view) + flip_W(render(opposite view))) / 2,
 * the frame GSVC's evaluation / decoder output (reference utils/report_utils.py:297-319): the opposite view
 * (frame.view_matrix_s) composites the same Gaussians at the mirrored pixels in reverse depth order, so one binning
 * and one walk of the tile lists produce both composites.  Same arguments as gsvc_raster_forward with `settings`
 * holding the forward view; final_T / n_contrib are not produced.  Agrees with two gsvc_raster_forward calls to
 * < 2e-4 per pixel (the opposite view's own early exit is not replayed). */
int gsvc_raster_forward_pair(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                             const float *means3D, const float *colors, const float *opacities, const float *scales,
                             const float *rotations, float *image_pair, int32_t *radii, void *geom, void *binning,
                             void *image_state, void *stream);

/* Backward: dL_dimage[3,H,W] + the forward's inputs and state  ->  gradients (all overwritten):
 * dL_dmeans3D[P,3], dL_dmeans2D[P,3] (screen-space gradient in NDC units, the tensor GSVC's densification
 * reads, reference scene/gaussian_model.py:1311), dL_dcolors[P,3], dL_dopacities[P], dL_dscales[P,3],
 * dL_drotations[P,4].  `scratch`: gsvc_raster_backward_scratch_bytes(P, max_instances) bytes (one 64-byte row of
 * partial sums per (tile, Gaussian) instance; every row that is read is written first, nothing needs zeroing).
 * No float atomics: two calls on the same inputs return bit-identical gradients. */
int64_t gsvc_raster_backward_scratch_bytes(int64_t P, int64_t max_instances);
int gsvc_raster_backward(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                         const float *means3D, const float *colors, const float *opacities, const float *scales,
                         const float *rotations, const int32_t *radii, const void *geom, const void *binning,
                         const void *image_state, const float *dL_dimage, float *dL_dmeans3D, float *dL_dmeans2D,
                         float *dL_dcolors, float *dL_dopacities, float *dL_dscales, float *dL_drotations,
                         void *scratch, void *stream);

/* Optional inputs of the 3DGS-lineage rasterizer call the _ex entry points below complete: GaussianRasterizer(shs=...,
 * cov3D_precomp=...) and visible_filter(cov3D_precomp=...) of diff_gaussian_rasterization (reference
 * ortho_gaussian_renderer/renderer.py:85-98, preprocess.py:99-104, arguments/__init__.py:130-131). */
typedef struct gsvc_raster_sources {
    const float *shs;        /* [P, sh_coeffs, 3] or NULL (then `colors` is read) */
    int32_t sh_degree;       /* active degree 0..3; (sh_degree+1)^2 <= sh_coeffs */
    int32_t sh_coeffs;       /* row stride of shs in coefficients (the lineage passes shs.shape[1]) */
    float campos[3];
    const float *cov3D;      /* [P, 6] = xx, xy, xz, yy, yz, zz, or NULL (then scales/rotations are read) */
} gsvc_raster_sources;

/* [BOUNDARY] The forms of gsvc_raster_visible_filter / _forward / _backward that take gsvc_raster_sources.  Exactly one colour
 * source (colors or sources->shs) and exactly one covariance source (scales + rotations, or sources->cov3D) must be given; the
 * unused pointers are NULL.  SH colours: colour = max(sum_k basis_k(dir) sh[k] + 0.5, 0) per channel over the (sh_degree+1)^2
 * real spherical-harmonic functions of the 3DGS lineage, dir as GSVC_RASTER_SH_VIEW_AXIS says.  A precomputed covariance is
 * used as given (scale_modifier is not applied to it, as in the lineage).  Single view only (no _pair form). */
int gsvc_raster_visible_filter_ex(const gsvc_raster_settings *settings, int64_t P, const float *means3D,
                                  const float *scales, const float *rotations, const gsvc_raster_sources *sources,
                                  int32_t *radii, void *stream);
int gsvc_raster_forward_ex(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                           const float *means3D, const float *colors, const float *opacities, const float *scales,
                           const float *rotations, const gsvc_raster_sources *sources, float *image, int32_t *radii,
                           void *geom, void *binning, void *image_state, void *stream);
/* As gsvc_raster_backward, plus dL_dshs[P, sh_coeffs, 3] (coefficients beyond the active degree get 0) and dL_dcov3D[P, 6] (the
 * gradient with respect to the six stored numbers: an off-diagonal one carries both symmetric entries), each may be NULL.
 * With cov3D, dL_dscales / dL_drotations are zero; with shs, dL_dmeans3D includes the term through dir (default convention). */
int gsvc_raster_backward_ex(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                            const float *means3D, const float *colors, const float *opacities, const float *scales,
                            const float *rotations, const gsvc_raster_sources *sources, const int32_t *radii,
                            const void *geom, const void *binning, const void *image_state, const float *dL_dimage,
                            float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacities,
                            float *dL_dscales, float *dL_drotations, float *dL_dshs, float *dL_dcov3D, void *scratch,
                            void *stream);

/* [BOUNDARY] The _ex entry points plus two per-pixel maps of the same composite, the ones 3DGS-lineage code reads next to the
 * image: depth[H, W] = sum_i w_i z_i (w_i = alpha_i T_i the compositing weight, z_i = viewmatrix[2,:3] . p_i + viewmatrix[2,3]
 * the view-space z of the slab test; not normalised: the mean depth is depth / alpha) and alpha[H, W] = 1 - T_final.  Every
 * decision is the image's, under every GSVC_RASTER_* switch.  `sources` may be NULL (colors + scales / rotations).  Each map
 * pointer may be NULL: that map is not written.  The backward takes dL_ddepth[H, W] and dL_dalpha[H, W] next to dL_dimage, each
 * may be NULL (= zero): the two maps are two more colour channels (z_i and 1) on a zero background, and dL/dz_i adds
 * dL/dz_i viewmatrix[2,:3] to dL_dmeans3D.  With both map pointers NULL these are the _ex calls, kernel for kernel.  Single view
 * only (no _pair form). */
int gsvc_raster_forward_aux(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                            const float *means3D, const float *colors, const float *opacities, const float *scales,
                            const float *rotations, const gsvc_raster_sources *sources, float *image, int32_t *radii,
                            void *geom, void *binning, void *image_state, float *depth, float *alpha, void *stream);
int gsvc_raster_backward_aux(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                             const float *means3D, const float *colors, const float *opacities, const float *scales,
                             const float *rotations, const gsvc_raster_sources *sources, const int32_t *radii,
                             const void *geom, const void *binning, const void *image_state, const float *dL_dimage,
                             const float *dL_ddepth, const float *dL_dalpha, float *dL_dmeans3D, float *dL_dmeans2D,
                             float *dL_dcolors, float *dL_dopacities, float *dL_dscales, float *dL_drotations,
                             float *dL_dshs, float *dL_dcov3D, void *scratch, void *stream);

/* Test/inspection helpers: locate the sorted per-tile lists inside the binning blob.
 * tile_offsets_host_out: byte offset of int32 tile_offsets[T+1]; point_list: byte offset of int32 ids. */
int gsvc_raster_binning_layout(const gsvc_raster_settings *settings, int64_t P, int64_t max_instances,
                               uint64_t *tile_offsets_byte_off_host, uint64_t *point_list_byte_off_host);
int gsvc_raster_image_layout(const gsvc_raster_settings *settings, uint64_t *final_T_byte_off_host,
                             uint64_t *n_contrib_byte_off_host);

/* ------------------------------------------------------------------------------------------------------
 * Multi-resolution hash grid (replaces _gridencoder.grid_encode_forward / grid_encode_backward)   [BOUNDARY; the _ex / _packed
 * forms and gsvc_pack_sign_bits are INTERNAL]
 * ---------------------------------------------------------------------------------------------------- */

/* inputs[N,D] in [0,1]; embeddings[rows,C]; offsets[L+1], resolutions[L] (int32, device, already sliced to
 * the levels to compute); outputs[L,N,C]; dy_dx[N, L*D*C] or NULL.
 * D in {1,2,3}, C in {1,2,4,8,16,32} (else GSVC_E_UNSUPPORTED with the reference's message). */
int gsvc_grid_forward(const float *inputs, const float *embeddings, const int32_t *offsets,
                      const int32_t *resolutions, float *outputs, uint32_t N, uint32_t D, uint32_t C, uint32_t L,
                      float *dy_dx, void *stream);

/* grad[L,N,C]; grad_embeddings[rows,C] is ACCUMULATED into (caller zero-fills, reference encodings.py:574);
 * grad_inputs[N,D] is overwritten when dy_dx != NULL. */
int gsvc_grid_backward(const float *grad, const float *inputs, const float *embeddings, const int32_t *offsets,
                       const int32_t *resolutions, float *grad_embeddings, uint32_t N, uint32_t D, uint32_t C,
                       uint32_t L, const float *dy_dx, float *grad_inputs, void *stream);

/* The same kernels with the caller's layout (no input-gradient path): the points' coordinates are columns in_col[0..D) of a
 * row-major [N, in_stride] matrix, the features of (level l, point b) are the C floats at l * feat_level_stride +
 * b * feat_point_stride of `outputs` / `grad` (strides in floats, multiples of min(C, 4)).  Several grids over the same
 * positions — Mix3d2dEncoding, reference scene/gaussian_model.py:81-147 — write their column blocks of ONE [N, sum L C] matrix
 * (feat_level_stride = C, feat_point_stride = its row length) and read the gradient the same way: no slices, permutes or cat. */
typedef struct gsvc_grid_io {
    int64_t feat_level_stride, feat_point_stride;
    int32_t in_stride, in_col[3];
} gsvc_grid_io;
int gsvc_grid_forward_ex(const float *inputs, const float *embeddings, const int32_t *offsets, const int32_t *resolutions,
                         float *outputs, uint32_t N, uint32_t D, uint32_t C, uint32_t L, const gsvc_grid_io *layout, void *stream);
int gsvc_grid_backward_ex(const float *grad, const float *inputs, const int32_t *offsets, const int32_t *resolutions,
                          float *grad_embeddings, uint32_t N, uint32_t D, uint32_t C, uint32_t L, const gsvc_grid_io *layout,
                          void *stream);

/* Several grids over the SAME points in one launch each way (Mix3d2dEncoding: one 3-D + three 2-D grids, reference
 * scene/gaussian_model.py:81-147 calls the four encoders one after the other): `features` is the grid's column block of the shared
 * [N, sum L C] matrix (forward: written; backward: the gradient, read), `layout` as for gsvc_grid_forward_ex.  Same arithmetic per
 * (grid, level, point) as the single-grid entries — the tables' gradients are added into grad_embeddings (zero them first); 1..4
 * grids of 2 or 3 dimensions, C in {2, 4, 8} features per level for all of them. */
typedef struct gsvc_grid_many_job {
    const float *embeddings;        /* forward: the table; backward: unused (may be NULL) */
    float *features;                /* forward: output block; backward: gradient block (read only) */
    float *grad_embeddings;         /* backward: the table's gradient (accumulated) */
    const int32_t *offsets, *resolutions;
    uint32_t D, L;
    gsvc_grid_io layout;
} gsvc_grid_many_job;
int gsvc_grid_forward_many(const float *inputs, const gsvc_grid_many_job *jobs, int32_t n_jobs, uint32_t N, uint32_t C, void *stream);
int gsvc_grid_backward_many(const float *inputs, const gsvc_grid_many_job *jobs, int32_t n_jobs, uint32_t N, uint32_t C, void *stream);

/* Lookup in BIT-PACKED binarised tables (8 features per row: one byte per row, bit f set = +1, clear = -1 — the {-1, +1} tables of
 * reference utils/encodings.py:375-392 STE_binary as the bitstream carries them: 1/32 of the float tables).  Same interpolation,
 * same results bit for bit as gsvc_grid_forward_ex on the float tables; layout may be NULL (default layout).  Inference only.
 * gsvc_pack_sign_bits: bits[row] from a float table x [rows, 8] (x >= 0 -> 1). */
int gsvc_pack_sign_bits(const float *x, int64_t rows, uint8_t *bits, void *stream);
int gsvc_grid_forward_packed(const float *inputs, const uint8_t *table_bits, const int32_t *offsets, const int32_t *resolutions,
                             float *outputs, uint32_t N, uint32_t D, uint32_t L, const gsvc_grid_io *layout, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Entropy-rate estimator (replaces utils/entropy_models.py EntropyGaussian.forward + Low_bound backward)   [BOUNDARY: gsvc_rate_forward /
 * _backward; the sampled-rate entries below them are INTERNAL]
 * ---------------------------------------------------------------------------------------------------- */

/* bits[n,c] = -log2(max(Phi((x+Q/2-mu)/sigma) - Phi((x-Q/2-mu)/sigma), 2^-16)) with x clamped to
 * [x_lo, x_hi] first (the caller computes x_mean -/+ 15000*mean(Q), reference entropy_models.py:40-47;
 * NULL disables; device scalars, or one pair per row [n] when bounds_per_row != 0 — used when several renders
 * are batched into one call).  x, mean, scale: [n,c];  Q: [n] (per row) or NULL with Q_scalar.
 * row_weight: [n,c] multiplier folded into the sum (the offsets mask) or NULL.
 * Outputs: bits[n,c] (may be NULL) and bits_sum[1] (may be NULL; double precision accumulate in a fixed order, float result,
 * ADDED to what it held).  scratch: gsvc_rate_forward_scratch_floats() floats, needed (and written) only with bits_sum. */
int64_t gsvc_rate_forward_scratch_floats(void);
int gsvc_rate_forward(const float *x, const float *mean, const float *scale, const float *Q, float Q_scalar,
                      const float *weight, const float *x_lo, const float *x_hi, int32_t bounds_per_row, int64_t n,
                      int64_t c, float *bits, float *bits_sum, float *scratch, void *stream);

/* d(sum(weight*bits)*gscale)/d{x, mean, scale, Q[n], weight}; any output pointer may be NULL.
 * Low_bound rule: gradient passes only where the likelihood >= 2^-16 (reference entropy_models.py:166-175,
 * net effect). gscale_dev: device scalar multiplying every gradient (dL/d bits_sum). dQ[n] is accumulated. */
int gsvc_rate_backward(const float *x, const float *mean, const float *scale, const float *Q, float Q_scalar,
                       const float *weight, const float *x_lo, const float *x_hi, int32_t bounds_per_row, int64_t n,
                       int64_t c, const float *gscale_dev, float *dx, float *dmean, float *dscale, float *dQ, float *dweight,
                       void *stream);

/* Sampled rate of the R (<= 16) renders of a fitting step in one pass (reference ortho_gaussian_renderer/guassian.py:73-132,
 * evaluated per render there): the n_sel selected rows (sel: row of x / Q / mask; sel_ctx: row of mean / scale, NULL = sel)
 * are gathered, clamped to x_mean[g] (a device array) -+ 15000 * (mean of Q[g] over the selected rows of the row's render), priced as in
 * gsvc_rate_forward and summed per render and group: S[r][g], g = 0 feature, 1 scaling, 2 offsets (weighted by
 * mask[row][col / 3] when mask != NULL).  row_bounds[renders + 1] (host): row offsets of the renders.
 * scratch: gsvc_rate_sample_scratch_floats(n_sel) floats; the forward leaves the per-render step statistics there and the
 * backward reads them.  Backward: gS[r][g] = dL/dS; dx[g] / dQ[g] rows are STORED (selected rows are distinct), dmean[g] /
 * dscale[g] / dmask are ADDED (rows of the context may repeat): all of them dense, zero-filled by the caller. */
typedef struct gsvc_rate_sample {
    const float *x[3], *mean[3], *scale[3], *Q[3];
    const float *mask;
    const int64_t *sel, *sel_ctx, *row_bounds;
    const float *x_mean;            /* device, 3 floats */
    int32_t C[3];
    int32_t K, renders;
    int64_t n_sel;
} gsvc_rate_sample;
int64_t gsvc_rate_sample_scratch_floats(int64_t n_sel);
int gsvc_rate_sample_forward(const gsvc_rate_sample *desc, float *scratch, float *S, void *stream);
int gsvc_rate_sample_backward(const gsvc_rate_sample *desc, const float *scratch, const float *gS, float *const *dx,
                              float *const *dmean, float *const *dscale, float *const *dQ, float *dmask, void *stream);

/* Normalisation of the sampled rate (reference gaussian_renderer/guassian.py:110-132 per render): out[r] = {all, features,
 * scalings, offsets} bits per coded parameter = S[r][g] / (n_sel_r dims[g]) x keep rate_r, keep rate = the render's rows whose K
 * offset masks (offset_masks [rows, K]) sum to more than 0 / its rows; n_sel_r = entries of the sorted row list sel inside
 * [row_bounds[r], row_bounds[r+1]).  coef [R, 4] (saved for the backward) = d out[r][i] / d S; sum[0] = sum_r out[r][0].
 * backward: gS [R, 3] from g_out [R, 4] and / or g_sum [1] (either may be NULL). */
int64_t gsvc_rate_normalise_scratch_bytes(void);
int gsvc_rate_normalise_forward(const float *S, const float *offset_masks, int32_t K, const int64_t *sel, int64_t n_sel,
                                const int64_t *row_bounds_host, int32_t R, const float *dims3_host, void *scratch, float *out,
                                float *coef, float *sum, void *stream);
int gsvc_rate_normalise_backward(const float *coef, const float *g_out, const float *g_sum, int32_t R, float *gS, void *stream);

/* Densification statistics of un-compacted renders (reference scene/gaussian_model.py:1281-1314 training_statis): row i of
 * the concatenated renders is anchor vis[i] with K Gaussians; opacity_accum[a] += sum_k max(opacity, 0), anchor_denom[a] += 1,
 * and where seen[i K + k]: grad_accum[a K + k] += |grad[i K + k][0:2]|, denom[a K + k] += 1 (grad rows grad_stride floats apart). */
int gsvc_training_statis(const int64_t *vis, const float *opacity, const uint8_t *seen, const float *grad, int32_t grad_stride,
                         int64_t rows, int32_t K, float *opacity_accum, float *anchor_denom, float *grad_accum, float *denom,
                         void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Image distortion of the fitting step (replaces utils/loss_utils.py l1_loss_func + ssim_func and their autograd)   [INTERNAL]
 * ---------------------------------------------------------------------------------------------------- */

/* img1, img2: [C,H,W].  workspace: 2048 floats of scratch.  sums[2] (device): sums[0] = sum of the SSIM map (11x11 Gaussian window,
 * sigma 1.5, zero padding, C1=.01^2, C2=.03^2, reference loss_utils.py:52-72), sums[1] = sum |img1-img2|
 * (:20-21); divide by C*H*W for the reference's means.  dm_*: [C,H,W] partial maps kept for the backward, or
 * all three NULL when no gradient is needed. */
int gsvc_ssim_l1_forward(const float *img1, const float *img2, int32_t C, int32_t H, int32_t W, float *sums,
                         float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12, void *stream);

/* dL_dimg1[C,H,W] = grads[0] * d(mean SSIM)/d img1 + grads[1] * d(mean |img1-img2|)/d img1; grads: device [2]. */
int gsvc_ssim_l1_backward(const float *img1, const float *img2, int32_t C, int32_t H, int32_t W, const float *grads,
                          const float *dm_dmu1, const float *dm_de11, const float *dm_de12, float *dL_dimg1,
                          void *stream);

/* The same with the first image formed on load as the two-view frame 0.5 * (img_f + flip_W(img_b)) (reference
 * pipeline/train.py:368-375); avg_out (may be NULL) receives that frame; the backward writes both views' gradients. */
int gsvc_ssim_l1_pair_forward(const float *img_f, const float *img_b, const float *img2, int32_t C, int32_t H, int32_t W,
                              float *sums, float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12, float *avg_out,
                              void *stream);
int gsvc_ssim_l1_pair_backward(const float *img_f, const float *img_b, const float *img2, int32_t C, int32_t H, int32_t W,
                               const float *grads, const float *dm_dmu1, const float *dm_de11, const float *dm_de12,
                               float *dL_dimg_f, float *dL_dimg_b, void *stream);

/* Spatially weighted distortion (csrc/wdist.hip; no counterpart in the reference).  weights: float32 [Hc, Wc], Hc = ceil(H / cell),
 * Wc = ceil(W / cell), cell 4, 8 or 16, finite and >= 0; pixel (y, x) of every channel has the weight w[y / cell][x / cell].
 * forward: window, padding, moments and map of gsvc_ssim_l1_forward, on x = img1 or, with img1b, on the two-view frame
 * 0.5 * (img1 + flip_W(img1b)), which avg_out (required then, optional otherwise) receives.  sums[0] = sum w ssim, sums[1] = sum w |x - img2|;
 * the three partial maps (all or none) are written already multiplied by the pixel's weight.  workspace: gsvc_wssim_workspace_floats(C, H, W)
 * floats (2 per 32 x 32 tile; -1 for a bad shape): every workgroup stores its own row and a second kernel adds the rows in a fixed order in
 * double, so the sums are the same bits in every run; nothing needs zeroing.
 * backward: dL_dimg1 = grads[0] / (C H W) * (the blurred weighted maps combined with x and img2, as gsvc_ssim_l1_backward)
 * + ((grads[1] / (C H W)) * w) * sign(x - img2); with img1b both views receive half of it, dL_dimg1b flipped (required then, NULL otherwise). */
int64_t gsvc_wssim_workspace_floats(int32_t C, int32_t H, int32_t W);
int gsvc_wssim_l1_forward(const float *img1, const float *img1b, const float *img2, const float *weights, int32_t C, int32_t H, int32_t W,
                          int32_t cell, float *sums, float *workspace, float *dm_dmu1, float *dm_de11, float *dm_de12, float *avg_out,
                          void *stream);
int gsvc_wssim_l1_backward(const float *img1, const float *img1b, const float *img2, const float *weights, int32_t C, int32_t H, int32_t W,
                           int32_t cell, const float *grads, const float *dm_dmu1, const float *dm_de11, const float *dm_de12,
                           float *dL_dimg1, float *dL_dimg1b, void *stream);

/* out[f, cy, cx] (int64 [n, Hc, Wc], 8-byte aligned) = the sum of squared differences of the luma codes of frames a[f], b[f] over cell
 * (cy, cx); yuv420p / yuv444p frames of 8 .. 16 bits, both buffers `stride` bytes apart (deep formats: even bases and stride); cell 4, 8
 * or 16, partial cells at the right and bottom edges sum their own pixels.  Exact (every sum < 2^40); one launch; the sum over a frame's
 * cells is gsvc_frames_sse's luma entry. */
int gsvc_frames_block_sse(const uint8_t *a, const uint8_t *b, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                          int32_t cell, int64_t *out, void *stream);

/* STE_binary forward (reference utils/encodings.py:375-392: y = x >= 0 ? +1 : -1) and count[0] = number of +1 entries
 * (the hash-bit term of the loss, pipeline/train.py:456, needs it); n < 2^24. */
int gsvc_ste_binary_count(const float *x, int64_t n, float *y, float *count, void *stream);
/* The same for up to 8 tables in one launch (x[k], y[k]: n[k] floats; counts[k]); its straight-through backward
 * grad_x[k][i] = |x[k][i]| <= 1 ? grad_y[k][i] + 0.5 count_grads[k count_grad_stride] : 0 (grad_y[k] or count_grads may be NULL = zero: a table
 * entry's share of its count is 1/2); and the Bernoulli code length of the tables from their counts (reference
 * utils/encodings.py:34-51 get_binary_vxl_size over all tables, pipeline/train.py:456): out[0] = bits, out[1] = d bits / d count
 * (the counts are added, and total - ones is formed, exactly: total may exceed 2^24). */
int gsvc_ste_binary_count_many(const float *const *x, float *const *y, const int64_t *n, int32_t tables, float *counts, void *stream);
int gsvc_ste_binary_backward_many(const float *const *x, const float *const *grad_y, const int64_t *n, int32_t tables,
                                  const float *count_grads, int32_t count_grad_stride, float *const *grad_x, void *stream);
int gsvc_table_bits(const float *counts, int32_t tables, int64_t total, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Per-Gaussian loss terms of the fitting step over UN-COMPACTED renders (every visible anchor contributes its K
 * Gaussians; mask[i] = opacity_i > 0)
 * ---------------------------------------------------------------------------------------------------- */

/* Optical-flow consistency of one adjacent-frame pair (reference utils/loss_utils.py:76-135,
 * calc_optical_loss_one_frame): over the Gaussians alive in both renders (same anchor, same offset slot) whose
 * frame-t pixel round((xy1 - (x_min, y_min)) * scale) lies inside [0, x_pix_max) x [0, y_pix_max):
 *   sums[0] = sum |(xy2 - xy1) - flow[:, py, px] / scale|_1,  sums[1] = number of such Gaussians;  loss = sums[0] / (2 sums[1]).
 * world{1,2}: [n,3] positions before the bound clamp; vis{1,2}: int64 anchor index of each row of K Gaussians;
 * flow: [2, flow_h, flow_w].  Scratch (caller-allocated): table int32[anchors*K], partner int32[n1] (kept for backward),
 * partial float[2*ceil(n1/256)] (per-workgroup sums; a second small kernel adds them — no atomics, deterministic). */
int gsvc_optical_forward(const float *world1, const uint8_t *mask1, const int64_t *vis1, int64_t n1, const float *world2,
                         const uint8_t *mask2, const int64_t *vis2, int64_t n2, int32_t K, int64_t anchors, const float *flow,
                         int32_t flow_h, int32_t flow_w, float x_min, float y_min, float scale, int32_t x_pix_max,
                         int32_t y_pix_max, int32_t *table, int32_t *partner, float *sums, float *partial, void *stream);
/* grad_world{1,2}[n,3] = d(loss)/d(world) * grad_out[0] (device scalar); both are overwritten. */
int gsvc_optical_backward(const int32_t *partner, int64_t n1, int64_t n2, const float *sums, const float *grad_out,
                          float *grad_world1, float *grad_world2, void *stream);

/* The same loss summed over P disjoint pairs of renders that are row ranges of ONE set of tensors (a fitting step's renders
 * f1, b1, f2, b2 concatenated, pairs f1 -> f2 and b1 -> b2: reference utils/loss_utils.py:138-153 calc_optical_loss).  world [N, 3],
 * mask [N], vis [N / K] cover all R renders, gaussian_offsets_host [R + 1]; pair p takes its frame-t Gaussians from render
 * pair_src_host[p] and their partners from pair_dst_host[p].  loss[0] = sum_p sums[2p] / (2 sums[2p + 1]).  Scratch: table
 * int32 [R, anchors] (anchor -> row + 1, kept for the backward), partner int32 [N], sums float [2 P], partial float
 * [gsvc_optical_many_partial_floats].  backward: grad_world [N, 3] is written completely (zeros outside the pairs). */
int64_t gsvc_optical_many_partial_floats(const int64_t *gaussian_offsets_host, int32_t R, const int32_t *pair_src_host,
                                         const int32_t *pair_dst_host, int32_t P, int32_t K);
int gsvc_optical_many_forward(const float *world, const uint8_t *mask, const int64_t *vis, const int64_t *gaussian_offsets_host, int32_t R,
                              const int32_t *pair_src_host, const int32_t *pair_dst_host, int32_t P, int32_t K, int64_t anchors,
                              const float *flow, int32_t flow_h, int32_t flow_w, float x_min, float y_min, float scale,
                              int32_t x_pix_max, int32_t y_pix_max, int32_t *table, int32_t *partner, float *sums, float *partial,
                              float *loss, void *stream);
int gsvc_optical_many_backward(const int32_t *partner, const int64_t *vis, const int64_t *gaussian_offsets_host, int32_t R,
                               const int32_t *pair_src_host, const int32_t *pair_dst_host, int32_t P, int32_t K, int64_t anchors,
                               const int32_t *table, const float *sums, const float *grad_out, float *grad_world, void *stream);

/* Regularisers of the R renders of one step (reference pipeline/train.py:417-424) over their concatenated Gaussians
 * (render r = [seg_offsets[r], seg_offsets[r+1]), host array of R+1 entries, R <= 8):
 *   out[0] = sum_r mean_{i in r, mask_i}(scaling_i0 scaling_i1 scaling_i2),  out[1] = sum_r mean_{i in r}(1 - neural_opacity_i).
 * sums: float[3R] kept for backward; partial: float[gsvc_regs_partial_floats()] scratch (per-workgroup sums). */
int64_t gsvc_regs_partial_floats(const int64_t *seg_offsets_host, int32_t R);
int gsvc_regs_forward(const float *scaling, const float *neural_opacity, const uint8_t *mask, const int64_t *seg_offsets_host,
                      int32_t R, float *sums, float *partial, float *out, void *stream);
int gsvc_regs_backward(const float *scaling, const uint8_t *mask, const int64_t *seg_offsets_host, int32_t R, const float *sums,
                       const float *grad_out, float *grad_scaling, float *grad_opacity, void *stream);

/* Training-time noise quantisation (reference utils/encodings.py:395-409 UniformQuantizer) of x[rows, C] for R renders
 * at once (render r = rows [row_offsets[r], row_offsets[r+1]), host array, R <= 8):
 *   y = clamp(x / Q, c_r - 15000, c_r + 15000) * Q + noise * Q,   c_r = mean(x over render r) / mean(Q over render r),
 * Q = q_rows[row] (per-row step, device) or q_scalar when q_rows is NULL; noise[rows, C] ~ U(-1/2, 1/2) is drawn by the
 * caller.  centre: float[R] (kept for backward); scratch: float[gsvc_noise_quant_scratch_floats()]. */
int64_t gsvc_noise_quant_scratch_floats(const int64_t *row_offsets_host, int32_t R);
int gsvc_noise_quant_forward(const float *x, const float *q_rows, float q_scalar, const float *noise,
                             const int64_t *row_offsets_host, int32_t R, int32_t C, float *scratch, float *centre, float *y,
                             void *stream);
/* grad_x[rows, C] and grad_q_rows[rows] (may be NULL) are overwritten; the centre carries no gradient (C <= 256). */
int gsvc_noise_quant_backward(const float *grad_y, const float *x, const float *q_rows, float q_scalar, const float *noise,
                              const float *centre, const int64_t *row_offsets_host, int32_t R, int32_t C, float *grad_x,
                              float *grad_q_rows, void *stream);

/* STE_multistep over the rows of R renders (reference utils/encodings.py:395-420 with input_mean given, as ortho_gaussian_renderer/
 * guassian.py:205-207 calls it): y = x1 + (round(x1 / Q) Q - x1), x1 = clamp(x / Q, trunc(c_r - 15000), trunc(c_r + 15000)) Q,
 * c_r = x_mean / (mean of Q over render r's rows); x_mean: one float on the device (the whole parameter's mean).  No backward: the
 * caller detaches the result, as the reference does.  scratch: gsvc_noise_quant_scratch_floats floats; bounds: 2 R floats (out). */
int gsvc_ste_quant_forward(const float *x, const float *q_rows, float q_scalar, const float *x_mean, const int64_t *row_offsets_host,
                           int32_t R, int32_t C, float *scratch, float *bounds, float *y, void *stream);

/* Tail of the anchor -> neural-Gaussian generation for un-compacted renders (reference
 * ortho_gaussian_renderer/guassian.py:262-296: opacity mask, sigmoid scaling, normalised rotation, world position, bound
 * clamp), n = rows*K Gaussians, Gaussian i belongs to anchor row i / K.  Inputs: opacity_raw[n], offset_mask[n],
 * grid_offsets[n,3], neural_offset[n,3], scale_rot[n,7], grid_scaling[rows,6], anchor[rows,3]; bounds: 3 host floats each.
 * Outputs: neural_opacity[n], mask[n] (opacity > 0), scaling[n,3], rot[n,4], world[n,3], xyz[n,3]. */
int gsvc_gen_tail_forward(const float *opacity_raw, const float *offset_mask, const float *grid_offsets,
                          const float *neural_offset, const float *scale_rot, const float *grid_scaling, const float *anchor,
                          const float *bound_min3_host, const float *bound_max3_host, int64_t rows, int32_t K,
                          float *neural_opacity, uint8_t *mask, float *scaling, float *rot, float *world, float *xyz, void *stream);
/* Incoming gradients g_* may be NULL (output unused).  d_offsets is the gradient of both grid_offsets and neural_offset;
 * d_anchor may be NULL.  All d_* are overwritten. */
int gsvc_gen_tail_backward(const float *opacity_raw, const float *offset_mask, const float *grid_offsets,
                           const float *neural_offset, const float *scale_rot, const float *grid_scaling, const float *world,
                           const float *bound_min3_host, const float *bound_max3_host, int64_t rows, int32_t K,
                           const float *g_neural_opacity, const float *g_scaling, const float *g_rot, const float *g_world,
                           const float *g_xyz, float *d_opacity_raw, float *d_offset_mask, float *d_offsets, float *d_scale_rot,
                           float *d_grid_scaling, float *d_anchor, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Optimizer (reference scene/gaussian_model.py:1034-1058: torch.optim.Adam(eps=1e-15), 15 parameter groups)   [INTERNAL]
 * ---------------------------------------------------------------------------------------------------- */
typedef struct gsvc_adam_tensor {
    float *param;             /* updated in place */
    const float *grad;
    float *exp_avg;           /* first / second moment, updated in place */
    float *exp_avg_sq;
    int64_t n;                /* elements */
    float lr;
    float bias_correction1;   /* 1 - beta1^t, t = number of updates of this tensor including this one */
    float bias_correction2;   /* 1 - beta2^t */
} gsvc_adam_tensor;

/* One Adam update (no weight decay, no amsgrad) of every tensor in the host array, in one launch per 64 tensors. */
int gsvc_adam_step(int32_t n_tensors, const gsvc_adam_tensor *tensors_host, double beta1, double beta2, double eps, void *stream);
/* The same update unless one of the (<= 4) device words guards_host[k] points to is non-zero when the launch runs: then nothing is
 * written.  A fitting step that updates some tensors before it has read the rasterizer's overflow words back (so that the next
 * step's visibility test can be queued early) passes those words: a step that has to be repeated leaves its parameters alone. */
int gsvc_adam_step_guarded(int32_t n_tensors, const gsvc_adam_tensor *tensors_host, double beta1, double beta2, double eps,
                           const int32_t *const *guards_host, int32_t n_guards, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [BOUNDARY] Model creation: mean squared distance to the 3 nearest neighbours (replaces
 * simple_knn._C.distCUDA2, reference simple-knn.zip simple_knn.cu:185-220, call sites scene/gaussian_model.py:762,784).
 * The caller bins the points into a uniform grid: points_by_cell[n,3] sorted by cell index ((z * gy + y) * gx + x, cell of
 * a point = floor((p - origin) / cell_edge) clamped to the grid), cell_start[gx*gy*gz + 1].  out[n] in the sorted order.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_knn3_mean_dist2(const float *points_by_cell, const int32_t *cell_start, const float *origin3_host, float cell_edge,
                         int32_t gx, int32_t gy, int32_t gz, int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [BOUNDARY; gsvc_ans_decode_many and gsvc_ans_table_checksum are INTERNAL] Entropy coding of quantised attributes with the learned
 * Gaussian model (replaces the external
 * gsvc_cuda_ans.ANSCoder the reference calls through utils/encodings.py:102-245 encoder_gaussian / decoder_gaussian:
 * integer symbols in [min_symbol, max_symbol], one Normal(mu, sigma) per symbol in symbol units).
 * rANS, 20-bit frequencies from the model itself (no tables), independent segments of seg_len symbols; the byte layout
 * is this library's own (the reference's coder is not in its tree): segment k = bytes [seg_offsets[k], seg_offsets[k+1]).
 * ---------------------------------------------------------------------------------------------------- */

/* number of segments / bytes of encode scratch for n symbols */
int64_t gsvc_ans_segments(int64_t n, int32_t seg_len);
/* checksum of the fixed-point Phi table encoder and decoder build their frequencies from: a stream records it, a decoder
 * whose own table differs (another platform's erfc rounded an entry the other way) must refuse the stream.
 * The first call of a process to this or to gsvc_ans_encode / _decode / _decode_many builds the table and uploads it with a
 * synchronous copy (nothing after that).  That copy must not meet a capturing stream: call gsvc_ans_table_checksum() once before
 * capturing a coder call.  Until the table is on the device, gsvc_ans_encode / _decode / _decode_many on a stream that is capturing
 * return GSVC_E_UNSUPPORTED without doing anything (the capture itself goes on). */
uint32_t gsvc_ans_table_checksum(void);
int64_t gsvc_ans_scratch_bytes(int64_t n, int32_t seg_len);

/* symbols[n] (device, int32) -> out (device; capacity gsvc_ans_scratch_bytes is always enough), seg_bytes[segments]
 * (uint32), seg_offsets[segments + 1] (uint64, seg_offsets[segments] = total bytes).  error_flag (device int32, zeroed by
 * the caller) becomes non-zero if a symbol lies outside [min_symbol, max_symbol]. */
int gsvc_ans_encode(const int32_t *symbols, const float *mu, const float *sigma, int64_t n, int32_t min_symbol,
                    int32_t max_symbol, int32_t seg_len, void *scratch, uint32_t *seg_bytes, uint64_t *seg_offsets, uint8_t *out,
                    int32_t *error_flag, void *stream);

/* inverse: bytes + seg_offsets[segments + 1] + the same mu, sigma -> symbols[n].  error_flag non-zero: corrupt stream
 * (3 a segment shorter than its 4 state bytes, 4 no symbol owns the slot, 5 a segment's bytes ran out, 6 a segment did not end
 * with every byte used and the coder back at its initial state 2^23; the encoder's codes are 1 symbol outside the range, 2 zero frequency).
 * `bytes` must be readable up to 16 bytes past seg_offsets[segments] (the kernel reads the stream in aligned 16-byte pieces).
 * `scratch`: gsvc_ans_decode_scratch_bytes(n, seg_len) bytes, 16-byte aligned: the part of the model that does not depend on
 * the coder state (the cumulative frequencies of every symbol's mode) is computed by a chip-wide parallel kernel first and laid
 * out so that the serial per-segment lanes of the decode kernel read it as one coalesced stream. */
int64_t gsvc_ans_decode_scratch_bytes(int64_t n, int32_t seg_len);
int gsvc_ans_decode(const uint8_t *bytes, const uint64_t *seg_offsets, const float *mu, const float *sigma, int64_t n,
                    int32_t min_symbol, int32_t max_symbol, int32_t seg_len, int32_t *symbols, int32_t *error_flag, void *scratch,
                    void *stream);

/* Per-anchor parameters of the batch's rows (reference ortho_gaussian_renderer/guassian.py:160-176 + the getters of
 * scene/gaussian_model.py:641-700), v = vis[row]: feat = anchor_feat[v] [rows,F], offsets = offset[v] [rows,3K], scaling =
 * exp(scaling_p[v]) [rows,S], mask = straight-through (sigmoid(mask_p[v]) > 0.01) [rows,K]; decoded != 0: the stored values as
 * they are.  F, K or S may be 0 (that group is left out: its pointers are not read).  Backward ADDS into the dense, caller-zeroed
 * d_* (an anchor is visible in several renders); g_* may be NULL. */
int gsvc_gather_rows_forward(const float *feat_p, const float *offset_p, const float *scaling_p, const float *mask_p,
                             const int64_t *vis, int64_t rows, int32_t F, int32_t K, int32_t S, int32_t decoded, float *feat,
                             float *offsets, float *scaling, float *mask, void *stream);
int gsvc_gather_rows_backward(const float *scaling_p, const float *mask_p, const int64_t *vis, int64_t rows, int32_t F, int32_t K,
                              int32_t S, int32_t decoded, const float *g_feat, const float *g_offsets, const float *g_scaling,
                              const float *g_mask, float *d_feat, float *d_offset, float *d_scaling, float *d_mask, void *stream);
/* The same gradients without atomics (and without a zero fill: every element of the d_* tensors is written), for rows that
 * are the concatenation of R ascending index lists over A anchors: seen [R*A] (1 = view r holds anchor a), rank [R*A] =
 * inclusive scan of seen (rank - 1 = the row), R <= 8.  Sums in view order: deterministic. */
int gsvc_gather_rows_backward_ranked(const float *scaling_p, const float *mask_p, const uint8_t *seen, const int64_t *rank, int32_t R,
                                     int64_t A, int32_t F, int32_t K, int32_t S, int32_t decoded, const float *g_feat,
                                     const float *g_offsets, const float *g_scaling, const float *g_mask, float *d_feat,
                                     float *d_offset, float *d_scaling, float *d_mask, void *stream);

/* Masks of a fitting step's plan in one pass over the A anchors: visible_host[r] = view r's visibility mask (bytes, 0 / 1),
 * M [R*A] = the masks side by side, present [A] = some view holds the anchor, chosen [R*A] (may be NULL: then mask_raw / u are
 * not read) = visible & live & (u <= rate), live = an offset mask of the anchor is on (mask_raw [A,K]: sigmoid(.) > 0.01, or the
 * stored 0 / 1 values when decoded; reference scene/gaussian_model.py get_mask_anchor), u [R*A] uniform draws of the caller. */
int gsvc_plan_masks(const uint8_t *const *visible_host, int32_t R, int64_t A, const float *mask_raw, int32_t K, int32_t decoded,
                    const float *u, float rate, uint8_t *M, uint8_t *present, uint8_t *chosen, void *stream);
/* The three quant_step networks of the EntropyParamsNets (reference scene/gaussian_model.py:198-232: Linear(in -> hidden), GELU,
 * Linear(hidden -> 1), evaluated at :1569-1597) on the same input rows X [M, in] in ONE launch each way (instantiated for
 * 192 -> 50 -> 1; other widths: GSVC_E_UNSUPPORTED, the caller keeps the layer kernels).  forward: z[i] [M, hidden] = the first
 * layer's pre-activation, a[i] = GELU(z[i]) (the operands of the backward and of the weight gradients), q[i] [M] = the raw output.
 * backward: dz[i] [M, hidden] = dq[i] W2_i GELU'(z[i]) (dq[i] NULL = zeros) and dX [M, in] = sum_i dz[i] W1_i; the weight
 * gradients are the products dz[i]^T X, dq[i]^T a[i] (gsvc_linear_wgrad_*). */
typedef struct gsvc_quant_step_net {
    const float *W1, *b1; /* [hidden][in], [hidden] */
    const float *W2, *b2; /* [1][hidden], [1] */
} gsvc_quant_step_net;
int gsvc_quant_step_nets_forward(const gsvc_quant_step_net *nets3, const float *X, int64_t M, int32_t in_dim, int32_t hidden,
                                 float *const *z3, float *const *a3, float *const *q3, void *stream);
int gsvc_quant_step_nets_backward(const gsvc_quant_step_net *nets3, const float *const *z3, const float *const *dq3, int64_t M,
                                  int32_t in_dim, int32_t hidden, float *const *dz3, float *dX, void *stream);

/* Per-row quantisation steps: out3 [3, rows], out3[g][i] = q_g adj_g[ctx_row ? ctx_row[i] : i] for the features, scalings and
 * offsets (reference gaussian_renderer/guassian.py:250-262, Q * Q_adj of the entropy context; ctx_row maps a row to its row of a
 * context evaluated once per distinct anchor).  raw != 0: adj_g holds the quant_step networks' raw outputs q and the adjustment
 * exp(clamp(q, -10, 10)) (reference scene/gaussian_model.py:1586-1596) is applied here.
 * backward: grad_adj3 [3, D] = scatter-add of q_g g_g[i] (any g_g may be NULL), times adj_g [|q| <= 10] when raw (the gradient
 * w.r.t. the raw outputs; adj_* are read only then). */
int gsvc_q_rows_forward(const float *adj_feat, const float *adj_scaling, const float *adj_offsets, const int64_t *ctx_row,
                        float q_feat, float q_scaling, float q_offsets, int64_t rows, int32_t raw, float *out3, void *stream);
int gsvc_q_rows_backward(const float *g_feat, const float *g_scaling, const float *g_offsets, const int64_t *ctx_row, float q_feat,
                         float q_scaling, float q_offsets, int64_t rows, int64_t D, const float *adj_feat, const float *adj_scaling,
                         const float *adj_offsets, int32_t raw, float *grad_adj3, void *stream);

/* Scans and compactions of a step plan in three launches.  view_masks [R, A] (bytes, 0 / 1), chosen [R, A] (a subset of
 * view_masks: the rate sample, or NULL), present [A] (the union of the views).  Outputs: scan [R A] = inclusive scan of the
 * flattened view masks (row of (view, anchor) in the concatenated rows + 1); flat = the anchors (position mod A) at the set
 * positions of view_masks in order — the views' visible-anchor lists one after the other (capacity R A); sel_rows = scan - 1 at the chosen positions (capacity R A); pos [A] = inclusive scan of present - 1; distinct =
 * the set positions of present (capacity A); counts [R + 2]: the scan at each view's end, the chosen pairs, the distinct anchors. */
int64_t gsvc_plan_scans_scratch_bytes(int32_t R, int64_t A);
int gsvc_plan_scans(const uint8_t *view_masks, const uint8_t *chosen, const uint8_t *present, int32_t R, int64_t A, void *scratch,
                    int64_t *scan, int64_t *flat, int64_t *sel_rows, int64_t *pos, int64_t *distinct, int64_t *counts, void *stream);

/* Row maps for FiLM rows shared by the opposite views of a frame (views 2 f and 2 f + 1 of R have the same camera z, hence the
 * same condition per anchor: reference frame_cube/frame.py:18-43, gaussian_renderer/guassian.py:225-230).  vis [rows]: anchor of
 * every chain row (views concatenated, row_bounds_host [R + 1]); pos [A]: anchor -> index in the list distinct [D] of the anchors
 * some view sees; view_masks [R A] / scan [R A]: the flattened view masks and their inclusive scan.  Outputs: row_of [rows] =
 * (view / 2) D + pos[vis]; src_a / src_b [R / 2, D] = chain row of the anchor in view 2 f / 2 f + 1, or -1. */
int gsvc_film_row_maps(const int64_t *vis, const int64_t *row_bounds_host, int32_t R, const int64_t *pos, int64_t D, int64_t A,
                   const uint8_t *view_masks, const int64_t *scan, const int64_t *distinct, int32_t *row_of, int32_t *src_a,
                   int32_t *src_b, void *stream);

/* out [rows_u, C] = g[src_a[j], :] + g[src_b[j], :] per row j, a source of -1 counting as zeros: the gradient of the generators'
 * outputs computed once per (frame, anchor) from the gradients of the frame's two opposite views (FULL_PRECISION / STE_ENTROPY
 * steps: both views see the same Gaussians, reference gaussian_renderer/guassian.py:225-273 evaluates the networks per view);
 * src_a / src_b as gsvc_film_row_maps writes them.  A gather per output row: no atomics, a fixed order of the two terms. */
int gsvc_pair_rows_sum(const float *g, const int32_t *src_a, const int32_t *src_b, int64_t rows_u, int32_t C, float *out, void *stream);

/* Deterministic mode (GSVC_DETERMINISTIC=1 through gsvc_amd.switches; SURVEY section 5 "deterministic-mode switch for bwd atomics").
 * gsvc_set_deterministic(1): the launches whose float sums depend on the order workgroups retire in take a fixed-order form —
 * the hash-grid backward gives every (level, table slice) to ONE workgroup (its 64-bit fixed-point LDS sums are exact, the single
 * float add per table word is the only rounding), and the host routes every scatter-add of rows through gsvc_segment_rows_sum:
 * dst[sorted_idx[p]][c] (= or +=, `accumulate`) the sum over the run of equal targets starting at p of src[order[j]][c], j in list
 * order (order = a STABLE argsort of the rows' targets, sorted_idx the targets in that order).  Replaces the float atomics of
 * reference-shaped scatter-adds (utils/entropy_models.py:159-175's gradient, the index_add of guassian.py:160-176's gathers). */
int gsvc_set_deterministic(int on);

int gsvc_segment_rows_sum(const float *src, const int64_t *order, const int64_t *sorted_idx, int64_t n, int32_t C, float *dst,
                          int32_t accumulate, void *stream);

/* out[scan[i] - 1] = (value ? value[i] + value_bias : i) for every i with mask[i] != 0, `scan` = inclusive scan of the mask
 * (int64): the index lists of the step plan in one elementwise pass each; entries of `out` past the count are not written. */
int gsvc_compact_by_scan(const uint8_t *mask, const int64_t *scan, const int64_t *value, int64_t value_bias, int64_t n, int64_t *out,
                         void *stream);

/* Means of three whole parameter tensors in one pass (the x_mean terms of the rate's clamp bounds: reference
 * utils/entropy_models.py EntropyGaussian.forward, x_mean = mean of the full attribute tensor): out3 = (mean(feat),
 * mean(scaling_exp ? exp(scaling) : scaling), mean(offset)).  scratch: gsvc_param_means_scratch_floats() floats.  Fixed order. */
int64_t gsvc_param_means_scratch_floats(void);
int gsvc_param_means(const float *feat, int64_t n_feat, const float *scaling, int64_t n_scaling, int32_t scaling_exp,
                     const float *offset, int64_t n_offset, float *scratch, float *out3, void *stream);

/* Tail of an EntropyParamsNet (reference scene/gaussian_model.py:1586-1596): params [n,2C] = [mean | scale], q [n] ->
 * mean [n,C], scale = max(scale, 1e-9) [n,C], adj = exp(clamp(q, -10, 10)) [n]; backward -> dparams [n,2C], dq [n]. */
int gsvc_ctx_post_forward(const float *params, const float *q, int64_t n, int32_t C, float *mean, float *scale, float *adj,
                          void *stream);
int gsvc_ctx_post_backward(const float *params, const float *q, const float *adj, int64_t n, int32_t C, const float *g_mean,
                           const float *g_scale, const float *g_adj, float *dparams, float *dq, void *stream);

/* FiLM of the generator networks (reference scene/gaussian_model.py:150-166) over n = rows * features elements (a multiple
 * of 4, 16-byte aligned tensors): y = gamma * h + beta; backward of the product: dgamma = g * h, dh = g * gamma. */
int gsvc_film_forward(const float *gamma, const float *h, const float *beta, float *y, int64_t n, void *stream);
int gsvc_film_backward(const float *g, const float *h, const float *gamma, float *dgamma, float *dh, int64_t n, void *stream);

/* Conditioning input of the generator / deformation MLPs for the concatenated rows of `renders` (<= 16) views (reference
 * ortho_gaussian_renderer/guassian.py:225-230, utils/time_util.py:7-55): pe[row] = [embed(cam_z[r]) | embed(anchor[row].z -
 * cam_z[r])] for the rows row_bounds[r] <= row < row_bounds[r + 1]; embed(x) = [x, sin(2^k x), cos(2^k x)]_{k < freqs}.
 * anchor: [rows, 3]; pe: [rows, 2 * (2 * freqs + 1)].  row_bounds / cam_z are host arrays. */
int gsvc_embed_pe(const float *anchor, const int64_t *row_bounds, const float *cam_z, int32_t renders, int32_t freqs, float *pe,
                  void *stream);

/* Several streams in one launch (each job as gsvc_ans_decode): a coded model is dozens of streams of a few waves each; one
 * launch lasts as long as a lane's seg_len serial symbols whatever the number of streams it carries. */
typedef struct gsvc_ans_decode_job {
    const uint8_t *bytes;
    const uint64_t *seg_offsets;
    const float *mu, *sigma;
    int64_t n;
    int32_t min_symbol, max_symbol, seg_len;
    int32_t *symbols, *error_flag;
    void *scratch;
} gsvc_ans_decode_job;
int gsvc_ans_decode_many(const gsvc_ans_decode_job *jobs, int32_t n_jobs, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Linear layers of the generator / deformation / entropy-parameter MLPs (reference scene/gaussian_model.py:
 * 150-232: every nn.Linear applied to the [anchors, features] matrix)
 * ---------------------------------------------------------------------------------------------------- */

/* Y[M,N] = X[M,K] W[N,K]^T + bias[N] (bias may be NULL; torch.nn.Linear layout), fp32 MFMA, weight matrix resident
 * in LDS and X streamed through registers: K, N <= 192 (GSVC_E_UNSUPPORTED beyond).
 * w_in_out != 0: W is [K][N] (input-major), so Y = X W — the backward's dX = G W without a transposed copy.
 * relu != 0: Y = max(Y, 0) fused into the store (the Linear -> ReLU pairs of the reference's nn.Sequential MLPs). */
int gsvc_linear_forward(const float *X, const float *W, const float *bias, float *Y, int64_t M, int32_t K, int32_t N,
                        int32_t w_in_out, int32_t relu, void *stream);

/* The same product with an epilogue program (the activations of the MLPs ride on the GEMM that produces their operand;
 * gsvc_amd/mlp.py runs every network of scene/gaussian_model.py:150-232 as one chain of these calls).  aux1 / aux2 / Y2 / Y3
 * have Y's shape [M,N]; v = X W^T + bias:
 *   GSVC_LIN_NONE / _RELU       as gsvc_linear_forward
 *   GSVC_LIN_GELU_DUAL          Y = v (the pre-activation the backward needs), Y2 = GELU(v) (exact, erf form)
 *   GSVC_LIN_TANH / _SIGMOID    Y = tanh(v) / sigmoid(v)
 *   GSVC_LIN_MUL_GELU_GRAD      Y = v * GELU'(aux1)            (dX of a layer behind a GELU: aux1 = its pre-activation)
 *   GSVC_LIN_MUL_RELU_MASK      Y = aux1 > 0 ? v : 0           (dX of a layer behind a ReLU: aux1 = its output)
 *   GSVC_LIN_FILM               Y = v (gamma), Y2 = v * aux1 + aux2          (FiLM: aux1 = h, aux2 = beta)
 *   GSVC_LIN_FILM_GRAD          Y = v (d beta), Y2 = v * aux1 (d gamma, aux1 = h), Y3 = v * aux2 (d h, aux2 = gamma)
 *   GSVC_LIN_ADD                Y = v + aux1 (aux1 may be Y itself: the input gradients of several networks that read the same
 *                               matrix — the six entropy sub-networks all read the hash-grid feature — accumulate in place) */
enum {
    GSVC_LIN_NONE = 0, GSVC_LIN_RELU = 1, GSVC_LIN_GELU_DUAL = 2, GSVC_LIN_TANH = 3, GSVC_LIN_SIGMOID = 4,
    GSVC_LIN_MUL_GELU_GRAD = 5, GSVC_LIN_MUL_RELU_MASK = 6, GSVC_LIN_FILM = 7, GSVC_LIN_FILM_GRAD = 8, GSVC_LIN_ADD = 9
};
int gsvc_linear_forward_ex(const float *X, const float *W, const float *bias, float *Y, int64_t M, int32_t K, int32_t N,
                           int32_t w_in_out, int32_t epilogue, const float *aux1, const float *aux2, float *Y2, float *Y3,
                           void *stream);

/* Y[M,N] = sum_p X_p[M,K_p] W_p with W_p given [K_p][N] (input-major: the dX = G W products of a backward pass whose input
 * gradients meet in one matrix — the six sub-networks of the three EntropyParamsNets all read the hash-grid feature, reference
 * scene/gaussian_model.py:198-232, 1569-1597) in ONE launch: a wave keeps its rows' accumulators in registers across the
 * products and stores the sum once.  At most 8 products, N, K_p <= 192, M <= 65536 (GSVC_E_UNSUPPORTED beyond: use
 * gsvc_linear_forward_ex with GSVC_LIN_ADD product by product). */
typedef struct {
    const float *X;      /* [M][K] */
    const float *W;      /* [K][N] */
    int32_t K;
    int32_t pad;
} gsvc_accum_job;
int gsvc_linear_accumulate_many(const gsvc_accum_job *jobs, int32_t n_jobs, float *Y, int64_t M, int32_t N, void *stream);

/* The forward counterpart: several layers that read the SAME input, Y_p[M,N_p] = X[M,K] W_p^T + b_p with W_p [N_p][K] as nn.Linear
 * stores it; Y2_p != NULL: Y_p keeps the pre-activation and Y2_p = GELU(Y_p) (the GSVC_LIN_GELU_DUAL pair).  One launch: a wave
 * reads its rows' fragments once and keeps them across the products.  At most 8 products, N_p <= 160, K <= 192 and a multiple
 * of 4, M <= 65536 (GSVC_E_UNSUPPORTED beyond: gsvc_linear_forward_ex layer by layer). */
typedef struct {
    const float *W;      /* [N][K] */
    const float *bias;   /* [N] or NULL */
    float *Y, *Y2;       /* [M][N]; Y2 may be NULL */
    int32_t N;
    int32_t pad;
} gsvc_shared_input_job;
int gsvc_linear_forward_shared_input(const float *X, int64_t M, int32_t K, const gsvc_shared_input_job *jobs, int32_t n_jobs,
                                     void *stream);

/* dW[N,K] = G[M,N]^T X[M,K] and (db != NULL) db[N] = column sums of G: the weight / bias gradients of the same
 * layers.  Rows are split over the chip instead of the tiny output; every workgroup writes its partial sums to its
 * slot of `workspace` ((N*K + N) floats per slot, gsvc_linear_wgrad_workspace() = 256 slots) and a second small
 * kernel adds the slots, so the result is deterministic (no atomics).  K, N <= 192. */
int64_t gsvc_linear_wgrad_workspace(int32_t N, int32_t K);
int gsvc_linear_wgrad(const float *G, const float *X, float *dW, float *db, int64_t M, int32_t N, int32_t K,
                      float *workspace, int64_t workspace_floats, void *stream);

/* The two halves of gsvc_linear_wgrad apart, so that one small launch adds up the partial sums of every layer of a network's
 * backward pass: _partial runs the row-split kernel only (workspace as above, one region per pending layer; *slots_used = the
 * slots it filled), _reduce_many adds the slots of n_jobs layers (db may be NULL when the partials were taken without it;
 * `partial` must then have been produced with want_db = 0). */
typedef struct gsvc_wgrad_reduce_job {
    const float *partial;
    float *dW, *db;
    int32_t slots, N, K;
} gsvc_wgrad_reduce_job;
int gsvc_linear_wgrad_partial(const float *G, const float *X, int32_t want_db, int64_t M, int32_t N, int32_t K,
                              float *workspace, int64_t workspace_floats, int32_t *slots_used, void *stream);
int gsvc_linear_wgrad_reduce_many(const gsvc_wgrad_reduce_job *jobs, int32_t n_jobs, void *stream);
/* The partial sums of n_jobs products at once: products of the usual shapes share launches (up to 8 per launch, the workgroups
 * dealt to them by their MFMA work: the weight gradients of a whole network over the same rows), anything else is launched alone.
 * Every job names its own workspace region; slots_used is written per job (the `slots` of its reduce job). */
typedef struct gsvc_wgrad_partial_job {
    const float *G, *X;
    float *workspace;
    int64_t M, workspace_floats;
    int32_t want_db, N, K;
    int32_t slots_used;      /* out */
} gsvc_wgrad_partial_job;
int gsvc_linear_wgrad_partial_many(gsvc_wgrad_partial_job *jobs, int32_t n_jobs, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Whole-network chain kernels of the generator and deformation MLPs (csrc/mlp_chain.hip): a 16-row block's activations stay
 * in registers from the network's input to its output; weights resident in LDS; fp32 MFMA.
 * Replaces, per anchor row: GeneratorNet.forward = out_act(out_linear(film(linear2(GELU(linear1(feature))), condition)))
 * with FiLM = gamma(c) * x + beta(c), gamma / beta = fc_*1(ReLU(fc_*0(c))) (reference scene/gaussian_model.py:150-196, used at
 * ortho_gaussian_renderer/guassian.py:251-262), and mlp_deform = 5 x Linear with GELU between (scene/gaussian_model.py:468-489,
 * guassian.py:264-273) on cat([feature, condition]).  All matrices row-major fp32, weights in torch.nn.Linear layout [out, in],
 * every pointer 16-byte aligned.  Instantiated widths: feature 50, condition 66, hidden 100, outputs 10 / 30 / 70 (generators)
 * and 30 (deform); anything else returns GSVC_E_UNSUPPORTED (callers keep the gsvc_linear_* layer path).
 * The condition receives no gradient (it is the positional embedding of detached anchor positions / the frame time).
 * out_act: 0 identity, 1 tanh, 2 sigmoid. */
typedef struct gsvc_generator_net {
    const float *W1, *b1, *W2, *b2, *W3, *b3;                             /* linear1, linear2, out_linear */
    const float *Wg0, *bg0, *Wg1, *bg1, *Wb0, *bb0, *Wb1, *bb1;           /* film.fc_gamma0/1, film.fc_beta0/1 */
    int32_t feat_dim, cond_dim, hidden_dim, out_dim, out_act;
} gsvc_generator_net;
typedef struct gsvc_generator_grads {
    float *W1, *b1, *W2, *b2, *W3, *b3, *Wg0, *bg0, *Wg1, *bg1, *Wb0, *bb0, *Wb1, *bb1;
} gsvc_generator_grads;
/* Shared FiLM rows.  gamma / beta depend on the condition only, and the two opposite views of a frame (the training step renders
 * both: reference pipeline/train.py:353-387) have the same condition for the same anchor — same camera z, same anchor z — while
 * their features differ (independent quantisation noise per render).  With a gsvc_film_rows the FiLM networks (4 of a
 * generator's 7 layers, forward, backward and weight gradients) run once per (frame, anchor) instead of once per (view, anchor):
 *   rows      number of FiLM rows;  cond [rows, cond_dim] their condition
 *   row_of    [M] int32: chain row (view, anchor) -> its FiLM row
 *   src_a/_b  [rows] int32: the (up to) two chain rows of a FiLM row, -1 = that view does not see the anchor
 * Precondition: every chain row r is named exactly once, by src_a[row_of[r]] or by src_b[row_of[r]] (gsvc_film_row_maps leaves the
 * maps so).  The backward relies on it: with shared rows k_trunk_bwd walks the FiLM rows and takes the two chain rows behind each
 * one through the chain together (a chain row nobody names gets no gradient written, one named twice is written twice), hands the
 * FiLM networks the two views' SUMMED d gamma / d beta, one row per FiLM row, and the scratch holds no per-view rows of them:
 * gsvc_generator_scratch_floats is (out + 2 hidden) M + (2 cond + 2 hidden) rows floats + the weight gradients' partial sums.
 * src_a / src_b increase within a view, so the gathered accesses stay nearly contiguous.
 * NULL (or rows = 0): one FiLM row per chain row, conditions = cond.  The sizes below take the FiLM row count (0 = M). */
typedef struct gsvc_film_rows {
    int64_t rows;
    const float *cond;
    const int32_t *row_of, *src_a, *src_b;
} gsvc_film_rows;
int64_t gsvc_generator_saved_floats(const gsvc_generator_net *net, int64_t M, int64_t film_rows);
int64_t gsvc_generator_scratch_floats(const gsvc_generator_net *net, int64_t M, int64_t film_rows);
int64_t gsvc_generator_inference_floats(const gsvc_generator_net *net, int64_t M, int64_t film_rows);

typedef struct gsvc_deform_net {
    const float *W[5], *b[5];                                             /* mlp_deform's five Linear layers, input = [feat | cond] */
    int32_t feat_dim, cond_dim, hidden_dim, out_dim;
} gsvc_deform_net;
typedef struct gsvc_deform_grads {
    float *W[5], *b[5];
} gsvc_deform_grads;
int64_t gsvc_deform_saved_floats(const gsvc_deform_net *net, int64_t M);
int64_t gsvc_deform_scratch_floats(const gsvc_deform_net *net, int64_t M);
int64_t gsvc_deform_inference_floats(const gsvc_deform_net *net, int64_t M);

/* A generation pass: n_nets (1 .. 3) generators and the deformation network on the same (feat, cond) rows, one call each way.
 * The generators share ONE pair of launches each way (workgroup b serves network b % n_nets: one prologue and one partial last
 * round for all of them).
 * gsvc_generate_all_forward: saved / y are arrays of n_nets + 1 pointers, the deformation network last; y[i] is [M, out].  Launch
 *   order on `stream`: k_film_nets_fwd, k_trunk_fwd, k_deform_a_fwd, k_deform_b_fwd.  keep_for_backward != 0: saved[i] (caller-owned,
 *   gsvc_*_saved_floats floats) receives what the backward reads.  keep_for_backward == 0 (the decoder's render loop, evaluation):
 *   the same kernels with every store the backward alone would read left out; saved[i] is then the small scratch of
 *   gsvc_*_inference_floats (gamma / beta of the FiLM networks; the deformation network's second activation).
 * gsvc_generate_all_backward: from gy (n_nets + 1 pointers, [M, out] each; y: the n_nets generators' outputs) forms the feature
 *   gradient and every weight / bias gradient (dW = G^T X by the row-split kernels of gsvc_linear_wgrad_partial + one batched slot
 *   reduce per network kind: deterministic, no atomics) into the pointers of gen_grads[i] / deform_grads (a NULL weight pointer skips
 *   that layer).  gfeat_parts[i] [M, feat] receives generator i's feature gradient (distinct buffers, written, not accumulated);
 *   the deformation kernel adds them to its own in the pass that writes gfeat_sum [M, feat] (the feature matrix feeds all the
 *   networks).  `scratch`: the generators' regions back to back (sum of gsvc_generator_scratch_floats, each rounded up to a multiple
 *   of 4 floats); `scratch_deform`: gsvc_deform_scratch_floats floats.
 *   wgrad_stream == NULL: everything on `stream`, in this order: k_trunk_bwd, k_film_nets_bwd, the generators' partial and reduce
 *   launches, k_deform_b_bwd, k_deform_a_bwd, the deformation network's partial and reduce launches, the two strided copies that
 *   interleave its first layer's halves.  scratch_deform may alias scratch (the larger of the two sizes).
 *   wgrad_stream != NULL: the four chain kernels go on `stream` first (a chain workgroup needs its whole CU: a product queued in
 *   between makes the second network's chain kernels wait for it), one event is recorded behind them, wgrad_stream waits for it
 *   and carries the generators' products and reduce, the deformation network's, then the copies — so `stream` can go on with the
 *   feature gradient while they run.  The generators' products still read `scratch` when the deformation network's chain kernels
 *   write `scratch_deform`: an overlap of the two is refused (GSVC_E_INVALID, nothing launched; M == 0 returns before any buffer
 *   is looked at).  If the event cannot be made, recorded or waited for, the products go on `stream` instead: still ordered, not
 *   overlapped.  The caller owns the remaining hazards: the products read feat, cond (the FiLM rows' condition), saved, both
 *   scratches and gy of the deformation network, and write the gradient tensors, until wgrad_stream has passed; the optimizer's
 *   stream must wait for it.
 * No state is kept between calls: thread-safe per stream like every other entry. */
int gsvc_generate_all_forward(const gsvc_generator_net *nets, int32_t n_nets, const gsvc_deform_net *deform, const float *feat,
                              const float *cond, int64_t M, const gsvc_film_rows *film, float *const *saved, float *const *y,
                              int32_t keep_for_backward, void *stream);
int gsvc_generate_all_backward(const gsvc_generator_net *nets, int32_t n_nets, const gsvc_deform_net *deform, const float *feat,
                               const float *cond, int64_t M, const gsvc_film_rows *film, const float *const *saved, const float *const *y,
                               const float *const *gy, float *scratch, float *scratch_deform, float *gfeat_sum, float *const *gfeat_parts,
                               const gsvc_generator_grads *gen_grads, const gsvc_deform_grads *deform_grads, void *stream,
                               void *wgrad_stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Anchor geometry decode (the G-PCC tmc3 step of reference utils/encodings.py:780-826 decode_anchor; coder and bitstream are this
 * library's own: gsvc_amd/anchor_codec.py).  An occupancy octree over the integer anchor lattice, one 8-bit mask per node,
 * per level a static 12-bit model and an interleaved rANS stream (32-bit states, 16-bit words, symbol i in lane i % lanes).
 * gsvc_anchor_rans_decode: all levels' symbols in one launch (one workgroup per level); error: OR of 1 bad table, 2 truncated,
 * 4 the coder did not return to its initial state.  gsvc_octree_popcount / _expand: a level's masks -> the next level's nodes
 * (Morton keys; counts_inclusive_scan = inclusive scan of the popcounts; error |= 8 on an empty mask or more than `capacity`
 * children).  gsvc_morton_decode: keys (x at bit 3 b + 2, y at 3 b + 1, z at 3 b) -> xyz [n, 3].
 * ---------------------------------------------------------------------------------------------------- */
typedef struct gsvc_anchor_level {
    const uint32_t *states;     /* [lanes] */
    const uint16_t *words;      /* [n_words] */
    const uint16_t *freq;       /* [256], sum 4096 */
    uint8_t *out;               /* [n] decoded masks */
    int64_t n, n_words;
    int32_t lanes;
} gsvc_anchor_level;
int gsvc_anchor_rans_decode(const gsvc_anchor_level *levels_host, int32_t n_levels, int32_t *error, void *stream);
int gsvc_octree_popcount(const uint8_t *occ, int64_t n, int64_t *counts, void *stream);
int gsvc_octree_expand(const int64_t *nodes, const uint8_t *occ, const int64_t *counts_inclusive_scan, int64_t n, int64_t capacity,
                       int64_t *nodes_out, int32_t *error, void *stream);
int gsvc_morton_decode(const int64_t *keys, int64_t n, int64_t *xyz, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Decoder output: 8-bit frames from the float images of the render loop (replaces the clamp + ToPILImage of reference
 * utils/report_utils.py:439-445; csrc/frames_out.hip).  One launch converts n (1 .. 16) float32 images [3, H, W] (RGB, nominal
 * [0, 1], separate allocations, each base 4-byte aligned) into n frames; frame k starts at out + k * out_stride.
 *   per pixel   c = x > 0 ? x : 0; c = min(c, 1)            (NaN and -inf give 0, +inf gives 1)
 *   layout      GSVC_FRAMES_RGB24: interleaved [H, W, 3].  GSVC_FRAMES_YUV444P / _YUV420P: planar Y, U (Cb), V (Cr) with
 *               Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr)); 4:2:0 chroma is the plain mean of
 *               the 2x2 block taken in float before quantisation (centre siting), H and W even, H W 3 / 2 bytes = one I420 frame
 *   matrix      GSVC_FRAMES_BT709 (Kr 0.2126, Kb 0.0722) or GSVC_FRAMES_BT601 (0.299, 0.114); Kg = 1 - Kr - Kb; ignored for RGB24
 *   range       GSVC_FRAMES_LIMITED: Y8 = 16 + 219 Y, C8 = 128 + 224 C.  GSVC_FRAMES_FULL: Y8 = 255 Y, C8 = 128 + 255 C.
 *               RGB24 is always 255 c.  The result is clamped to [0, 255].
 *   rounding    GSVC_FRAMES_TRUNC: (uint8) v (what ToPILImage does to a float tensor).  GSVC_FRAMES_NEAREST: (uint8)(v + 0.5).
 * images_host: host array of n device pointers (they travel in the kernel arguments: no upload).  out_stride >= the frame's bytes;
 * bytes between frames are not written.  gsvc_frames_u8_bytes: bytes of one frame, < 0 for an invalid size or layout.
 * ---------------------------------------------------------------------------------------------------- */
#define GSVC_FRAMES_MAX_BATCH 16
enum { GSVC_FRAMES_RGB24 = 0, GSVC_FRAMES_YUV444P = 1, GSVC_FRAMES_YUV420P = 2 };
enum { GSVC_FRAMES_BT709 = 0, GSVC_FRAMES_BT601 = 1 };
enum { GSVC_FRAMES_LIMITED = 0, GSVC_FRAMES_FULL = 1 };
enum { GSVC_FRAMES_TRUNC = 0, GSVC_FRAMES_NEAREST = 1 };
int64_t gsvc_frames_u8_bytes(int32_t H, int32_t W, int32_t layout);
int gsvc_frames_to_u8(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix, int32_t range,
                      int32_t rounding, uint8_t *out, int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Encoder input: float images from 8-bit frames, the mirror image of gsvc_frames_to_u8 (replaces the per-file PIL load +
 * ToTensor of reference frame_cube/frame.py:141-152; csrc/frames_in.hip).  One launch converts n (1 .. 16) 8-bit frames of H x W —
 * frame k starts at in + k * in_stride, any alignment — into n float32 images [3, H, W] (RGB, separate allocations, each base 4-byte
 * aligned).  Sample codes are b, y8, cb8, cr8 in 0 .. 255; every float operation below is one float32 operation.
 *   layout      GSVC_FRAMES_RGB24, interleaved [H, W, 3]: c = b / 255, an IEEE float32 division (not a multiply by a reciprocal: 126 of
 *               the 256 codes differ between the two) = torch.uint8 -> float32 -> div(255).
 *               GSVC_FRAMES_YUV444P / _YUV420P, planar Y, U (Cb), V (Cr), the layouts of gsvc_frames_to_u8:
 *                 R = Y + 2 (1 - Kr) Cr,  B = Y + 2 (1 - Kb) Cb,  G = Y - (2 Kr (1 - Kr) / Kg) Cr - (2 Kb (1 - Kb) / Kg) Cb,
 *               each then clamped to [0, 1].  The four constants are formed in double on the host and rounded once to float; in the
 *               kernel R = fma(r_cr, Cr, Y), B = fma(b_cb, Cb, Y), G = fma(-g_cb, Cb, fma(-g_cr, Cr, Y)).
 *   matrix      GSVC_FRAMES_BT709 (Kr 0.2126, Kb 0.0722) or GSVC_FRAMES_BT601 (0.299, 0.114); Kg = 1 - Kr - Kb; ignored for RGB24
 *   range       GSVC_FRAMES_LIMITED: Y = (y8 - 16) / 219, C = (c8 - 128) / 224.  GSVC_FRAMES_FULL: Y = y8 / 255, C = (c8 - 128) / 255
 *               (divisions).  Ignored for RGB24.
 *   chroma      4:2:0 only; the chroma samples are centre sited (Y4M C420jpeg) and are upsampled on the CODES, before the affine map
 *               (exact in float32: every interpolated code is a multiple of 1/16 below 256).
 *               GSVC_FRAMES_CHROMA_NEAREST: each chroma sample serves its 2x2 block.
 *               GSVC_FRAMES_CHROMA_BILINEAR, per axis: luma column x = 2 j takes 0.25 c[j - 1] + 0.75 c[j], column x = 2 j + 1 takes
 *               0.75 c[j] + 0.25 c[j + 1], indices clamped to [0, W / 2 - 1]; rows likewise, so the 2-D weights are 9/16, 3/16, 3/16,
 *               1/16 (= bilinear interpolation at scale 2 with half-pixel centres, align_corners = False).
 * images_host: host array of n device pointers (they travel in the kernel arguments: no upload).  in_stride >= the frame's bytes
 * (gsvc_frames_u8_bytes); H and W even for 4:2:0.  Nothing synchronises; every element of the n images is written, nothing else.
 * ---------------------------------------------------------------------------------------------------- */
enum { GSVC_FRAMES_CHROMA_NEAREST = 0, GSVC_FRAMES_CHROMA_BILINEAR = 1 };
int gsvc_frames_from_u8(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                        int32_t range, int32_t chroma, float *const *images_host, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Decoder output, deep frames: planar YUV of d = 9 .. 16 bits per sample, every sample one little-endian 16-bit word
 * whose upper 16 - d bits are zero (ffmpeg's yuv420p10le, yuv444p12le, ...; Y4M's C420p10, C444p12, ...).  Everything not said here is
 * as in gsvc_frames_to_u8: n, the images, the clamp of the inputs, Y / Cb / Cr, the plane order Y, U, V, the 4:2:0 chroma mean taken in
 * float before quantisation, matrix, rounding.  A frame has twice the bytes of its 8-bit form.
 *   range       GSVC_FRAMES_LIMITED: the 8-bit expression with both constants scaled by 2^(d - 8),
 *                 Y_d = 2^(d - 8) (16 + 219 Y), C_d = 2^(d - 8) (128 + 224 C)
 *               (a scaling by a power of two: the float32 value is exactly 2^(d - 8) times the 8-bit kernel's).
 *               GSVC_FRAMES_FULL: Y_d = (2^d - 1) Y, C_d = 2^(d - 1) + (2^d - 1) C.
 *               The value is clamped to [0, 2^d - 1]; then (uint16) v (TRUNC) or (uint16)(v + 0.5) (NEAREST).
 * Refused with an error before any launch: GSVC_FRAMES_RGB24, a depth outside 9 .. 16, n outside 1 .. 16, an odd H or W for 4:2:0, a
 * frame base or an out_stride that is not a multiple of 2, out_stride below the frame's bytes.  Nothing synchronises.
 * gsvc_frames_bytes: bytes of one frame of the given depth: gsvc_frames_u8_bytes for depth 8, twice that for depth 9 .. 16; < 0 for
 * RGB24 with a depth other than 8, for any other depth and for an invalid size or layout.
 * ---------------------------------------------------------------------------------------------------- */
int64_t gsvc_frames_bytes(int32_t H, int32_t W, int32_t layout, int32_t depth);
int gsvc_frames_to_u16(const float *const *images_host, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix, int32_t range,
                       int32_t rounding, int32_t depth, uint8_t *out, int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Encoder input, deep frames: the mirror image of gsvc_frames_to_u16.  Sample codes y, cb, cr are the 16-bit words as
 * they are in the frame (a code above 2^d - 1 is NOT masked; the result clamps).  Everything not said here is as in
 * gsvc_frames_from_u8: n, the images, the three fused multiply-adds and the clamp, matrix, the chroma modes and their weights.
 *   range       GSVC_FRAMES_LIMITED: Y = (y - 16 2^(d - 8)) / (219 2^(d - 8)), C = (c - 2^(d - 1)) / (224 2^(d - 8)).
 *               GSVC_FRAMES_FULL:    Y = y / (2^d - 1),                        C = (c - 2^(d - 1)) / (2^d - 1).
 *               IEEE float32 divisions, as in the 8-bit kernel (for a limited-range 8-bit code times 2^(d - 8) the quotients are the
 *               same real numbers: the two kernels then give the same bits).
 *   chroma      4:2:0 chroma is upsampled on the codes with the weights of gsvc_frames_from_u8; still exact in float32 (16 bits of
 *               code and 4 bits of sixteenths are fewer than 24).
 * Refused with an error before any launch: GSVC_FRAMES_RGB24, a depth outside 9 .. 16, n outside 1 .. 16, an odd H or W for 4:2:0, a
 * frame base or an in_stride that is not a multiple of 2, in_stride below the frame's bytes (gsvc_frames_bytes).  Nothing synchronises;
 * every element of the n images is written, nothing else.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_frames_from_u16(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                         int32_t range, int32_t chroma, int32_t depth, float *const *images_host, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] The fitting step's distortion in the delivered domain: float Y'CbCr planes (csrc/yuv_loss.hip).
 *
 * A plane buffer of a picture of H x W in layout L (GSVC_FRAMES_YUV444P or _YUV420P; RGB24 has none) is one contiguous float32 array
 *     [ Y: H W | Cb: ch cw | Cr: ch cw ],   (ch, cw) = (H / 2, W / 2) for 4:2:0 (H and W even), (H, W) for 4:4:4,
 * gsvc_yuv_planes_floats(H, W, L) floats in all (< 0 for an invalid size or layout); as tensors, Y [1, H, W] and C [2, ch, cw].  Every
 * plane is on a nominal [0, 1]: Y is the Y of gsvc_frames_to_u8's formulas and a chroma plane is that formula's C + 0.5, so that the
 * constants of SSIM meet the value range they were chosen for.  Nothing is clamped (a clamp would cut the gradient):
 * gsvc_frames_to_u8 / _u16 differ from gsvc_yuv_planes_forward only by their clamp of the inputs, their range map and their rounding.
 *
 * gsvc_frames_planes: the ground truth straight from a file's sample codes.  n (1 .. 16) frames of depth 8 (bytes) or 9 .. 16
 * (little-endian 16-bit words), frame k at in + k * in_stride, into n plane buffers (planes_host: host array of n device pointers,
 * each 4-byte aligned):
 *     Y = (y - y_off) / y_scale,   C = (c - c_off) / c_scale + 0.5
 * with the constants of the range at that depth (LIMITED: 16, 219, 128, 224, each times 2^(d - 8); FULL: 0, 2^d - 1, 2^(d - 1),
 * 2^d - 1): one float32 subtraction (exact), one IEEE float32 division and, for chroma, one float32 addition.  No matrix enters and
 * there is no chroma upsampling: a chroma code becomes one chroma float.  Refused before any launch: RGB24, n outside 1 .. 16, a depth
 * outside 8 .. 16, an odd H or W for 4:2:0, in_stride below the frame's bytes (gsvc_frames_bytes), and for deep frames an odd base or
 * in_stride.  Every float of the n buffers is written, nothing else.
 *
 * gsvc_yuv_planes_forward: the render as planes.  img_f, img_b: float32 [3, H, W] RGB; img_b may be NULL.
 *     a = 0.5 (f + flip_W(b))            the two-view frame gsvc_ssim_l1_pair_forward forms on load; a = f when img_b is NULL
 *     Y  = fma(Kr, R, fma(Kg, G, Kb B))
 *     Cb = fma(B - Y, 1 / (2 (1 - Kb)), 0.5),   Cr = fma(R - Y, 1 / (2 (1 - Kr)), 0.5)
 * of a's channels; Kr, Kg = 1 - Kr - Kb, Kb and the two reciprocals are formed in double and rounded once to float.  4:2:0 chroma is
 * 0.25 ((c00 + c01) + (c10 + c11)) of the 2x2 block's Cb / Cr (c_rs = row r, column s), added in exactly that order: the same bits
 * for every launch shape and alignment.  avg_out (float32 [3, H, W], may be NULL) receives a.
 *
 * gsvc_yuv_planes_backward: the exact adjoint.  d_planes: the gradient (gY, gCb, gCr) in the plane-buffer layout.  Per pixel, with
 * q = 0.25 for 4:2:0 (gCb / gCr of the pixel's block) and 1 for 4:4:4, s_b = 1 / (2 (1 - Kb)), s_r = 1 / (2 (1 - Kr)):
 *     gB' = q gCb s_b,  gR' = q gCr s_r,  gY' = gY - gB' - gR'
 *     dR = Kr gY' + gR',  dG = Kg gY',  dB = Kb gY' + gB'
 * dL_dimg_f = 0.5 d and dL_dimg_b = 0.5 d at the flipped column; with dL_dimg_b = NULL, dL_dimg_f = d.  Every element of the outputs
 * given is written, nothing else.
 *
 * All pointers 4-byte aligned; the kernels take a vector path when W is a multiple of 4, H is even and every base is 16-byte
 * aligned, and give the same bits on either path.  Nothing synchronises.
 * ---------------------------------------------------------------------------------------------------- */
int64_t gsvc_yuv_planes_floats(int32_t H, int32_t W, int32_t layout);
int gsvc_frames_planes(const uint8_t *in, int64_t in_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t range,
                       int32_t depth, float *const *planes_host, void *stream);
int gsvc_yuv_planes_forward(const float *img_f, const float *img_b, int32_t H, int32_t W, int32_t layout, int32_t matrix,
                            float *planes_out, float *avg_out, void *stream);
int gsvc_yuv_planes_backward(const float *d_planes, int32_t H, int32_t W, int32_t layout, int32_t matrix, float *dL_dimg_f,
                             float *dL_dimg_b, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Video metrics on the codes (csrc/metrics.hip).
 *
 * gsvc_frames_sse: out[k, p] (uint64 [n, 3], 8-byte aligned) = the sum over the samples of plane p of frame k of (a - b)^2, a and b the
 * sample codes of the two frame buffers (frame k of a starts at a + k * a_stride, of b at b + k * b_stride), in exact integer
 * arithmetic: one squared difference is below 2^32, every sum is 64-bit.  The same bits in every run.
 *   layout      GSVC_FRAMES_RGB24 (depth 8 only): p = R, G, B, the sample index mod 3.  GSVC_FRAMES_YUV444P / _YUV420P: p = Y, U, V, the
 *               planes one after the other (H W samples, then twice H W, or twice H W / 4 for 4:2:0).
 *   depth       8: one byte per sample.  9 .. 16: one little-endian 16-bit word per sample, compared as it is (nothing is masked).
 * Refused with an error before any launch: an unknown layout, a depth outside 8 .. 16, rgb24 deeper than 8, an odd H or W for 4:2:0,
 * a stride below the frame's bytes (gsvc_frames_bytes), an odd base or stride for a deep format, a NULL pointer, n < 1.  Bytes
 * between frames are not read.  The call zeroes out on the stream and does not synchronise.
 *
 * gsvc_msssim: the per-scale means of multi-scale SSIM (Wang et al. 2003) of P pairs of planes of H x W; x, y: plane p starts at
 * base + p * plane_pitch samples, its row r at + r * row_pitch samples.
 *   samples     GSVC_SAMPLE_F32: v = the float.  GSVC_SAMPLE_U8 / _U16 (little-endian words): v = code / peak, one IEEE float32
 *               division (= torch's uint -> float32 -> div(peak)); peak = 2^d - 1 puts a d-bit code on [0, 1].
 *   window      g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, 11 taps, applied along the rows and along the columns WITHOUT padding:
 *               a scale of h x w has (h - 10) (w - 10) outputs.  For an output, with mu1 = g*x, mu2 = g*y (* = the 2-D window sum),
 *                 s1 = g*x^2 - mu1^2, s2 = g*y^2 - mu2^2, s12 = g*(x y) - mu1 mu2,     C1 = 0.01^2, C2 = 0.03^2 (data range 1)
 *                 cs = (2 s12 + C2) / (s1 + s2 + C2),   ssim = cs (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)
 *               (the kernel takes the moments of x - cx, y - cy, cx and cy one pixel of the workgroup's tile: the same real numbers).
 *   scales      5; scale k + 1 is the 2x2 mean of scale k, h' = (h + 1) / 2: an odd side gets ONE leading zero row / column — its first
 *               window covers the indices -1 and 0 — and the divisor stays 4.
 *   out         double [5, P]: out[k, p] = the mean of cs over the outputs of scale k for k = 0 .. 3 and of ssim for k = 4, not
 *               clipped.  (MS-SSIM = the product over k of max(out[k], 0)^w[k], w = 0.0448, 0.2856, 0.3001, 0.2363, 0.1333: the
 *               caller's, in float64.)  A tile of 32 x 32 outputs sums in float32; the tiles of a (scale, plane) are added in a fixed
 *               order in double: the same bits in every run.
 * workspace: gsvc_msssim_workspace_bytes(P, H, W) bytes (the pooled pictures of both inputs and the tile sums; < 0 for a shape
 * gsvc_msssim refuses), 16-byte aligned, the caller's.  Refused with an error before any launch: a side of 160 or less (the last
 * scale would have fewer than 11 rows or columns), P outside 1 .. 65535, an unknown sample type, a row pitch below W, a plane pitch
 * below (H - 1) row_pitch + W (P > 1), a base not aligned to its sample type, a NULL pointer.  Nothing synchronises.
 * ---------------------------------------------------------------------------------------------------- */
enum { GSVC_SAMPLE_F32 = 0, GSVC_SAMPLE_U8 = 1, GSVC_SAMPLE_U16 = 2 };
int gsvc_frames_sse(const uint8_t *a, int64_t a_stride, const uint8_t *b, int64_t b_stride, int32_t n, int32_t H, int32_t W,
                    int32_t layout, int32_t depth, uint64_t *out, void *stream);
int64_t gsvc_msssim_workspace_bytes(int32_t P, int32_t H, int32_t W);
int gsvc_msssim(const void *x, int64_t x_row_pitch, int64_t x_plane_pitch, const void *y, int64_t y_row_pitch, int64_t y_plane_pitch,
                int32_t P, int32_t H, int32_t W, int32_t sample_type, float peak, void *workspace, double *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] MS-SSIM + L1 as a fitting loss (csrc/msssim_loss.hip).
 *
 * Over P planes of H x W float32 samples (contiguous, [P, H, W]): x the fitted picture, gt the ground truth.
 *   out[0]      the mean over the planes of prod_k max(t[k], 0)^w[k], t[k] the per-scale means of gsvc_msssim (same window, same
 *               pooling, same weights; float64, tile sums added in a fixed order), rounded to float32 once
 *   out[1]      the mean of |x - gt| over all P H W samples
 * img_b != NULL is the pair form: x = (img + flip_W(img_b)) / 2, formed on load; avg_out (may be NULL; pair form only) receives x.
 * keep_maps != 0 stores what gsvc_msssim_loss_backward reads (three maps over the valid outputs of every scale); with 0 the call is
 * a measurement and the workspace must not be handed to the backward.
 *
 * gsvc_msssim_loss_backward: d_img = grads[0] d out[0] / d x + grads[1] d out[1] / d x (grads: two floats on the device), from the
 * workspace a forward with keep_maps != 0 left and the same images.  Pair form: d_img = half of that, d_img_b = flip_W(d_img); img_b
 * and d_img_b go together.  gt gets no gradient.  A plane with any t[k] <= 0 has value 0 and an MS-SSIM gradient of exactly 0.  Every
 * pixel has one owner and every sum a fixed order: two runs give the same bits.
 *
 * workspace: gsvc_msssim_loss_workspace_bytes(P, H, W) bytes (< 0 for a shape the calls refuse), 16-byte aligned, the caller's, and
 * untouched between a forward and its backward.  Refused with an error before any GPU call: a NULL pointer, a side of 160 or less or
 * above 32768, P outside 1 .. 65535, an image not 4-byte aligned, a workspace not 16-byte aligned.  Nothing synchronises.
 * ---------------------------------------------------------------------------------------------------- */
int64_t gsvc_msssim_loss_workspace_bytes(int32_t P, int32_t H, int32_t W);
int gsvc_msssim_loss_forward(const float *img, const float *img_b, const float *gt, int32_t P, int32_t H, int32_t W, int32_t keep_maps,
                             void *workspace, float *out, float *avg_out, void *stream);
int gsvc_msssim_loss_backward(const float *img, const float *img_b, const float *gt, int32_t P, int32_t H, int32_t W, void *workspace,
                              const float *grads, float *d_img, float *d_img_b, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Picture hash on the codes (csrc/picture_hash.hip): what the PHSH section of a bitstream file holds.
 *
 * gsvc_picture_hash: out[k, p] (uint64 [n, 3], 8-byte aligned) = the hash of plane p of frame k of a buffer of delivered frames (frame
 * k starts at frames + k * stride).  With s the 0-based raster index of a sample within its plane and c its code, all in uint32
 * (wrapping):
 *     x = s * 0x9E3779B1 ^ (c + 1) * 0x85EBCA6B;   x ^= x >> 15;   x *= 0x2C1B3C6D;   x ^= x >> 12
 *     out[k, p] = the sum of x over the samples of the plane, modulo 2^64
 * A sum of integers: the same bits in every run and for every launch shape; it depends on where a sample sits, not only on the
 * multiset of codes.
 *   layout      GSVC_FRAMES_RGB24 (depth 8 only): p = R, G, B, the sample index mod 3, and s = the pixel index.  GSVC_FRAMES_YUV444P /
 *               _YUV420P: p = Y, U, V, the planes one after the other (H W samples, then twice H W, or twice H W / 4 for 4:2:0).
 *   depth       8: one byte per sample.  9 .. 16: one little-endian 16-bit word per sample, hashed as it is (nothing is masked).
 * Refused with an error before any launch: an unknown layout, a depth outside 8 .. 16, rgb24 deeper than 8, an odd H or W for 4:2:0,
 * a stride below the frame's bytes (gsvc_frames_bytes), an odd base or stride for a deep format, a NULL pointer, n < 1.  Bytes
 * between frames are not read.  The call zeroes out on the stream and does not synchronise.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_picture_hash(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                      uint64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Per-plane code histograms of delivered frames (csrc/scene.hip): what the scene-cut detector reads.
 *
 * gsvc_frames_histogram: out[k, p, b] (uint32 [n, 3, 256], 4-byte aligned) = the number of samples of plane p of frame k of a buffer of
 * delivered frames (frame k starts at frames + k * stride) whose code c falls in bin
 *     b = min(c >> (depth - 8), 255)
 * The min keeps a deep sample with bits above its depth inside the 256 bins (it counts in bin 255).  The bins of a plane add up to
 * the plane's samples (at most 2^30).  Sums of integers: the same bits in every run and for every launch shape.
 *   layout, depth, and what is refused before any launch: as gsvc_picture_hash (rgb24: p = the channel); out must be 4-byte aligned.
 * Bytes between frames are not read.  The call zeroes out on the stream and does not synchronise.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_frames_histogram(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth,
                          uint32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Content-adaptive initial anchors (csrc/detail.hip, gsvc_amd/detail.py): a detail map of the luma codes
 * and points drawn from it.  Replaces the uniform draw of the reference's init_point_cloud (frame_cube/utils.py:6-15) for init="detail".
 *
 * gsvc_frames_detail: out[f, cy, cx] (uint32 [n_out, Hc, Wc], Hc = ceil(H / cell), Wc = ceil(W / cell), 4-byte aligned) = the sum of
 *     e = gx + gy + 2 gt
 * over the pixels (x, y) of cell (cy, cx) of frame f (an edge cell: over the pixels it has), in integers on the luma codes Y as they
 * are (the first H W samples of a frame; nothing is shifted or masked):
 *     gx = |Y(min(x + 1, W - 1), y) - Y(max(x - 1, 0), y)|,   gy likewise in y,   gt = |Y_g(x, y) - Y_f(x, y)|
 * with g the temporal neighbour: f + 1 if f + 1 < n, else f - 1 if n > 1, else gt = 0.  At most 4 * 65535 * 256 < 2^32 per cell.
 * 1 <= n_out <= n: the first n_out frames get a map and frame n_out - 1 may look at frame n_out (a caller that goes through a video
 * in chunks overlaps them by one frame).  Every output is written once by a plain store: out need not be zeroed.
 *   layout      GSVC_FRAMES_YUV444P or _YUV420P; rgb24 is refused.     depth  8, 10, 12 or 16.     cell  4, 8 or 16.
 * Refused with an error before any launch, besides those: n outside 1 .. 65535, n_out outside 1 .. n, an odd H or W for 4:2:0, a stride
 * below the frame's bytes (gsvc_frames_bytes), an odd base or stride for a deep format, a NULL pointer.  Nothing outside the luma planes
 * of the n frames is read.  Does not synchronise.
 *
 * gsvc_detail_sample: N points drawn from a map.  cdf (int64 [cells], on the device) = the inclusive prefix sum of the flattened
 * [T, Hc, Wc] map; its total D = cdf[cells - 1] is read on the device.  With
 *     h(seed, i, k) = splitmix64 of seed + (5 i + k + 1) * 0x9E3779B97F4A7C15 (mod 2^64):
 *                     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;   z = (z ^ z >> 27) * 0x94D049BB133111EB;   h = z ^ z >> 31
 *     mulhi64(a, b) = the upper 64 bits of a b,     f_k = (h(seed, i, k) >> 40) * 2^-24
 * point i is uniform if D == 0 or (h(seed, i, 0) >> 40) < mix24: its pixel is p = mulhi64(h(seed, i, 1), T H W), t = p / (H W),
 * y0 = (p mod H W) / W, x0 = p mod W, cw = ch = 1, and cell_of[i] = the cell that holds the pixel.  Otherwise r = mulhi64(h(seed, i, 1), D),
 * cell_of[i] = the first index with cdf[index] > r (a cell of weight 0 is never drawn) = (t Hc + cy) Wc + cx, x0 = cx cell, y0 = cy cell,
 * cw = min(cell, W - x0), ch = min(cell, H - y0).  Then, in float32,
 *     points[i] = (fmaf(f_2, cw, x0), fmaf(f_3, ch, y0), (f_4 - 0.5) + t)          (x and y in pixels, t in frames; one rounding each)
 * Refused with an error before any launch: cells != T Hc Wc, cells >= 2^31, mix24 > 2^24, a cell other than 4, 8, 16, T outside
 * 1 .. 65535, a side outside 1 .. 32768, N < 1, a NULL or misaligned pointer.  Does not synchronise.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_frames_detail(const uint8_t *frames, int64_t stride, int32_t n, int32_t n_out, int32_t H, int32_t W, int32_t layout,
                       int32_t depth, int32_t cell, uint32_t *out, void *stream);
int gsvc_detail_sample(const int64_t *cdf, int64_t cells, int32_t T, int32_t H, int32_t W, int32_t cell, int32_t N, uint64_t seed,
                       uint32_t mix24, float *points, int32_t *cell_of, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Film grain (csrc/grain.hip, gsvc_amd/grain.py): grain synthesised on delivered Y'CbCr frames from a
 * few dozen bytes of parameters (section GRAN of a bitstream file), and the statistics an encoder fits those parameters to.  Integers
 * only; gsvc_amd/grain.py's docstring states the synthesis sample by sample, tests/_grain_ref.py restates it in numpy.
 *
 * gsvc_grain_apply: adds grain IN PLACE to n (1 .. 16) frames (frame k at frames + k * stride) of GSVC_FRAMES_YUV444P / _YUV420P,
 * depth 8, 10, 12 or 16.  frame_ids_host: host array of n frame indices in the whole clip, each 0 .. 2^32 - 1 (they travel in the
 * kernel arguments).  With GOLD = 0x9E3779B97F4A7C15 and mix(z) the splitmix64 finaliser of gsvc_detail_sample, for plane p (0 Y, 1 U,
 * 2 V) of frame f and the sample (y, x) of the plane's own grid, y and x from -1 to the plane's height / width (the hash is defined
 * outside the picture: edges have no special case):
 *     key  = mix(seed + (3 f + p + 1) GOLD)
 *     h    = mix(key + (((y + 1) << 32) | ((x + 1) >> 1)) GOLD);     w = the upper 32 bits of h if (x + 1) is odd, else the lower
 *     g    = the sum of the four bytes of w - 510                                       (-510 .. 510, variance 21845)
 *     t    = kx[p] (g(y, x - 1) + g(y, x + 1)) + 64 g(y, x);     v = ky[p] (t(y - 1, x) + t(y + 1, x)) + 64 t(y, x)
 *     n    = (v + 2048) >> 12                                                           (arithmetic shift)
 *     l    = min(m >> (depth - 8), 255), m = the co-located UNGRAINED luma code (4:2:0 chroma: (a + b + c + d + 2) >> 2 of its four)
 *     s    = (scale[p][i] (16 - r) + scale[p][i + 1] r + 8) >> 4,  i = l >> 4,  r = l & 15
 *     grain = (n s + 2^(S - 1)) >> S,  S = 24 - depth       (scale: Q16 multipliers of n in 8-bit codes; a deep format gets 2^(depth - 8) times)
 *     out  = min(max(c + grain, min(lo, c)), max(hi, c))     lo .. hi: LIMITED 16 .. 235 (luma) / 16 .. 240 (chroma) times 2^(depth - 8),
 *                                                            FULL 0 .. 2^depth - 1: grain never moves a sample out of the nominal range,
 *                                                            and a sample whose grain is 0 keeps its code
 * A workgroup owns a 128 x 16 luma tile and the chroma tiles under it and reads nothing outside them: in place is safe.  Bytes of a
 * frame's row beyond the frame are not touched.  Refused with an error before any launch: a NULL pointer, rgb24 or an unknown layout,
 * a depth other than 8, 10, 12, 16, an unknown range, n outside 1 .. 16, an odd H or W for 4:2:0, a stride below the frame's bytes
 * (gsvc_frames_bytes), an odd base or stride for a deep format, a tap outside -32 .. 32, a frame index outside 0 .. 2^32 - 1.
 *
 * gsvc_grain_stats: out (uint64 [3, 16, 6], 8-byte aligned; the bits of int64 sums) over the n (1 .. 65535) frame pairs of two buffers, src
 * the source's codes and dec the decoder's.  Every plane is cut into whole 8 x 8 blocks of its own grid (partial blocks at the right and
 * bottom edges are skipped).  Per block: r = src - dec; A = the sum of the 112 absolute differences of horizontally and vertically
 * adjacent dec codes inside the block; bin = min((the sum of the dec LUMA codes of the co-located 8 x 8 region, 16 x 16 for 4:2:0 chroma)
 * >> (6 or 8) >> (depth - 8), 255) >> 4.  A block with A <= flat_threshold 2^(depth - 8) and every |r| <= max_residual 2^(depth - 8) adds
 * to out[plane][bin]:  1,  S1 = sum r,  S2 = sum r^2,  S1^2,  Px = sum r(x, y) r(x + 1, y) (56 pairs),  Py = sum r(x, y) r(x, y + 1).
 * Integer sums (64-bit atomics): the same bits in every run and for every launch shape.  The call zeroes out on the stream.  Refused
 * before any launch: as gsvc_picture_hash for both buffers, rgb24, a depth other than 8, 10, 12, 16, flat_threshold outside 0 .. 65535,
 * max_residual outside 0 .. 255.  Neither call synchronises.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t seed;
    uint16_t scale[3][17];        /* per plane, at 8-bit-normalised luma 0, 16, .., 256 */
    int8_t kx[3], ky[3];          /* per plane, -32 .. 32 (Q6) */
} gsvc_grain_params;
int gsvc_grain_apply(uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth, int32_t range,
                     const gsvc_grain_params *params, const int64_t *frame_ids_host, void *stream);
int gsvc_grain_stats(const uint8_t *src, int64_t src_stride, const uint8_t *dec, int64_t dec_stride, int32_t n, int32_t H, int32_t W,
                     int32_t layout, int32_t depth, int32_t flat_threshold, int32_t max_residual, uint64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Motion-compensated temporal prefilter of source frames (csrc/tfilter.hip, gsvc_amd/tfilter.py).  Integers
 * only; gsvc_amd/tfilter.py's docstring states the filter sample by sample, tests/_tfilter_ref.py restates it in numpy.
 *
 * gsvc_tfilter_frames: filters the n (1 .. 16) target frames first .. first + n - 1 of a resident clip of T (1 .. 65535) frames (frame t
 * at frames + t * stride) of GSVC_FRAMES_YUV444P / _YUV420P, depth 8, 10, 12 or 16, H, W >= 8, into out (target k at out + k *
 * out_stride; it may not overlap the clip).  flows: float32 [n, 4, 2, H, W] on the device; slot j of target k holds the flow from frame
 * t = first + k to frame t + d, d = (-2, -1, +1, +2)[j], as gsvc_flow_estimate writes it.  A slot whose t + d lies outside 0 .. T - 1 is
 * never read and its neighbour contributes nothing.  With // the floor division, per neighbour d:
 *     mv    = clamp(rint(4 f), -32768, 32767) per component (the float32 product, rounded half to even): quarter luma pels
 *             (flows should be finite: +-inf clamps like any large value and a NaN component is read as -32768 — memory-safe, as every
 *             position is clamped, but meaningless; nothing checks them)
 *     pred  : for an h x w plane with `unit` sub-positions per sample, px = clamp(unit x + mvx, 0, unit (w - 1)), x0 = min(px // unit,
 *             w - 2), fx = px - unit x0 (py, y0, fy likewise), and over the codes a of frame t + d
 *             pred = ((unit - fx)(unit - fy) a00 + fx (unit - fy) a01 + (unit - fx) fy a10 + fx fy a11 + unit^2 / 2) // unit^2
 *             luma and 4:4:4 chroma: unit 4, the pixel's own mv; 4:2:0 chroma: unit 8, the mv of luma pixel (2y, 2x)
 *     i_b   = min(63, 2048 SSE // (n_B q[0]^2)), SSE = the sum of (Y_t - pred)^2 over the n_B pixels of the sample's 8 x 8 luma block
 *             (partial blocks at the right and bottom edges count the pixels they have; chroma: the block holding (2y, 2x), 4:4:4 (y, x))
 *     i_p   = min(63, 128 |c - pred| // q[p])
 *     w_d   = (wt[|d| - 1] lut_b[i_b] lut_p[i_p] + 2^15) >> 16
 *     out   = (256 c + sum_d w_d pred_d + Wt // 2) // Wt,   Wt = 256 + sum_d w_d
 * q_host (3), wt_host (2), lut_b_host and lut_p_host (64 each) are host arrays that travel in the kernel arguments.  Every sampled
 * position is clamped into its plane: no flow value makes the kernel read outside a frame.  No atomics, no workspace; the result does
 * not depend on the launch geometry.  Bytes of an output row beyond the frame are not touched.  Refused with an error before any
 * launch: a NULL pointer, rgb24 or an unknown layout, a depth other than 8, 10, 12, 16, n outside 1 .. 16, T outside 1 .. 65535,
 * first < 0 or first + n > T, a side below 8, an odd H or W for 4:2:0, a stride below the frame's bytes (gsvc_frames_bytes), an odd base
 * or stride for a deep format, flows not 4-byte aligned, an output that overlaps the clip, q outside 1 .. 65535, wt or a table entry
 * above 256.
 *
 * gsvc_noise_sums: out[k, p] (uint64 [n, 3], 8-byte aligned; n 1 .. 16) = over the interior samples (1 <= y <= h - 2, 1 <= x <= w - 2) of
 * plane p of frame k the sum of
 *     |c(y-1,x-1) - 2 c(y-1,x) + c(y-1,x+1) - 2 c(y,x-1) + 4 c(y,x) - 2 c(y,x+1) + c(y+1,x-1) - 2 c(y+1,x) + c(y+1,x+1)|
 * (Immerkaer's noise estimator before its scaling).  Integer sums: the same bits in every run and for every launch shape.  The call
 * zeroes out on the stream.  Formats and refusals as gsvc_tfilter_frames.  Neither call synchronises.
 * ---------------------------------------------------------------------------------------------------- */
int gsvc_tfilter_frames(const uint8_t *frames, int64_t stride, int32_t T, int32_t first, int32_t n, int32_t H, int32_t W, int32_t layout,
                        int32_t depth, const float *flows, const uint32_t *q_host, const uint32_t *wt_host, const uint16_t *lut_b_host,
                        const uint16_t *lut_p_host, uint8_t *out, int64_t out_stride, void *stream);
int gsvc_noise_sums(const uint8_t *frames, int64_t stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth, uint64_t *out,
                    void *stream);

/* ------------------------------------------------------------------------------------------------------
 * [INTERNAL] Lanczos-3 resampler on the sample codes of planar frames (csrc/resample.hip, gsvc_amd/resample.py).
 * Integers only; gsvc_amd/resample.py's docstring states the taps and the arithmetic, tests/_resample_ref.py restates it in numpy.
 *
 * gsvc_resample_frames: resamples n (1 .. 16) frames (frame k at src + k * src_stride) of GSVC_FRAMES_YUV444P / _YUV420P, depth d = 8,
 * 10, 12 or 16, from H x W to out_H x out_W (frame k at dst + k * dst_stride), every plane on its own between its own dimensions
 * (4:2:0 chroma: (H / 2, W / 2) -> (out_H / 2, out_W / 2)).  A table (first, coef, nt) describes one axis of one plane size: for output
 * index j, first[j] (int32 [dst]) is the first source index and coef[j, 0 .. nt - 1] (int16 [dst, GSVC_RESAMPLE_TAPS], Q14, summing to
 * 16384, sum of magnitudes <= 32767; zeros behind a row's own taps) its weights; nt (1 .. 24) is the largest tap count of the table and
 * slots at or beyond it are never read.  Tables are device arrays: lx / ly for the luma columns / rows, cx / cy for the chroma ones
 * (4:4:4: the same arrays again).  gsvc_amd/resample.py builds them (filter_taps: Lanczos-3, widened by the ratio when downscaling,
 * centre-aligned).  With >> the arithmetic shift and every tap index clamped into the plane, clamp(first + k, 0, src - 1):
 *     t(y, j)   = sum_k cx[j, k] a(y, clamp(fx[j] + k))                                   |t| < 2^31
 *     m(y, j)   = (t + 2^(d - 3)) >> (d - 2)                                              not clamped
 *     u(i, j)   = sum_k cy[i, k] m(clamp(fy[i] + k), j)                                   exact, 64-bit
 *     out(i, j) = clamp((u + 2^(29 - d)) >> (30 - d), 0, 2^d - 1)
 * Codes are read as they are (a word above 2^d - 1 in a deep frame is not masked).  An axis with src == dst has one coefficient of
 * 16384 per row, so a 1:1 call copies the frames.  The intermediate m lives in LDS only; no atomics, no workspace; the result does not
 * depend on the launch geometry; bytes of an output row beyond the frame are not touched.  Every index the kernel derives from a
 * table is clamped, so no table content makes it read outside a plane.  Refused with an error before any launch: a NULL pointer, rgb24
 * or an unknown layout, a depth other than 8, 10, 12, 16, n outside 1 .. 16, an odd side for 4:2:0, a side below 2, a ratio above 4
 * either way, nt outside 1 .. 24, a stride below the frame's bytes (gsvc_frames_bytes), an odd base or stride for a deep format, a
 * table not aligned to its element, an output that overlaps the input.  Does not synchronise.
 * ---------------------------------------------------------------------------------------------------- */
#define GSVC_RESAMPLE_TAPS 24
int gsvc_resample_frames(const uint8_t *src, int64_t src_stride, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t depth, uint8_t *dst,
                         int64_t dst_stride, int32_t out_H, int32_t out_W, const int32_t *lx_first, const int16_t *lx_coef, int32_t lx_nt,
                         const int32_t *ly_first, const int16_t *ly_coef, int32_t ly_nt, const int32_t *cx_first, const int16_t *cx_coef,
                         int32_t cx_nt, const int32_t *cy_first, const int16_t *cy_coef, int32_t cy_nt, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Dense optical flow of adjacent frames (csrc/flow.hip): coarse-to-fine Horn-Schunck with warping.  No weights, stencils only: the
 * same bits in every run, for every batch size and launch geometry.
 *
 * gsvc_flow_estimate: pair k reads the luma planes luma0 + k * plane_pitch and luma1 + k * plane_pitch (float32 [H, W] in [0, 1],
 * rows contiguous; the T - 1 pairs of T resident frames are one call with luma1 = luma0 + plane_pitch) and writes flow_out[k], float32
 * [2, H, W]: flow[0] = the x displacement, flow[1] = the y displacement in pixels at the pixel of the first frame,
 *   I0(x, y) ~ I1(x + flow[0], y + flow[1])
 * (what gsvc_optical_forward reads).
 *   pyramid     P[0] = blur(luma), P[l + 1] = blur(pool(P[l])) while min(h, w) / 2 >= min_side and fewer than max_levels levels exist.
 *               blur: the 5-tap binomial (1 4 6 4 1) / 16 down the columns, then along the rows, borders replicated.  pool: the 2 x 2
 *               mean, (h, w) -> (h / 2, w / 2); an odd last row or column is dropped.
 *   bilinear    bil(a, x, y) of an h x w plane: x clamped to [0, w - 1], x0 = min(floor(x), w - 2), fx = x - x0 (y likewise);
 *               top = a00 + fx (a01 - a00), bot = a10 + fx (a11 - a10), value = top + fy (bot - top).
 *   levels      from the coarsest to the finest; (u0, v0) = 0 on the coarsest, on a finer level
 *               2 bil(coarse, (x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5) for both components.
 *   warp        `warps` times per level: Bw = bil(P1, x + u0, y + v0); central differences 0.5 (a[x + 1] - a[x - 1]) of P0 and of Bw with
 *               replicated borders; ox = max(-(x + u0), (x + u0) - (w - 1), 0), oy likewise, m = clamp(1 - max(ox, oy), 0, 1);
 *               Ix = m 0.5 (P0x + Bwx), Iy = m 0.5 (P0y + Bwy), It = m (Bw - P0), c = It - Ix u0 - Iy v0, den = 1 / (alpha^2 + Ix^2 + Iy^2).
 *   solve       (U, V) = (u0, v0), then `iters` Jacobi sweeps, every pixel from the previous iterate: Ub, Vb = the means of the four
 *               neighbours (replicated borders), t = (Ix Ub + Iy Vb + c) den, U = Ub - Ix t, V = Vb - Iy t.
 *               Then u0 += clamp(U - u0, -max_step, max_step), v0 likewise.
 * The finest level's (u0, v0) after its last warp is the result.  Every a * b + c rounds twice (no contraction).
 * workspace: gsvc_flow_workspace_bytes(n, H, W, max_levels, min_side) bytes, 16-byte aligned, the caller's, not relied on to hold
 * anything: both pyramids, three flow fields and three coefficient planes at full size (about 11.7 floats per pixel and pair; < 0 for
 * a shape gsvc_flow_estimate refuses).  Refused with an error before any launch: a NULL pointer, n outside 1 .. 65535, a side
 * outside 2 .. 32768, min_side < 2, min(H, W) < min_side, alpha <= 0, max_step <= 0, warps, iters or max_levels < 1, plane_pitch
 * below H W, a plane base that is not 4-byte or a workspace that is not 16-byte aligned.  Nothing synchronises.
 *
 * [INTERNAL] the stages, for tests (planes [n, h, w] contiguous):
 * gsvc_flow_pyramid_step   dst = blur(src) (pool = 0) or blur(pool(src)) (pool = 1: dst is [n, sh / 2, sw / 2]).
 * gsvc_flow_warp           Ix, Iy, c of one warp.  coarse_u, coarse_v NULL: u0, v0 are read.  Else they are WRITTEN: the coarse flow
 *                          [n, ch, cw] upsampled as above, formed inside the same pass.
 * gsvc_flow_solve          `iters` sweeps from U, V; u0, v0 NULL: out = (U, V) after them, else out = u0 + clamp(U - u0, +-max_step)
 *                          (the epilogue of a warp's last solver launch).  A workgroup owns 56 x 56 pixels and runs 4 sweeps per launch
 *                          on 64 x 64 staged ones; a level of at most 64 x 64 runs all its sweeps in one launch.  workspace:
 *                          gsvc_flow_solve_workspace_bytes(n, h, w) bytes, 16-byte aligned; out may not alias an input.
 * ---------------------------------------------------------------------------------------------------- */
int64_t gsvc_flow_workspace_bytes(int32_t n, int32_t H, int32_t W, int32_t max_levels, int32_t min_side);
int gsvc_flow_estimate(const float *luma0, const float *luma1, int64_t plane_pitch, int32_t n, int32_t H, int32_t W, float alpha,
                       int32_t warps, int32_t iters, int32_t min_side, int32_t max_levels, float max_step, float *flow_out,
                       void *workspace, void *stream);
int gsvc_flow_pyramid_step(const float *src, int32_t n, int32_t sh, int32_t sw, int32_t pool, float *dst, void *stream);
int gsvc_flow_warp(const float *P0, const float *P1, float *u0, float *v0, int32_t n, int32_t h, int32_t w, const float *coarse_u,
                   const float *coarse_v, int32_t ch, int32_t cw, float *Ix, float *Iy, float *c, void *stream);
int64_t gsvc_flow_solve_workspace_bytes(int32_t n, int32_t h, int32_t w);
int gsvc_flow_solve(const float *U, const float *V, const float *Ix, const float *Iy, const float *c, const float *u0, const float *v0,
                    int32_t n, int32_t h, int32_t w, float alpha, int32_t iters, float max_step, float *out_u, float *out_v,
                    void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSVC_HIP_H */
