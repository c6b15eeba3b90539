/*
 * egonerf_hip.h — C ABI of libegonerf_hip.so: EgoNeRF's volume-rendering hot path on MI355X (gfx950).
 *
 * Plain pointers and sizes only (no torch types).  Every pointer marked "dev" is device memory owned
 * by the caller; the library allocates nothing, keeps no global mutable state and launches every
 * kernel on the hipStream_t handed in (`stream`, may be NULL = default stream).  All entry points
 * return 0 on success or a negative EGO_E_* / positive hipError_t code; ego_last_error() returns a
 * thread-local message.  The reference signals errors with Python exceptions / assert
 * (models/EgoNeRF.py:504,522); the Python host layer turns non-zero codes into RuntimeError.
 *
 * Reference interface replaced by each entry point (paths relative to the reference repo):
 *   ego_erp_rays            get_ray_directions_360 + get_rays      dataLoader/ray_utils.py:24-40, :85-113
 *   ego_ray_batch_gather    allrays[ids], allrgbs[ids]            train.py:247-248, dataLoader/dataset_omniblender.py:71-84
 *   ego_ray_batch_sample    SimpleSampler / ThetaImportanceSampler.nextids   sampler.py:4-38 (device generator, not numpy's stream)
 *   ego_camera_rays         get_ray_directions{,_blender,_360} + get_rays   dataLoader/ray_utils.py:24-113 (pose in device memory)
 *   ego_finish_frame        clamp, * 255, uint8; visualize_depth_numpy; rgbd   renderer.py:227-240, :141-174, utils.py:14-27
 *   ego_camera_rays_ex      the same with the eyes of an omnidirectional-stereo panorama and s x s rays per pixel (no counterpart)
 *   ego_resolve_frame       ego_finish_frame of the average of s x s samples per pixel (no counterpart)
 *   ego_sample_ray_exp      EgoNeRF.sample_ray_exp              models/EgoNeRF.py:56-87
 *   ego_from_cartesian      YinYangSphericalCoords.from_cartesian  models/coordinates.py:468-498
 *   ego_normalize_coord     YinYangSphericalCoords.normalize_coord models/coordinates.py:442-466 (+ :110-131)
 *   ego_density_feature     EgoNeRF.compute_densityfeature         models/EgoNeRF.py:291-347
 *                           EgoNeRF.compute_coarse_densityfeature  models/EgoNeRF.py:232-289 (coarse=1)
 *   ego_app_feature         EgoNeRF.compute_appfeature             models/EgoNeRF.py:349-413
 *   ego_feature2density     TensorBase.feature2density             models/tensorBase.py:415-419
 *   ego_raw2alpha           raw2alpha                              models/tensorBase.py:22-27
 *   ego_mlp_fea             MLPRender_Fea.forward                  models/tensorBase.py:54-78
 *   ego_sample_pdf_merge    sample_pdf + sort(cat(z, z_fine))      dataLoader/ray_utils.py:156-187, models/EgoNeRF.py:532-542
 *   ego_envmap_radiance     EnvironmentMap.get_radiance            models/envmap.py:6-14,26-34
 *   ego_avgpool_tables      EgoNeRF.update_coarse_sigma_grid       models/EgoNeRF.py:124-133
 *   ego_pack_mlp            (new) weight re-layout for the MFMA kernels; no reference counterpart
 *   ego_march_density       EgoNeRF.forward lines 507-529 / 544-553 (sampling -> sigma -> alpha,w)   models/EgoNeRF.py
 *   ego_shade               EgoNeRF.forward lines 555-556 / 571-572 (app feature -> renderModule)   models/EgoNeRF.py
 *   ego_composite           EgoNeRF.forward lines 579-598 (acc, rgb_map, envmap, clamp, depth)       models/EgoNeRF.py
 *   ego_render_forward      EgoNeRF.forward (whole call)                                          models/EgoNeRF.py:491-602
 *
 * Table layout in HBM ("channel-last"): a reference plane parameter (1,C,H,W) is stored as [H][W][C]
 * and a line parameter (1,C,L,1) as [L][C], fp32, so one bilinear tap is one contiguous C*4-byte read
 * (64 B for the 16 density components, 192 B for the 48 appearance components).  torch's
 * channels_last memory format of the reference-shaped tensor is exactly this layout.
 */
#ifndef EGONERF_HIP_H
#define EGONERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGO_ABI_VERSION 17

enum { EGO_PREC_F16X3 = 0, EGO_PREC_F32 = 1, EGO_PREC_F16F8 = 2, EGO_PREC_F16F6 = 3 };
/* ego_scene.head: the appearance head TensorBase.init_render_func selected (models/tensorBase.py:186-200) */
enum { EGO_HEAD_MLP_FEA = 0, EGO_HEAD_RGB = 1 };

enum {
  EGO_OK = 0,
  EGO_E_BADARG = -1,   /* null pointer / bad size / unsupported configuration */
  EGO_E_UNSUPPORTED = -2,
};

/* One VM-decomposed field of both grids.  grid index 0 = yin, 1 = yang; i = 0..2 follow the
 * reference's matMode [[0,1],[0,2],[1,2]] / vecMode [2,1,0] over axes (r, theta, phi):
 *   plane[g][0]: [N_theta][N_r][C]   line[g][0]: [N_phi][C]
 *   plane[g][1]: [N_phi][N_r][C]     line[g][1]: [N_theta][C]
 *   plane[g][2]: [N_phi][N_theta][C] line[g][2]: [N_r][C]                                      */
/* The 12 tables of one field must lie within 4 GB of each other (allocate them from one buffer, as the Python host layer
 * does): the forward gathers address every tap as lowest-table-address + 32-bit byte offset (scalar base + one VGPR per
 * address).  Entry points return EGO_E_BADARG for a field that does not. */
typedef struct ego_vm_field {
  const float* plane[2][3]; /* dev */
  const float* line[2][3];  /* dev */
  int32_t n_comp;           /* C: 16 (density) or 48 (appearance) in every shipped config */
  int32_t res[3];           /* (N_r, N_theta, N_phi) of THIS field (coarse field = full / 2) */
} ego_vm_field;

typedef struct ego_scene {
  /* coordinates (models/coordinates.py:76,500-505): all float32 values computed by the host exactly
   * as the reference computes them */
  float center[3];
  float ang_near[2]; /* theta, phi lower bounds: pi/4, -3pi/4 */
  float ang_inv[2];  /* 1/(far-near) per angle */
  const float* r_lut; /* dev [n_r_lut] = reference_r_grid, n_r_lut = N_r + 1 */
  int32_t n_r_lut;
  int32_t n_r;        /* N_r used in the final division (coordinates.py:156) */
  /* density activation (tensorBase.py:415-419) and compositing scale (opt.py:144) */
  int32_t act_softplus; /* 1 softplus, 0 relu */
  float density_shift;
  float distance_scale;
  /* tables */
  ego_vm_field density;
  ego_vm_field density_coarse;
  ego_vm_field app;
  const float* basis[2]; /* dev [app_dim][3*C_app] row-major = nn.Linear.weight, per grid */
  int32_t app_dim;       /* 27 */
  /* MLP_Fea (tensorBase.py:54-78): reference-layout weights (row-major [out][in]) ... */
  const float* mlp_w[3]; /* dev [128][150], [128][128], [3][128] */
  const float* mlp_b[3]; /* dev */
  int32_t mlp_in, mlp_hidden, view_pe, fea_pe;
  /* ... and the MFMA re-layout of the same weights produced by ego_pack_mlp (dev, EGO_PACKED_FLOATS) */
  const float* packed;
  /* environment map (models/envmap.py): emission [3][2h][h] or NULL */
  const float* envmap;
  int32_t envmap_h;
  /* arithmetic of the basis/MLP matrix products: EGO_PREC_F16X3 (0) = three fp16 MFMAs per product (hi*hi + lo*hi + hi*lo,
   * fp32 accumulate, ~2^-21 relative: fp32-grade); EGO_PREC_F32 = fp32-input MFMA; EGO_PREC_F16F8 = layers 1 and 2 of the MLP
   * with the main term in fp16 and both correction terms in one block-scaled fp8 (e4m3) MFMA per pair of k-steps (~2^-16
   * relative per product; composited max |d RGB| ~8e-6, i.e. > 10x inside the 1e-4 bar; inference only, the training forward
   * keeps the fp16 split); EGO_PREC_F16F6 = the same split with the correction terms on the fp6 (e2m3) path of the block-scaled
   * MFMA, two instructions per group of four k-steps, one power-of-two block scale per lane and 32 K values - static for the
   * weights, taken from the largest activation of the block at run time (so no fixed range to saturate); per-sample error 1.1x
   * F16F8's, shade kernel 3-4 % faster */
  int32_t mlp_precision;
  /* Opt-in skipping (EgoNeRF.forward itself evaluates every sample; these follow TensorBase.forward's mask semantics,
   * models/tensorBase.py:464-478, and YinYangAlphaGridMask, models/EgoNeRF.py:11-24):
   * occ: two {0,1} byte volumes [grid][N_phi][N_theta][N_r] (occ_res = N_r, N_theta, N_phi) or NULL.  A sample whose
   * trilinear mask value (align_corners, zero padding) is <= 0 gets sigma = 0.
   * term_eps > 0: samples whose incoming transmittance T is below term_eps get weight 0 (|d rgb| <= term_eps). */
  const uint8_t* occ;
  int32_t occ_res[3];
  float term_eps;
  /* Optional half-precision copy of the appearance tables (inference only): same shapes/layout as `app`, elements are
   * IEEE binary16 (the pointer type is nominal).  app_f16 != 0 makes ego_shade / ego_app_feature gather from it
   * (halves the bytes through the vector L1; interpolation and everything after stay fp32).  Measured effect on RGB in
   * DESIGN.md.
   * app_f16 selects the source of the appearance features in inference: EGO_APP_TABLES (0) = the fp32 tables `app`; EGO_APP_HALF (1) =
   * the half tables in app16, as above; EGO_APP_DENSE (2) = the baked node grid of the features (no struct member was added for it, so
   * sizes and offsets stand and EGO_ABI_VERSION stays 17): app16.plane[0][0] then points to what ego_bake_app_dense wrote for `app` and
   * `basis` (128 bytes per node, 16-byte aligned, both grids under 4 GB together; the pointer type is nominal), app16.res holds the
   * resolution it was baked at, which must equal app.res, app16.n_comp is 48 and the other eleven pointers of app16 are not read.  The
   * split-arithmetic inference kernels behind ego_shade (without dumps), ego_shade_composite, ego_shade_live and ego_app_feature then
   * interpolate the 27 features from the grid (8 taps of one node each per sample) instead of gathering the 18 table taps and
   * multiplying by the basis; EGO_PREC_F32 and every dumping (training) call keep the fp32 tables.  The grid is a SNAPSHOT of the tables
   * and of both basis matrices, like `packed`: bake again after either changed. */
  ego_vm_field app16;
  int32_t app_f16;
#define EGO_APP_TABLES 0
#define EGO_APP_HALF 1
#define EGO_APP_DENSE 2
  /* Radius LUT of the fine pass after resampling, when it differs from r_lut: with the plain exponential grid
   * (interval_th = False, coordinates.py:132-155) the first pass normalises r on the `downsample=2` grid (EgoNeRF.py:524) and
   * the fine pass on the full one (EgoNeRF.py:546).  NULL / 0: the fine pass uses r_lut. */
  int32_t n_r_lut_fine;
  const float* r_lut_fine;
  int32_t n_r_fine;
  /* Appearance skip of TensorBase.forward (models/tensorBase.py:482-487, `rayMarch_weight_thres`): < 0 = off (every sample is
   * shaded); >= 0: a sample whose weight is <= weight_thres contributes colour 0 — its weight still counts in acc / depth — and
   * 32-sample tiles without any sample above the threshold are not shaded.  weight_thres = 0 is EXACT (EgoNeRF.forward adds
   * w * rgb = 0 for those samples, models/EgoNeRF.py:583) and is what the host layer sets by default. */
  float weight_thres;
  /* Optional accelerator for `occ` (NULL = off): [grid][N_phi - 1][N_theta - 1][N_r - 1] bytes, 1 iff any of the cell's eight corner
   * voxels is set.  The march then decides "mask value > 0" for a sample strictly inside a cell from this one byte (identical result:
   * all eight trilinear weights are positive there) and keeps the eight-tap evaluation for samples on lattice planes / outside. */
  const uint8_t* occ_cell;
  /* Appearance head (models/tensorBase.py:186-200).  EGO_HEAD_MLP_FEA (0): MLPRender_Fea (tensorBase.py:54-78); shadingMode 'MLP'
   * (MLPRender, tensorBase.py:107-129) is the same network with fea_pe = 0, i.e. mlp_in = 3 + 6 view_pe + app_dim.  EGO_HEAD_RGB (1):
   * RGBRender (tensorBase.py:37-39): the per-sample colour is the 3-channel appearance feature itself (no MLP, no sigmoid; app_dim must be
   * 3, mlp_in = mlp_hidden = 0, mlp_w / mlp_b unused).  'MLP_PE' cannot run in EgoNeRF.forward (it is handed 7-column coordinates for a
   * 3-column encoding), 'SH' crashes there too (its stage op is ego_sh_render). */
  int32_t head;
  /* Optional baked node grids of the 16-component density fields (inference only; NULL = off; append-only, EGO_ABI_VERSION stays 17):
   * what ego_bake_density_dense writes for `density` / `density_coarse`, [grid][N_phi][N_theta][N_r][4] float32 at that field's
   * resolution, 16-byte aligned, both grids under 4 GB together.  ego_march_density then interpolates the field it was asked for from
   * its grid (8 taps of 16 B per sample) instead of gathering the 18 table taps (1152 B).  A SNAPSHOT of the tables, like `packed`:
   * bake again after the tables changed. */
  const float* density_dense;
  const float* density_coarse_dense;
} ego_scene;

/* number of floats ego_pack_mlp writes: the packed weight blob used by ego_shade / ego_mlp_fea / ego_app_feature
 * (fp32 fragment layout, the fp16-split layout, then the basis fragments in the K order of the fp16-table gather) */
int64_t ego_packed_floats(void);
/* the same for the shape of `sc` (app_dim, app.n_comp, mlp_in, mlp_hidden, view_pe, fea_pe): ego_packed_floats() for the tuned shape
 * every shipped config resolves to (27 / 48 / 150 / 128 / 2 / 2), the fp32 layout of the any-shape compatibility kernels otherwise
 * (opt.py:87-100 lets a user choose n_lamb_sh, data_dim_color, featureC, view_pe, fea_pe; supported: n_comp a multiple of 4 up to
 * 48, app_dim <= 32, featureC 64 or 128, view_pe / fea_pe <= 8; density n_comp a multiple of 4 up to 48).  Those kernels compute
 * in plain fp32 and are about an order of magnitude slower than the tuned path; they train through ego_shade_train_generic /
 * ego_shade_backward_generic / ego_scatter_generic (row-major buffers; ego_shade's `dump` argument is for the tuned shape only). */
int64_t ego_packed_floats_scene(const ego_scene* sc);

int ego_abi_version(void);
const char* ego_last_error(void);
/* sizeof the ABI structs as compiled (0 ego_scene, 1 ego_render_args, 2 ego_vm_field, 3 ego_adam_tensor, 4 ego_shade_dump, 5 ego_ray_bank): lets a foreign-
 * language binding verify its struct mirrors at load time */
int64_t ego_sizeof(int32_t which);

/* Run-time self-test of the team-gather kernel family (no reference counterpart).  Builds of these kernels that contain
 * packed fp32 instructions broadcasting the high dword of a register pair returned different bits call after call on MI355X; the build
 * fences that off and this entry point checks the SHIPPED code on the device at hand: ego_app_feature and ego_shade (f16x3, f16f8, f16f6) run
 * `reps` times on a synthetic scene laid out in `workspace` (dev, ego_selftest_workspace_bytes() bytes, 256-byte aligned) and every
 * result is bit-compared with the first.  Synchronises `stream`.  Returns EGO_OK and *mismatching_calls = 0, or EGO_E_UNSUPPORTED with
 * the number of calls whose bits differed (host pointer).  The host layer calls it once per process and device (EGO_SKIP_SELFTEST=1 opts out). */
int64_t ego_selftest_workspace_bytes(void);
int ego_selftest(void* workspace, int64_t workspace_bytes, int32_t reps, int32_t* mismatching_calls, void* stream);

/* ---- separately callable stages (back the reference's public methods; parity-tested one by one) ---- */

/* rays [N][6] (o,d); r_sched [S] = radial offsets (host-built, float32); jitter [N][S] in [0,1) or NULL.
 * z = near + r (+ step*jitter); xyz = o + d*z.  Outputs xyz [N][S][3], z [N][S] (either may be NULL). */
int ego_sample_ray_exp(const float* rays, const float* r_sched, const float* jitter, float near_, int64_t N, int32_t S,
                       float* xyz, float* z, void* stream);

/* Equirectangular rays of rows [row0, row0+n_rows) of an H x W panorama for the camera-to-world pose c2w (HOST pointer,
 * 3x4 row-major): get_ray_directions_360 + get_rays (dataLoader/ray_utils.py:24-40, :85-113).  normalize != 0 divides the
 * camera-space direction by its norm first, as both ERP datasets do before get_rays (dataset_egocentric_video.py:57-58,
 * dataset_omniblender.py:42-43).  rays [n_rows*W][6] dev. */
int ego_erp_rays(int32_t H, int32_t W, int32_t row0, int32_t n_rows, const float* c2w, int32_t normalize, float* rays,
                 void* stream);

/* ---- device-resident training batches (csrc/ego_batch.hip; append-only additions, EGO_ABI_VERSION stays 17: no existing symbol,
 * struct or argument list changed) ----
 * A ray bank is what train.py:247-248 indexes as allrays[ids] / allrgbs[ids], kept as its sources instead of materialised: K poses and K
 * 8-bit RGBA images (a 3-channel image is stored with A = 255) of H x W pixels, and the ROI window of get_rays (dataLoader/ray_utils.py:
 * 100-103: rows [r0, r0 + n_rows), columns [c0, c0 + n_cols)).  Ray index space = the layout of the reference's all_rays:
 * idx = img * (n_rows * n_cols) + row * n_cols + col with (row, col) counted inside the window; total = K * n_rows * n_cols. */
typedef struct ego_ray_bank {
  const float* poses;    /* dev [K][3][4] camera-to-world, row-major */
  const uint8_t* images; /* dev [K][H][W][4] RGBA, 4-byte aligned; may be NULL when no colours are asked for */
  int32_t K, H, W;       /* images, full image size */
  int32_t r0, n_rows, c0, n_cols;
  int32_t normalize;     /* as ego_erp_rays */
} ego_ray_bank;

/* allrays[idx], allrgbs[idx] of train.py:247-248 without the arrays: idx [B] int64 dev -> rays [B][6] (bit-equal to the rows ego_erp_rays
 * writes for that pose and pixel), rgb [B][3] = the pixel's u8 / 255 blended on white, rgb * a + (1 - a), each operation rounded on its own
 * (dataLoader/dataset_omniblender.py:71-81; with a = 1 exactly u8 / 255).  rays or rgb may be NULL (not written).  The entry point cannot
 * see device values: 0 <= idx[i] < total is the caller's contract; a row whose index is outside reads nothing and is filled with NaN.
 * B == 0 is a no-op. */
int ego_ray_batch_gather(const ego_ray_bank* bank, const int64_t* idx, int64_t B, float* rays, float* rgb, void* stream);

/* sampler.nextids() of train.py:247 (sampler.py:4-38) on the device: fills idx [B] (int64 dev) for iteration *counter (int64 dev, read by the
 * kernel: a replayed hipGraph draws a new batch whenever the counter has been advanced) and, where rays / rgb are not NULL, gathers them in the
 * same launch.  Every index is a pure function of (seed, *counter, lane) through Philox4x32-10 - NOT numpy's legacy stream.
 * EGO_BATCH_SIMPLE (SimpleSampler, sampler.py:4-16): permutation epochs of floor(total / B) batches (the tail of a permutation is dropped as
 * there), epoch = *counter / that, position p = (*counter % that) * B + lane sent through a keyed bijection of [0, total): a six-round
 * balanced Feistel network over the smallest even number of bits covering total, cycle-walked back into range, round keys = Philox(seed,
 * epoch); no permutation is materialised.  Needs total >= 2 B.
 * EGO_BATCH_THETA (ThetaImportanceSampler, sampler.py:19-38): image uniform in [0, K), column uniform in [0, n_cols), row by inverse CDF:
 * row_cdf [n_rows] float32 dev, non-decreasing, last entry 1 (the cumulative sum of the host-built weights cos(lat) * lambda + 1), row =
 * first entry > u for a 24-bit uniform u. */
enum { EGO_BATCH_SIMPLE = 0, EGO_BATCH_THETA = 1 };
int ego_ray_batch_sample(const ego_ray_bank* bank, int32_t mode, uint64_t seed, const int64_t* counter, const float* row_cdf, int64_t B,
                         int64_t* idx, float* rays, float* rgb, void* stream);

/* Patch batches (append-only addition, EGO_ABI_VERSION stays 17; no reference counterpart: its samplers draw independent pixels): one launch,
 * like ego_ray_batch_sample, fills idx [B] (and rays [B][6] / rgb [B][3] where not NULL) with B = P ph pw + n_random rows for iteration
 * *counter (int64 dev, read by the kernel).  Row p ph pw + a pw + b is pixel (row0_p + a stride, col0_p + b stride) of image img_p, counted
 * inside the bank's window: a patch is contiguous and row-major, so rgb[0 .. P ph pw) reads as [P][ph][pw][3] (ego_patch_ssim's layout).  The
 * trailing n_random rows are independent uniform pixels of the window.  idx uses the bank's index space, so ego_ray_batch_gather and the
 * depth / mask gathers work on it unchanged.
 * The rule, with c = *counter, hi(x, n) = (x * n) >> 32 (the high half of a 32 x 32-bit product, bias <= n / 2^32) and Philox4x32-10:
 *   patch p:   x = Philox(counter words (p lo, p hi, c lo, c hi), key (seed lo ^ 0x50415443, seed hi));  img_p = hi(x0, K),
 *              row0_p = hi(x1, n_rows - (ph - 1) stride), col0_p = hi(x2, C).  When the window spans the full width (c0 == 0 and n_cols == W)
 *              the panorama wraps: C = n_cols and the columns are (col0_p + b stride) mod n_cols, so a patch may straddle the seam;
 *              otherwise C = n_cols - (pw - 1) stride, the origins whose patch fits.
 *   random r:  x = Philox(counter words (r lo, r hi, c lo, c hi), key (seed lo ^ 0x52414E44, seed hi));  image hi(x0, K), column hi(x1, n_cols),
 *              row hi(x2, n_rows): EGO_BATCH_THETA's image and column draw with the row uniform too.
 * The key tweaks keep both streams apart from EGO_BATCH_THETA's, which keys the same counter words with the seed itself.  Every draw is a pure
 * function of (seed, *counter, p) or (seed, *counter, r).  Refuses, before any launch: P < 0 or n_random < 0; ph, pw or stride < 1; a patch
 * extent (ph - 1) stride + 1 > n_rows or (pw - 1) stride + 1 > n_cols (with or without the wrap); null counter or idx with B > 0.  B == 0 is
 * a no-op. */
int ego_ray_batch_sample_patches(const ego_ray_bank* bank, uint64_t seed, const int64_t* counter, int64_t P, int32_t ph, int32_t pw,
                                 int32_t stride, int64_t n_random, int64_t* idx, float* rays, float* rgb, void* stream);

/* Depth targets next to a bank (append-only addition, EGO_ABI_VERSION stays 17; ego_ray_bank itself does not change): depth [K][H][W] dev,
 * float32 (is_half == 0) or float16 (is_half != 0), one value per pixel of the bank's full images, in units of distance along the
 * normalised ray, 0 = no target.  out[i] (float32 [B] dev) = the depth of the pixel idx[i] names in the bank's index space (img, r0 + row,
 * c0 + col), converted exactly.  As in ego_ray_batch_gather, a row whose index is outside [0, total) reads nothing and is filled with NaN
 * (ego_ray_depth_loss then treats that ray as invalid).  The bank's images may be NULL.  B == 0 is a no-op. */
int ego_ray_batch_gather_depth(const ego_ray_bank* bank, const void* depth, int32_t is_half, const int64_t* idx, int64_t B, float* out,
                               void* stream);
/* Per-pixel masks next to a bank (append-only addition, EGO_ABI_VERSION stays 17; ego_ray_bank itself does not change): mask [K][H][W]
 * uint8 dev, one value per pixel of the bank's full images, 0 = ignore, 255 = full weight.  out[i] (float32 [B] dev) = mask / 255 of the
 * pixel idx[i] names (one correctly rounded division).  A row whose index is outside [0, total) reads nothing and is filled with NaN
 * (ego_photo_loss then treats that ray as invalid), as with depth.  The bank's images may be NULL.  B == 0 is a no-op.  One launch. */
int ego_ray_batch_gather_mask(const ego_ray_bank* bank, const uint8_t* mask, const int64_t* idx, int64_t B, float* out, void* stream);

/* ---- camera paths (csrc/ego_camera.hip; append-only additions, EGO_ABI_VERSION stays 17: no existing symbol, struct or argument list
 * changed): the two ends of evaluation_path (renderer.py:199-255) and of the tail of evaluation (renderer.py:141-174) ---- */
enum { EGO_CAM_ERP = 0, EGO_CAM_PINHOLE = 1, EGO_CAM_PINHOLE_BLENDER = 2 };

/* Rays [count][6] (8-byte aligned, dev) of pixels [first, first + count) - row-major pixel index row * W + col - of an H x W image, for the
 * camera-to-world pose c2w: DEVICE memory, [3][4] row-major, read by the kernel, so a captured launch follows a pose that is overwritten
 * between replays (ego_erp_rays takes a host pointer).  A chunk of an image is generated in place: no full-image ray array.
 * EGO_CAM_ERP: get_ray_directions_360 + get_rays (dataLoader/ray_utils.py:24-40, :85-113) with `normalize` as ego_erp_rays; every row has
 *   the bits of the row ego_erp_rays writes for that pixel (one device function computes both).  fx, fy, cx, cy are ignored.
 * EGO_CAM_PINHOLE: get_ray_directions (dataLoader/ray_utils.py:43-61): dir = ((col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, 1); the
 *   reference's default centre is cx = W / 2, cy = H / 2 (the caller passes it).
 * EGO_CAM_PINHOLE_BLENDER: get_ray_directions_blender (dataLoader/ray_utils.py:64-82): the same with y and z negated.
 * Both pinhole models continue with get_rays (dataLoader/ray_utils.py:85-113): d = R dir, o = t, NOT normalised, as there; `normalize` is
 * ignored.  Every operation is rounded on its own in float32, in the reference's order, with true divisions: the camera-space direction has
 * the bits of the float32 torch computation; the three-term dot products are summed left to right ((x R0 + y R1) + z R2) without fused
 * multiply-adds.  count == 0 is a no-op; bad sizes, a window outside the image or a pinhole camera without a finite non-zero focal length
 * return EGO_E_BADARG before anything is queued. */
int ego_camera_rays(int32_t model, int32_t H, int32_t W, float fx, float fy, float cx, float cy, int32_t normalize, const float* c2w,
                    int64_t first, int64_t count, float* rays, void* stream);

/* The frame products of renderer.py:227-240 (evaluation_path) and :141-174 (evaluation) for pixels [first, first + count) of an H x W frame:
 * rgb [count][3], depth [count] float32 dev (the chunk) -> bytes at those pixels' places in whole-frame images (rgb8, depth8 = the FRAME's
 * base pointers; device memory or mapped pinned host memory, whole 4-byte words are written where the images are 4-byte aligned).
 *   colour: rgb8 = (uint8)(clamp(rgb, 0, 1) * 255), float32 multiply, truncation: `(rgb_map.clamp(0, 1).numpy() * 255).astype('uint8')`
 *     (renderer.py:227, :233).
 *   depth index: idx8 = (uint8)(255 * ((nan_to_num(depth) - mi) / den)), every operation rounded on its own in float32:
 *     visualize_depth_numpy (utils.py:14-25), where the host passes mi = float32(near) and den = float32(far - near + 1e-8), the sum formed in
 *     double precision as Python does.
 *   palette: dev [256][3] uint8 or NULL.  With one, depth8 [H W][3] = palette[idx8] (utils.py:26, cv2.applyColorMap: the caller supplies
 *     the table, none is embedded); without, depth8 [H W] = idx8.
 *   side_by_side != 0: rgb8 is the reference's `rgbd` image [H][2 W][3] = concatenate((rgb, depth colours), axis=1) (renderer.py:239);
 *     needs a palette, depth8 is not used.
 * DELIBERATE DEVIATION: an index outside [0, 256) - depth below near or above far - SATURATES to 0 / 255 here.  The reference's
 * float -> uint8 cast is undefined behaviour in C for such values and wraps modulo 256 in numpy on x86 (a depth just above far comes out
 * near 0); a NaN colour likewise becomes 0. */
int ego_finish_frame(const float* rgb, const float* depth, int64_t first, int64_t count, int32_t H, int32_t W, float mi, float den,
                     const uint8_t* palette, int32_t side_by_side, uint8_t* rgb8, uint8_t* depth8, void* stream);

/* ---- stereo panoramas and supersampled frames (csrc/ego_camera.hip; append-only additions, EGO_ABI_VERSION stays 17) ---- */
enum { EGO_EYE_CENTRE = 0, EGO_EYE_LEFT = 1, EGO_EYE_RIGHT = 2 };

/* ego_camera_rays with an eye and ss x ss rays per output pixel (ss = 1..4).
 * H, W, fx, fy, cx, cy describe the FINE camera (the host scales an output frame's size, focal length and centre by ss); first and count
 * address OUTPUT pixels of the (H / ss) x (W / ss) frame, and count ss^2 rays are written: ray p ss^2 + a ss + b is fine pixel
 * (row ss + a, col ss + b) of output pixel first + p = row (W / ss) + col.  The samples of a pixel are contiguous, so any chunk of output
 * pixels resolves on its own (ego_resolve_frame).  Every ray has the bits ego_camera_rays writes for that fine pixel.
 * eye: EGO_EYE_LEFT / EGO_EYE_RIGHT need EGO_CAM_ERP and give the rays of an omnidirectional-stereo panorama.  In the panorama's camera
 *   space (x right, y up, z backward; get_ray_directions_360) pixel column col has phi = (1 - 2 (col + 0.5) / W) pi and the horizontal viewing
 *   direction (-sin phi, 0, -cos phi); the eye sits at o_cam = +-half_ipd (cos phi, 0, -sin phi), + for the right eye (forward x up), and
 *   o = R o_cam + t = (o_cam.x R_r0 + o_cam.z R_r2) + t_r per row r, float32, every operation rounded on its own.  The direction is the
 *   centre eye's, bit for bit.  The offset is not tapered toward the poles.  With eye == EGO_EYE_CENTRE or half_ipd == 0 the origin is t.
 * count == 0 is a no-op; ss outside 1..4, H or W not divisible by ss, an eye other than the centre with a pinhole camera, a negative or
 * non-finite half_ipd and everything ego_camera_rays refuses return EGO_E_BADARG before anything is queued. */
int ego_camera_rays_ex(int32_t model, int32_t H, int32_t W, float fx, float fy, float cx, float cy, int32_t normalize, const float* c2w,
                       int64_t first, int64_t count, int32_t eye, float half_ipd, int32_t ss, float* rays, void* stream);

/* ego_finish_frame for ss x ss samples per pixel: rgb [count ss^2][3], depth [count ss^2] in ego_camera_rays_ex's order; H, W, first, count
 * and the images are the OUTPUT frame's.  Per pixel: colour = (sum over its samples, in order, of clamp(rgb, 0, 1)) / float(ss^2), depth =
 * (sum of nan_to_num(depth)) / float(ss^2) - float32 sums, one true division - then ego_finish_frame's arithmetic, saturation, palette and
 * layouts.  With ss == 1 the bytes are ego_finish_frame's.  One thread per output pixel; whole words are written where ego_finish_frame
 * writes them. */
int ego_resolve_frame(const float* rgb, const float* depth, int64_t first, int64_t count, int32_t H, int32_t W, int32_t ss, float mi,
                      float den, const uint8_t* palette, int32_t side_by_side, uint8_t* rgb8, uint8_t* depth8, void* stream);

/* ---- multi-sphere images (csrc/ego_msi.hip; append-only additions, EGO_ABI_VERSION stays 17) ----
 * A scene baked into L concentric shells of PREMULTIPLIED RGBA around a centre, each an Hm x Wm equirectangular image, and views composited
 * from the shells alone.  A texel is four values (r, g, b, a) of one type: */
enum { EGO_MSI_F32 = 0 /* float32, 16 B per texel */, EGO_MSI_F16 = 1 /* IEEE half, 8 B per texel */ };

/* Per-sample results of N rays -> per-layer premultiplied RGBA.  z [N][S] ascending along every ray (ego_march_density's z_out), alpha
 * [N][alpha_stride] (the march's alpha; alpha_stride 0 = S), rgb [N][S][3] (ego_shade's per-sample colours), bounds [L + 1] ascending, dev.
 * Layer k owns the samples with bounds[k] <= z < bounds[k + 1]; samples outside [bounds[0], bounds[L]) belong to no layer.  Per ray and
 * layer, in sample order, from t = 1: C += (t * alpha_i) * rgb_i, t *= (1 - alpha_i); then A = 1 - t - float32, every operation rounded on
 * its own.  (C.r, C.g, C.b, A) goes to texel first + n of layer k of `layers` [L][texels][4] (texels = Hm Wm; aligned to one texel), as
 * float32 or rounded to the nearest half: one 16-byte or 8-byte store.  A layer without samples writes zeros.  N == 0 is a no-op; bad sizes,
 * an unknown texel type or a window [first, first + N) outside the image return EGO_E_BADARG before anything is queued. */
int ego_msi_layers(const float* z, const float* alpha, int32_t alpha_stride, const float* rgb, int64_t N, int32_t S, const float* bounds,
                   int32_t L, int64_t first, int64_t texels, int32_t texel_type, void* layers, void* stream);

/* Playback: rays [N][6] (origin, direction; 8-byte aligned: what ego_camera_rays writes) -> rgb [N][3], depth [N] float32, what
 * ego_finish_frame / ego_resolve_frame consume.  (cx, cy, cz) the centre, radii [L] ascending (dev), layers [L][Hm][Wm][4] of texel_type,
 * background [Hm][Wm][4] of the same type or NULL.  The direction is normalised first, d = dir / |dir| (exact when |dir| is exactly 1; the
 * pinhole cameras do not normalise their rays).  Per ray, with p = o - c, b = p.d, T = 1, for k = 0 .. L - 1: skip the layer
 * if radii[k] <= |p| (the eye is not inside it); t_k = -b + sqrt(b b - p.p + R_k R_k); u = (p + t_k d) / R_k; theta = asin(clamp(u.y, -1, 1)),
 * phi = atan2(-u.x, -u.z) - the inverse of the EGO_CAM_ERP mapping under an identity pose; row = (1 - 2 theta / pi) Hm / 2 - 0.5,
 * col = (1 - phi / pi) Wm / 2 - 0.5; a bilinear tap (C, A) whose columns wrap modulo Wm and whose rows clamp to [0, Hm - 1];
 * rgb += T C, depth += (T A) (t_k / |dir|) - the GIVEN ray's parameter, as a model reports it - T *= (1 - A).  After the last layer
 * rgb += T * (the background's tap in direction d; its alpha is ignored and taken as 1).  Every layer is visited (no early exit), nothing
 * is clamped; float32 without contraction throughout.  N == 0 is a no-op; bad sizes, an unknown texel type, a NaN centre or misaligned
 * pointers return EGO_E_BADARG before anything is queued. */
int ego_msi_render(const float* rays, int64_t N, float cx, float cy, float cz, const float* radii, int32_t L, int32_t Hm, int32_t Wm,
                   int32_t texel_type, const void* layers, const void* background, float* rgb, float* depth, void* stream);

/* The backward of ego_msi_render for float32 texels (DESIGN.md 3.3 "Refinement"): g_rgb [N][3] = d loss / d rgb -> ADDED into g_layers
 * [L][Hm][Wm][4] and g_background [Hm][Wm][4] (float32; the caller zeroes them; either may be NULL, not both).  The arguments up to `background` are
 * ego_msi_render's; EGO_MSI_F16 is refused.  Per ray, over the live layers with T_k = prod_{j<k} (1 - A_j): dC_k = T_k g,
 * dA_k = -T_k B_{k+1}, B_k = C_k.g + (1 - A_k) B_{k+1}, B_end = C_bg.g (0 without a background), dC_bg = T_end g, the background's alpha
 * gets nothing; each goes to the four taps of the forward with the forward's weights.  Nothing divides by (1 - A_k): T_k of the forward
 * walk is kept in `workspace` (ego_msi_render_backward_workspace_bytes(N, L) = 4 N L bytes, 4-byte aligned, the caller's), so everything
 * behind a layer with A = 1 receives exactly 0.  A skipped layer receives nothing; depth, rays, radii and the centre have no gradient.
 * The adds are float atomics: the sums depend on the order of arrival and are not bit-reproducible.  Four adjacent lanes add the four
 * channels of one texel (values exchanged across the quad).  Hm Wm < 2^31.  N == 0 is a no-op; no host synchronisation; bad arguments
 * return EGO_E_BADARG before anything is queued. */
int64_t ego_msi_render_backward_workspace_bytes(int64_t N, int32_t L);
int ego_msi_render_backward(const float* rays, int64_t N, float cx, float cy, float cz, const float* radii, int32_t L, int32_t Hm, int32_t Wm,
                            int32_t texel_type, const void* layers, const void* background, const float* g_rgb, float* g_layers,
                            float* g_background, void* workspace, int64_t workspace_bytes, void* stream);

/* In place on n_texels float32 texels (16-byte aligned): C <- max(C, 0), A <- clamp(A, 0, 1); a NaN becomes 0.  Run after every optimiser
 * step on an image's texels, it keeps the transmittance of playback inside [0, 1]. */
int ego_msi_project(float* texels, int64_t n_texels, void* stream);

/* Adam that steps only the texels a batch hit, each on its own clock (DESIGN.md 3.3 "Texel Adam"; append-only addition, EGO_ABI_VERSION
 * stays 17).  texels and grad [n_texels][4] float32, moments [n_texels][2][4] float32 - m, then v, of one texel in one 32-byte record - all
 * 16-byte aligned; hits [n_texels] int32: how many steps each texel has taken; bias [n_bias][2] float32, dev, 8-byte aligned: entry t - 1 is
 * {1 - beta1^t, sqrt(1 - beta2^t)}, evaluated in float64 by the caller and rounded once.  A texel whose four gradient values all compare
 * equal to 0 is UNTOUCHED: its texel, moments and count keep their bits, and it is not projected.  Every other texel (a NaN gradient
 * included) takes, on all four channels, float32 without contraction: t = ++hits (saturating at 2^31 - 1); m = beta1 m + (1 - beta1) g;
 * v = beta2 v + ((1 - beta2) g) g; c = bias[min(t, n_bias) - 1]; p = p - ((lr / c.x) m) / (sqrt(v) / c.y + eps) - torch.optim.Adam's rule
 * and order at step t.  With EGO_TEXEL_ADAM_PROJECT the new texel is then clamped as ego_msi_project clamps (the same device function);
 * with EGO_TEXEL_ADAM_ZERO_GRAD its gradient is stored as zeros, so that after the call no gradient value is non-zero, without a memset.
 * One lane per texel, no atomics (bit-reproducible), no host synchronisation (capturable).  n_texels == 0 is a no-op; null or misaligned
 * pointers, n_bias < 1, betas outside [0, 1), eps <= 0, unknown flag bits or n_texels >= 2^39 (ego_msi_project's limit; the strided
 * launch here has none of its own) return EGO_E_BADARG before anything is queued. */
enum { EGO_TEXEL_ADAM_PROJECT = 1, EGO_TEXEL_ADAM_ZERO_GRAD = 2 };
int ego_msi_adam_step(float* texels, float* grad, float* moments, int32_t* hits, int64_t n_texels, float lr, float beta1, float beta2,
                      float eps, const float* bias, int32_t n_bias, int32_t flags, void* stream);

int ego_from_cartesian(const ego_scene* sc, const float* xyz, int64_t M, float* c7, void* stream);
int ego_normalize_coord(const ego_scene* sc, const float* c7, int64_t M, float* c7n, void* stream);

/* c7n [M][7] normalised yin-yang coordinates; out [M].  coarse != 0 uses sc->density_coarse. */
int ego_density_feature(const ego_scene* sc, const float* c7n, int64_t M, int32_t coarse, float* out, void* stream);
/* out [M][app_dim] */
int ego_app_feature(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream);
int ego_feature2density(const ego_scene* sc, const float* feat, int64_t M, float* sigma, void* stream);
/* sigma, dist [N][S] (dist already multiplied by distance_scale, like the reference call site);
 * alpha, weight [N][S]; bg_weight [N].  tensorBase.py:22-27.  alpha = 1 - exp(-sigma * dist) is evaluated as -expm1(-sigma * dist),
 * the correctly rounded value of that expression (the literal float32 form loses ~6e-8 absolute in the subtraction; the fused
 * march does the same) */
int ego_raw2alpha(const float* sigma, const float* dist, int64_t N, int32_t S, float* alpha, float* weight,
                  float* bg_weight, void* stream);
/* viewdirs [M][3], feat [M][app_dim] -> rgb [M][3] */
int ego_mlp_fea(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, float* rgb, void* stream);
/* models/tensorBase.py:30-34 SHRender with models/sh.py:87-112 (degree-2 real spherical harmonics):
 * rgb[m][c] = relu(sum_k Y_k(viewdirs[m]) * features[m][9c + k] + 0.5), features [M][27]. */
int ego_sh_render(const float* viewdirs, const float* features, int64_t M, float* rgb, void* stream);
/* z [N][Sc] coarse distances, weight [N][Sc] coarse weights (bins = midpoints of z, pdf = weight[1:-1]),
 * u [N][n_fine] or NULL (= linspace(0,1,n_fine), eval mode).  use_coarse != 0: z_out [N][Sc+n_fine] =
 * sort(cat(z, z_new)); else z_out [N][n_fine] = sort(z_new).  z_new_out [N][n_fine] optional (unsorted). */
int ego_sample_pdf_merge(const float* z, const float* weight, const float* u, int64_t N, int32_t Sc, int32_t n_fine,
                         int32_t use_coarse, float* z_out, float* z_new_out, void* stream);
int ego_envmap_radiance(const ego_scene* sc, const float* dirs, int64_t N, float* out, void* stream);
/* 2x average pooling of one channel-last plane [H][W][C] -> [H/2][W/2][C] (W==1: line [H][C] -> [H/2][C]) */
int ego_avgpool_table(const float* src, int32_t H, int32_t W, int32_t C, float* dst, void* stream);
/* the same for all 12 tables of a field in one launch (EgoNeRF.py:124-133 update_coarse_sigma_grid, called after every training
 * step when resampling): dst->res must be src->res / 2 per axis, dst's tables allocated by the caller */
int ego_avgpool_field(const ego_vm_field* src, const ego_vm_field* dst, void* stream);
/* 8-tap occupancy lookup of YinYangAlphaGridMask.sample_alpha (models/EgoNeRF.py:19-24): c7n [M][7] -> out [M] (the
 * trilinear mask value; > 0 means occupied). */
int ego_alpha_mask_sample(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream);
/* reference-layout basis/MLP weights in `sc` -> packed blob (dev, ego_packed_floats_scene(sc) floats) */
int ego_pack_mlp(const ego_scene* sc, float* packed_out, void* stream);
/* the same with a choice of what is written: for_training != 0 writes only the regions the differentiable path reads (the fp32 and
 * fp16-split fragment layouts and the basis fragments) and leaves the f16f8 / f16f6 inference images of the blob untouched - a training
 * step re-packs after every optimiser step and never reads them (a memset and three kernels saved per step).  A scene packed this way
 * must be shaded with EGO_PREC_F16X3 or EGO_PREC_F32.  ego_pack_mlp(sc, out, st) == ego_pack_mlp_for(sc, out, 0, st). */
int ego_pack_mlp_for(const ego_scene* sc, float* packed_out, int32_t for_training, void* stream);
/* The fp32 compatibility layout (what ego_packed_floats_scene / ego_pack_mlp produce for a non-tuned shape) for ANY supported shape,
 * the tuned one included: a scene whose `packed` points at this blob can be trained through ego_shade_train_generic /
 * ego_shade_backward_generic / ego_scatter_generic, i.e. with fp32 activations, fp32 dumps and fp32 weight-gradient operands like the
 * reference's autograd (train.py:312-314) - the parity mode beside the tuned training path, whose x / h1 / h2 dumps and dh1 / dh2 are
 * halves (weight gradients carry ~2^-12 relative error per operand, activations above 65504 are not representable). */
int64_t ego_packed_floats_compat(const ego_scene* sc);
int ego_pack_mlp_compat(const ego_scene* sc, float* packed_out, void* stream);

/* ---- the fused hot path ------------------------------------------------------------------------ */

/* Sampling -> yin-yang coords -> density lookup -> sigma -> alpha, transmittance scan.
 * z_in [N][S] explicit sample distances, or NULL: z = near + r_sched[s] (+ jitter).  coarse bit 0 selects the
 * pooled tables, bit 1 the fine-pass radius LUT (ego_scene.r_lut_fine, if set).  Outputs (any may be NULL): z_out [N][S], alpha [N][alpha_stride] (alpha_stride 0 = S;
 * columns S.. are filled with 1, the reference's trailing ones column when an envmap is present,
 * EgoNeRF.py:587), weight [N][S], bg_weight [N], coords_out [N][S][4] = normalised (r, theta, phi) of the sample's
 * grid + is_yang flag (what ego_shade needs; saves it the acos/atan2/LUT search), sigma_out [N][S] (kept for the
 * backward pass), tile_active [ceil(N*S/32)] bytes: 1 for every 32-sample tile that holds a weight above the shading
 * threshold, 0 otherwise (lets ego_shade skip tiles that are fully masked / terminated).  When S is a multiple of 32 every
 * flag is written; otherwise tiles straddle rays, flags are only ever set to 1 and the caller must zero them first. */
int ego_march_density(const ego_scene* sc, const float* rays, int64_t N, int32_t S, const float* z_in,
                      const float* r_sched, const float* jitter, float near_, int32_t coarse, float* z_out,
                      float* alpha, int32_t alpha_stride, float* weight, float* bg_weight, float* coords_out, float* sigma_out,
                      uint8_t* tile_active, void* stream);

/* The node grid behind ego_scene.density_dense / density_coarse_dense (csrc/ego_dense.hip; append-only addition, EGO_ABI_VERSION stays
 * 17; no reference counterpart): for a 16-component field f, out [grid][N_phi][N_theta][N_r][4] float32 (dev, 16-byte aligned,
 * 2 * N_r * N_theta * N_phi * 16 bytes < 4 GB) = (G_0, G_1, G_2, 0) with G_i = sum over c of plane[g][i][node] * line[g][i][node], the
 * plane and line of lookup i read at the voxel's own indices along the axes they span.  The feature of EgoNeRF.compute_densityfeature
 * (models/EgoNeRF.py:291-347), sum_i relu(sum_c bilerp(plane_i,c) * lerp(line_i,c)), is then sum_i relu(trilerp(G_i)): the plane and the
 * line interpolate on one lattice along independent axes.  One thread per voxel; the sum over c runs in ascending order as one chain of
 * fused multiply-adds from 0 (acc = fma(plane_c, line_c, acc), float32), so a bake is a pure function of the tables. */
int ego_bake_density_dense(const ego_vm_field* f, float* out, void* stream);

/* The node grid behind ego_scene.app_f16 = EGO_APP_DENSE (csrc/ego_dense.hip; append-only addition, EGO_ABI_VERSION stays 17; no reference
 * counterpart).  The appearance feature of EgoNeRF.compute_appfeature (models/EgoNeRF.py:349-413) is basis_g . concat_i(bilerp(plane_i)
 * * lerp(line_i)); plane and line interpolate on one lattice along independent axes and the basis is linear, so it is the trilinear
 * interpolation of F[g][phi][theta][r][27] = basis_g . concat_i(plane_i[node] * line_i[node]), zero padding included.
 * f: the 48-component appearance field; basis_yin / basis_yang: the two [27][144] row-major basis matrices (ego_scene.basis); app_dim
 * must be 27.  out (dev, 16-byte aligned, 2 * N_r * N_theta * N_phi * 128 bytes < 4 GB): [grid][N_phi][N_theta][N_r][8 quads][4] float32, r
 * fastest.  A node's 128 bytes: quad 2 q + h holds slots 4 q .. 4 q + 3 of lane half h, and slot s of half h is feature 2 s + h (14 + 13
 * features); i.e. feature f sits at float (2 ((f >> 1) >> 2) + (f & 1)) * 4 + ((f >> 1) & 3) of its node.  The five floats that hold no
 * feature are exactly 0.  Arithmetic: the 144 products plane * line are exact in float64; each feature is one chain of 144 float64 fused
 * multiply-adds acc = fma(basis[f][k], product_k, acc) from 0 in the order k = 48 i + c, rounded to float32 once.  Refused before any
 * launch: n_comp != 48, app_dim != 27 (EGO_E_UNSUPPORTED); a grid of 4 GB or more, an out that is not 16-byte aligned (EGO_E_BADARG). */
int ego_bake_app_dense(const ego_vm_field* f, const float* basis_yin, const float* basis_yang, int32_t app_dim, float* out, void* stream);

/* Per-sample activations the training forward keeps for the backward pass (all dev).  Logical matrices x [M][160] (layer-1
 * inputs), h1, h2 [M][128] (post-ReLU hidden activations), v [M][144] (plane x line products); element kk of lane half h
 * is logical column 8 (kk / 4) + 4 h + kk % 4 (ego_train_layout() maps columns to the reference's inputs / units).  Storage
 * is tile-blocked, lane-major, whole tiles (each buffer needs ceil(M / 32) * 32 rows):
 *   v: fp32 [tile = m / 32][quad pair q = column / 8][lane = 32 h + m % 32][4 floats] (float offset tile * 32 * width + q * 256 +
 *      (32 h + m % 32) * 4 + c);
 *   x, h1, h2: IEEE halves, rounded to nearest, in the MFMA operand order of the kernels themselves: [tile][k-step s][lane][8], element
 *      e = logical column 8 (2 s + e / 4) + 4 h + e % 4 - they only feed the weight-gradient sums (sum over samples of dh * x: the
 *      2^-12 rounding is unbiased and averages out; pinned by the gradient goldens), at half the bytes of fp32 (round 4: the training
 *      step is bound by its dump traffic).  What the DATA gradients need of the forward stays exact: the ReLU masks (relu_bits) and
 *      the feature slots in fp32 (fe).
 * ego_weight_grad reads these layouts directly (a_layout / b_layout).  relu_bits [ceil(M / 32)][2 (h1, h2)][64 lanes][2] uint32 holds the ReLU masks of
 * the two hidden layers (bit 16 (t & 1) + r of word t >> 1 of lane 32 h + m % 32 <=> unit 32 t + slot_row(r, h) of sample m is
 * > 0): all the shade backward needs of h1 / h2 (autograd of torch.nn.ReLU, tensorBase.py:68-71), 32 B instead of 1 KB per sample. */
typedef struct ego_shade_dump {
  uint16_t* x;   /* optional (NULL: not written): only d(W1) reads it, and ego_weight_grad_x re-derives it from `fe` and the rays */
  uint16_t* h1;
  uint16_t* h2;
  float* v;      /* optional since v15 (NULL: not written): only d(basis) reads it, and ego_scatter_app_sorted(dfe, gbasis) takes that product along */
  uint32_t* relu_bits;
  float* fe;   /* [ceil(M / 32)][4][64 lanes][4] fp32: the 16 feature slots of lane 32 h + m % 32 (basis output, slot r = feature 2 r + h);
                * the backward re-derives the encodings' sines and cosines from them with the forward's own instructions */
} ego_shade_dump;

/* Static facts about the shade kernel that implements `precision` (EGO_PREC_*), for roofline accounting by a caller that times it
 * (bench.py): out[0] samples per tile (one wave-level unit of work), [1] fp16 / fp32-input MFMA instructions per tile of samples
 * that lie in one grid, [2] block-scaled fp8 / fp6 MFMA instructions per tile, [3] flop per instruction of [1], [4] flop per
 * instruction of [2], [5] f32 -> fp8 conversion instructions (F16F6: 32-value fp6 conversions) per lane and tile, [6] algorithmic flop per sample (basis +
 * MLP_Fea of tensorBase.py:54-78: 2 (144 x 27 + 150 x 128 + 128 x 128 + 128 x 3)), [7] gathered appearance tap bytes per
 * sample (EgoNeRF.py:349-413: 3 x (4 + 2) taps x 48 channels x 4 B).  n must be 8.  The counts are computed from the same
 * constants the kernel's loops run over. */
int ego_shade_kernel_info(int32_t precision, int32_t* out, int32_t n);

/* Appearance lookup -> basis -> positional encoding -> MLP for every sample: rgb [N][S][3].
 * z [N][S] sample distances (from ego_march_density); coords [N][S][4] optional (ego_march_density's coords_out),
 * NULL = recompute the yin-yang coordinates from rays and z. */
int ego_shade(const ego_scene* sc, const float* rays, const float* z, const float* coords, int64_t N, int32_t S, float* rgb,
              const ego_shade_dump* dump /* NULL for inference */, const uint8_t* tile_active /* NULL = shade every tile */,
              void* stream);

/* ego_shade + ego_composite as ONE launch (rows F, G, H, J; EgoNeRF.py:555-598): the shade kernel's waves own whole rays and finish the
 * pixel in their epilogue, no per-sample colours are written.  For the tuned model shape with fp32 tables, a split-precision arithmetic
 * (not EGO_PREC_F32), weight_thres <= 0 and S a multiple of 32 (EGO_E_UNSUPPORTED otherwise: call ego_shade + ego_composite); coords
 * is required.  Sums run in a different order than ego_composite's (per lane over the ray's tiles, then across 32 lanes): equal to it
 * within fp32 rounding of the sums, not bit for bit.  3.5 % faster than ego_shade alone since round 5 (the folded kernel has the registers
 * to load a plane's basis fragments ahead of the next plane's taps), so ego_render_forward takes it by default where it applies and
 * where its ray-granular deal of the work is balanced (ego_render_forward_folds below); it also saves the [N][S][3] colour buffer. */
int ego_shade_composite(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* weight,
                        const float* bg_weight /* NULL without an envmap */, int64_t N, int32_t S,
                        const uint8_t* tile_active /* NULL = shade every tile */, float* rgb_map, float* depth /* may be NULL */,
                        float* bg_map /* may be NULL */, float* env_map /* may be NULL */, void* stream);

/* 1 iff ego_render_forward shades and composites N rays x S samples of this scene in ONE launch (ego_shade_composite): the scene
 * qualifies (above) and whole rays divide evenly enough over the kernel's waves (critical path within 3 % of the tile-granular
 * ego_shade's: 4096 x 512 and 16384 x 256 fold, 333 or 4097 rays do not).  Environment: EGO_RENDER_FOLD=0 never folds, =1 folds
 * whenever the scene qualifies.  No device work. */
int32_t ego_render_forward_folds(const ego_scene* sc, int64_t N, int32_t S);

/* 1 iff ego_render_forward renders N rays x S samples of this scene in ONE launch: the folded dense shade kernel whose waves march the
 * rays they are about to shade themselves, ahead of their tiles, into the workspace slots ego_march_density fills (same bits; coords
 * behind an exactly opaque prefix are zeros, as in the one-wave march).  Taken without resampling when ego_render_forward_folds holds,
 * the scene carries both baked grids (density_dense and the dense appearance grid) at one resolution, 16 density components, no mask,
 * no term_eps, weight_thres <= 0 (with weight_thres = 0, the exact skip of all-zero tiles, the kernel writes and reads the tile flags
 * itself), and the compact path is not taken.  The answer is for a call WITHOUT ego_render_args.marched: a call that passes that event
 * keeps the march a launch of its own, so that the event stays behind the march and ahead of the shade.  Environment:
 * EGO_RENDER_MARCH=0 keeps the two launches (read per call).  No device work. */
int32_t ego_render_forward_marches(const ego_scene* sc, int64_t N, int32_t S);

/* 1 iff ego_render_forward shades only the LIVE samples of N rays x S samples of this scene - weight > max(weight_thres, 0), the
 * app_mask of TensorBase.forward (models/tensorBase.py:480-487), which runs the appearance lookup and the MLP on coords_sampled[app_mask]
 * only - instead of the 32-sample tiles of the flat [N][S] order that hold one: it builds the list of those samples (ray-major, no
 * atomics, no host synchronisation, inside the workspace), shades tiles cut from the list and composites with ego_composite; same bits.
 * Taken for the tuned shape with weight_thres >= 0 when the call can leave dead samples INSIDE rays (an occupancy mask, or
 * weight_thres > 0); with the exact skip alone the dead samples are ray tails, which the tile skip already passes over.  Environment:
 * EGO_RENDER_COMPACT=0 never compacts, =1 compacts whenever the shape is the tuned one and weight_thres >= 0.  No device work. */
int32_t ego_render_forward_compacts(const ego_scene* sc, int64_t N, int32_t S);

/* acc, rgb_map (+ envmap background), clamp, depth (+ (1-acc)*d_z quirk, EgoNeRF.py:598).
 * Outputs rgb_map [N][3], depth [N]; bg_map/env_map [N][3] written only when sc->envmap != NULL (may be NULL);
 * rgb_raw [N][3] optional = rgb_map before the clamp (the backward pass needs the clamp mask). */
int ego_composite(const ego_scene* sc, const float* rays, const float* z, const float* weight, const float* bg_weight,
                  const float* rgb, int64_t N, int32_t S, float* rgb_map, float* depth, float* bg_map, float* env_map,
                  float* rgb_raw, void* stream);

/* ---- training step: backward of the path (autograd of EgoNeRF.forward, train.py:312-314) ---------
 * Table gradients are accumulated with float atomics straight into channel-last gradient tables (same layout as the
 * parameters; the caller zeroes them).  Weight gradients of the basis / MLP are left to the caller as plain GEMMs over
 * the per-sample buffers these kernels write (lane order; ego_train_layout gives the column maps). */
typedef struct ego_vm_grad {
  float* plane[2][3]; /* dev, [H][W][C] like the parameter */
  float* line[2][3];
} ego_vm_grad;

int64_t ego_train_packed_floats(void);
/* transposed fp16-split fragments of W2, W1, the basis matrices and W3 for the data-gradient chain */
int ego_pack_train(const ego_scene* sc, float* out, void* stream);
/* which = 0: x column [160] -> MLP input column | 1: hidden column [128] -> unit | 2: dfe column [32] -> feature |
 * 3: v column [144] -> basis input column; -1 marks padding.  Host memory. */
int ego_train_layout(int32_t which, int32_t* out, int32_t n);
/* compositing backward (autograd of EgoNeRF.py:579-593 and tensorBase.py:22-27,415-419).
 * g_rgb [N][3] = dL/d rgb_map, rgb_raw = rgb_map before the clamp, env_map [N][3] or NULL.  alpha has row stride
 * alpha_stride (S, or S+1 when the envmap's ones column is appended); g_alpha = dL/d alpha with the same stride or NULL
 * (train.py:306-309 ray_entropy_loss).  depth_map carries no gradient in the reference (computed under no_grad,
 * EgoNeRF.py:595-598).  Writes dc [N][S][3] = dL/d rgb_sample and dfeat [N][S] = dL/d(density feature) (the per-plane relu
 * mask of EgoNeRF.py:340,346 is applied by ego_scatter_density). */
int ego_march_backward(const ego_scene* sc, const float* z, const float* alpha, int32_t alpha_stride, const float* weight,
                       const float* sigma, const float* bg_weight, const float* rgb, const float* g_rgb, const float* g_alpha,
                       const float* rgb_raw, const float* env_map, int64_t N, int32_t S, float* dc, float* dfeat, void* stream);
/* shade backward: dc [N][S][3] in = dL/d rgb_sample, out = dL/d(pre-sigmoid).  Writes dh2, dh1 (logical [M][128]), dfe [M][32]
 * (the feature-slot gradients of the sample's OWN grid; ego_weight_grad's a_layout 3 routes them by coords.w) and dv = dL/d(plane x line products).  dh2 / dh1 are stored as SCALED fp16 in the order the kernel's own
 * matrix products consume them: [tile = m / 32][k-step s = 0..7][lane = 32 h + m % 32][8 halves], element e = logical column
 * 8 (2 s + e / 4) + 4 h + e % 4 (the column numbering of the forward's dumps), value = half * dh_scale[row][m] with dh_scale
 * [2][ceil(M / 32) * 32] per-sample powers of two (row 0: dh2, row 1: dh1) chosen so that a sample's largest magnitude lies in
 * [2^12, 2^13): 11 significant bits, rounded to nearest, half the bytes of fp32 (ego_weight_grad's a_layout 2 reads it).  dv is
 * [tile][plane * 3 + line][sample][16 channels] fp32 (it feeds single table texels, where fp16 rounding would show); all three
 * need ceil(M / 32) * 32 rows.  Reads fwd->fe and fwd->relu_bits only. */
int ego_shade_backward(const ego_scene* sc, const float* train_packed, const float* coords, float* dc, const float* rgb,
                       const ego_shade_dump* fwd, uint16_t* dh2, uint16_t* dh1, float* dh_scale, float* dfe, float* dv, float* dv_absmax,
                       int64_t N, int32_t S, void* stream);
/* dv_absmax (v15; dev, one float, may be NULL): receives max |dv| over the valid samples (NaN if a sample's gradient is not finite) - the
 * bound ego_scatter_app_sorted derives the fixed-point unit of its line sums from, so that it need not read dv once more to find it. */
/* backward of the VM lookups (autograd of F.grid_sample in EgoNeRF.py:291-347 / :349-413): accumulates into the gradient
 * tables (same channel-last layout as the parameters).  coords [N][S][4] = the forward's normalised (r, theta, phi, grid). */
int ego_scatter_density(const ego_scene* sc, const ego_vm_grad* gdensity, const float* coords, const float* dfeat, int64_t N, int32_t S,
                        void* stream);
int ego_scatter_app(const ego_scene* sc, const ego_vm_grad* gapp, const float* coords, const float* dv, int64_t N, int32_t S,
                    void* stream);

/* ---- the same table gradients without atomics: bit-reproducible (the sort: csrc/ego_scatter_sort.hip; the scatters: csrc/ego_scatter_sorted.hip) ----
 * ego_scatter_density / ego_scatter_app add with float atomics: their sums depend on the order the hardware serves them.  The three
 * entry points below bin the step's samples by texel cell once (three stable radix sorts of the forward's coordinates; both fields share
 * them) and then write every gradient texel exactly once from sums taken in a fixed order: two calls return the same bits, no zero fill
 * of `grad` is needed, and there is no atomic traffic (they are also faster: DESIGN.md 4.2).  Same mathematics as F.grid_sample's
 * backward in compute_densityfeature / compute_appfeature (models/EgoNeRF.py:291-347, :349-413) under train.py:312-314; same argument
 * meaning as ego_scatter_density / ego_scatter_app.  `workspace` (dev, 256-byte aligned, ego_scatter_sorted_workspace_bytes(sc, N, S)
 * bytes; -1 = bad arguments) carries the sort from ego_scatter_sort to the two scatters and holds their scratch: calls that share a
 * workspace must be ordered on one stream (or by events).  The density and appearance fields must have one resolution. */
int64_t ego_scatter_sorted_workspace_bytes(const ego_scene* sc, int64_t N, int32_t S);
int ego_scatter_sort(const ego_scene* sc, const float* coords, int64_t N, int32_t S, void* workspace, int64_t workspace_bytes, void* stream);
int ego_scatter_density_sorted(const ego_scene* sc, const ego_vm_grad* gdensity, const float* coords, const float* dfeat, int64_t N, int32_t S,
                               void* workspace, int64_t workspace_bytes, void* stream);
int ego_scatter_app_sorted(const ego_scene* sc, const ego_vm_grad* gapp, const float* coords, const float* dv, const float* dv_absmax,
                           const float* dfe, float* gbasis, int32_t ldg, int64_t N, int32_t S, void* workspace, int64_t workspace_bytes,
                           void* stream); /* dv: ego_shade_backward's blocked layout */
/* dfe / gbasis (v15; both or neither; NULL = as before): the basis gradient rides along as well.  d(basis_mat)[slot][plane x 48 + channel] =
 * sum over samples of dfe[s][slot] x (plane value x line value)[s][channel] - and the walk has both factors of that product in registers,
 * so the forward need not dump v (ego_shade_dump.v = NULL: 576 B per sample less to write) for ego_weight_grad to read it back.  dfe =
 * ego_shade_backward's [M][32] (the sample's own grid's slots); gbasis [64][ldg >= 144] receives row 32 g + slot, column plane x 48 +
 * channel (reference channel order), written, not accumulated; bf16 hi / lo split MFMA (three terms, ~16 significand bits per operand), per-wave partial products added
 * in a fixed order (bit-reproducible).  Only in the walk form (EGO_E_UNSUPPORTED with EGO_SORTED_WALK=0). */
/* dv == NULL (v16; needs dfe, gbasis, dv_absmax and sc->basis): the walk re-derives dv = basis_g^T dfe for its own plane's 48 channels (the
 * 27 feature-slot gradients of a sample are 128 B where its dv is 576 B) in ego_shade_backward's own arithmetic for that product (operands scaled
 * by a power of two per sample / per channel, fp16 hi + lo, three MFMA terms, fp32 accumulation), so ego_shade_backward
 * need not write dv at all (pass it dv = NULL: its dv_absmax then carries max |dfe|, which is what this call expects in that case - the
 * fixed-point unit comes from max |dfe| x the largest column sum of |basis|).  A sample's dv differs from ego_shade_backward's by the
 * rounding of that arithmetic (~2^-21 per product; the fp32 summation order over the 27 slots differs).  The padding columns of dfe (slots
 * 14, 15 of either half and feature 27) meet zero weights here and must be finite, as ego_shade_backward writes them (zeros). */
/* v15: ONE pass over dfeat / dv.  The gradient of a plane and of the line it is multiplied with (the table of the axis that is not in the
 * plane) come out of the same walk over the plane's cells: a cell's samples share the four plane texels, so the line's contribution of a
 * sample is four multiply-adds away - but it lands in an arbitrary line texel.  Those sums are therefore taken in 64-bit FIXED POINT
 * (integer LDS atomics per workgroup, integer partial tables added at the end: integer addition is associative, any order returns the same
 * bits).  The unit is one power of two per table: 2^k with k = e(max |d|) + e(max |plane texel|) + 1 - nbits, nbits = min(50, 62 -
 * ceil(log2(N S))), i.e. >= 40 bits below the largest possible contribution at 2^21 samples (an fp32 sum keeps 24 bits below its running
 * value; a contribution more than ~2^-40 below the table's largest possible one is rounded to the unit).  max |plane texel| is taken by
 * the call itself; max |dfeat| too; dv_absmax (dev, one float, may be NULL = computed here by one more read of dv) is ego_shade_backward's.
 * Non-finite inputs give NaN line gradients.  Line tables too large for the LDS (axis > ~1 200 texels) and EGO_SORTED_LINES=separate take
 * the two-pass form of v14 (float partial sums of fixed 256-sample sub-blocks, added in sub-block order).  An empty batch (N = 0)
 * zero-fills the tables. */
/* d(envmap.emission) [3][2h][h] += backward of bg_weight * sigmoid(bilinear(emission, dir)) (envmap.py:26-34,
 * EgoNeRF.py:588-590).  dirs = N directions dir_stride floats apart (rays + 3 with stride 6, or a packed [N][3]);
 * env_map = the forward's radiance [N][3]; the clamp mask is taken from rgb_raw (pass values in [0,1] for none). */
int ego_envmap_backward(const ego_scene* sc, const float* dirs, int32_t dir_stride, const float* g_rgb, const float* rgb_raw, const float* bg_weight,
                        const float* env_map, int64_t N, float* g_emission, void* stream);
/* Weight gradients of nn.Linear layers over all samples: G [32 ceil(ca/32)][ldg] += A^T B for A (M rows, ca <= 128 columns
 * used of lda) and B (M rows, cb <= 160 of ldb), G accumulated (zero it first).  a_layout 0: row-major fp32 | 1: fp32 in the
 * shade kernels' dump layout [tile = m / 32][quad pair q][lane = 32 h + m % 32][4] with logical column 8 q + 4 h + c
 * (ceil(M / 32) * 32 rows allocated) | 2: ego_shade_backward's scaled-fp16 layout (ca = lda = 128, a_scale [M] = that matrix's
 * row of dh_scale) | 3: row-major fp32 [M][32] standing for 64 logical columns, row m filling columns [32 g, 32 g + 32) with
 * g = (a_scale[4 m + 3] != 0) (ego_shade_backward's dfe; ca = 64, lda = 32, a_scale = the forward's coords [M][4]); a_scale NULL for
 * layouts 0 / 1.  b_layout 0: row-major fp32 | 1: fp32 in the dump layout (ego_shade_dump.v) | 2: halves in the dump layout of
 * ego_shade_dump's x / h1 / h2 ([tile][k-step][lane][8]; cb a multiple of 16, ldb = cb).  ones_col >= 0 replaces that column
 * of B by ones (it may lie beyond cb, < 160), which yields the bias gradient = column sums of A in G[:, ones_col].  bf16 hi/lo
 * split MFMA, ~17 significand bits per operand. */
int ego_weight_grad(const void* A, int32_t lda, int32_t ca, int32_t a_layout, const float* a_scale, const void* B, int32_t ldb,
                    int32_t cb, int32_t b_layout, int32_t ones_col, int64_t M, float* G, int32_t ldg, void* stream);
/* The same product, bit-reproducible: every workgroup stores its partial product block to `partial` (dev, ego_weight_grad_partial_floats()
 * floats) and a second kernel adds the blocks in workgroup order and STORES the result (G needs no zero fill; rows [0, 32 ceil(ca/32)) x
 * columns [0, 32 ceil(cols/32)) of G are overwritten - EXCEPT on the d(W3) fast path (ca == 3, cb == 128, b_layout 2: the VALU kernel
 * k_wgrad3), which writes rows [0, 3) x columns [0, 160) only and leaves the padding rows 3..31 as they were: zero G once if those rows
 * are read).  ego_weight_grad adds with float atomics: its sums depend on the order the
 * hardware serves them (differences in the last bits from run to run).  partial = NULL is ego_weight_grad. */
int64_t ego_weight_grad_partial_floats(void);
/* d(W1) and d(b1) of the tuned head WITHOUT the x dump: G [128][ldg >= 160] = dh1^T [x | 1] where x - the MLP input of
 * tensorBase.py:68-75 in the shade kernels' column order - is re-derived per sample from the forward's feature-slot dump
 * (ego_shade_dump.fe) and the ray's view direction (rays [N][6], sample m belongs to ray m / S) with the forward's own instructions and
 * rounding, i.e. the operands are bit-identical to ego_weight_grad(dh1, .., a_layout 2, x dump, b_layout 2, ones_col) and
 * ego_shade_dump.x may be NULL in the training forward (320 B per sample less to write, 192 B less to read).  dh1 / dh_scale as
 * ego_shade_backward writes them; ones_col = the zero-padding column that yields the bias gradient; partial as in ego_weight_grad_det
 * (NULL = float atomics into a zeroed G). */
int ego_weight_grad_x(const void* dh1, const float* dh_scale, const float* fe, const float* rays, int32_t S, int32_t ones_col, int64_t M, float* G,
                      int32_t ldg, float* partial, int64_t partial_floats, void* stream);
int ego_weight_grad_det(const void* A, int32_t lda, int32_t ca, int32_t a_layout, const float* a_scale, const void* B, int32_t ldb, int32_t cb,
                        int32_t b_layout, int32_t ones_col, int64_t M, float* G, int32_t ldg, float* partial, int64_t partial_floats,
                        void* stream);

/* ---- training of model shapes other than the tuned one (opt.py:87-100 lets a user choose n_lamb_sigma / n_lamb_sh, data_dim_color,
 * featureC, view_pe, fea_pe; supported shapes as for ego_packed_floats_scene).  Plain fp32 compatibility kernels over ROW-MAJOR
 * per-sample buffers, about an order of magnitude slower than the tuned path; ego_march_density / ego_march_backward /
 * ego_composite / ego_weight_grad (a_layout 0, b_blocked 0, 160-column chunks) serve every shape.  Autograd of EgoNeRF.py:349-413 and
 * tensorBase.py:54-78, as train.py:312-314 runs it. ---- */
/* ego_shade for training: rgb [N][S][3] plus the activations the backward needs: x [M][ldx] = the MLP input row in the reference's
 * column order (tensorBase.py:68-75; columns >= mlp_in are not written: zero the buffer), h1 / h2 [M][ldh] = post-ReLU hidden
 * activations, v [M][ldv] = plane x line products (column = plane * n_comp + channel; 16-byte aligned, ldv % 4 == 0). */
int ego_shade_train_generic(const ego_scene* sc, const float* rays, const float* coords, int64_t N, int32_t S, float* rgb, float* x, int32_t ldx,
                            float* h1, float* h2, int32_t ldh, float* v, int32_t ldv, void* stream);
/* dc [M][3] in = dL/d rgb_sample, out = dL/d(pre-sigmoid).  Writes dh2, dh1 [M][mlp_hidden], dfe64 [M][64] (the feature gradients of
 * the sample's own grid g in columns [32 g, 32 g + 32), zeros in the other half: dfe64^T v gives both basis gradients in one
 * product) and dv [M][ldv] = dL/d(plane x line products).  ldv == 0 (48 appearance components only): dv in ego_shade_backward's blocked layout
 * ([ceil(M / 32)][9][32][16] floats), so that the tuned scatters (ego_scatter_app_sorted / ego_scatter_app) serve a model whose HEAD has
 * another shape but whose tables have the shipped one. */
int ego_shade_backward_generic(const ego_scene* sc, const float* coords, float* dc, const float* rgb, const float* x, int32_t ldx, const float* h1,
                               const float* h2, int32_t ldh, float* dh2, float* dh1, float* dfe64, float* dv, int32_t ldv, int64_t N, int32_t S,
                               void* stream);
/* backward of the VM lookups of `field` (any n_comp that is a multiple of 4 up to 48) into `grad` (channel-last like the parameters,
 * accumulated with float atomics).  ldd == 0: d = dfeat [M] from ego_march_backward (density: the per-plane relu mask of
 * EgoNeRF.py:340,346 is applied here); ldd > 0: d = dv [M][ldd] from ego_shade_backward_generic (appearance). */
int ego_scatter_generic(const ego_vm_field* field, const ego_vm_grad* grad, const float* coords, const float* d, int32_t ldd, int64_t N, int32_t S,
                        void* stream);

/* ---- training-step table ops (train.py:245-330).  Tables are channel-last [H][W][C].  `value` (device double, may be
 * NULL) and `grad` (device, same layout as the table, may be NULL) are ACCUMULATED into, so one buffer collects a whole
 * regulariser and gradients add onto the render's. ---- */
/* utils.py:155-171 TVLoss on one plane: value += scale * 2 (sum dH^2 / (C (H-1) W) + sum dW^2 / (C H (W-1)));
 * EgoNeRF.py:214-228 call it with scale = 1e-2 per plane. */
int ego_tv_plane(const float* table, int32_t C, int32_t H, int32_t W, float scale, double* value, float* grad, void* stream);
/* EgoNeRF.py:206-212 density_L1 term of one table: value += scale * mean |x|. */
int ego_l1_table(const float* table, int64_t n, float scale, double* value, float* grad, void* stream);
/* EgoNeRF.py:189-201 vectorDiffs term of one line table [n][C]: value += scale * mean |off-diagonal of L^T L|. */
int ego_line_ortho(const float* line, int32_t C, int32_t n, float scale, double* value, float* grad, void* stream);
/* utils.py:175-183 ray_entropy_loss over alpha [N][S] (row stride `stride`): value += mean_ray H(alpha / (sum alpha + 1e-10)),
 * g_alpha (same stride, WRITTEN) = d value / d alpha. */
int ego_ray_entropy(const float* alpha, int64_t N, int32_t S, int32_t stride, double* value, float* g_alpha, void* stream);
/* Distortion regulariser (Mip-NeRF 360, point-sampled form; not in the reference; append-only addition, EGO_ABI_VERSION stays 17).
 * Sample i of a ray covers [z_i, z_{i+1}] (z_S = z_{S-1} + (z_{S-1} - z_{S-2}): the render's quadrature); the ends are mapped to
 * s in [0, 1] by `space`, m_i and delta_i are the mapped interval's midpoint and width, w_i = alpha_i prod_{j<i} (1 - alpha_j + 1e-10):
 *   value += (1 / N) sum_rays [ sum_i sum_j w_i w_j |m_i - m_j| + (1 / 3) sum_i w_i^2 delta_i ]
 * in O(S) per ray (csrc/ego_reg.hip states the algebra).  alpha [N][alpha_stride] (the first S columns are used: an envmap's trailing
 * ones column does not enter), z [N][S] ascending per ray and constant.  `value`: float64 device scalar zeroed by the caller, or NULL;
 * each ray's term is rounded to a multiple of 2^-51 (at most N 2^-52 absolute in all), which makes the adds exact and the result
 * independent of the order in which the rays arrive.  g_alpha [N][alpha_stride] or NULL: WRITTEN, d value / d alpha,
 * columns at or beyond S as 0, bit-reproducible; it must not overlap alpha.  Requires S >= 2, alpha_stride >= S, finite near_ < far_,
 * near_ > 0 for the log and disparity spaces, a known space, non-null alpha and z, and value or g_alpha; N == 0 is a no-op.  One
 * launch, no allocation, no synchronisation. */
enum { EGO_DIST_LINEAR = 0 /* (z - near) / (far - near) */, EGO_DIST_LOG = 1 /* log(max(z, near) / near) / log(far / near) */,
       EGO_DIST_DISPARITY = 2 /* (1 / near - 1 / max(z, near)) / (1 / near - 1 / far) */ };
int ego_ray_distortion(const float* alpha, int32_t alpha_stride, const float* z, int64_t N, int32_t S, float near_, float far_, int32_t space,
                       double* value, float* g_alpha, void* stream);
/* Depth supervision (train.py:249-251, :275-283: masked MSE between depth_map and a per-ray target; append-only addition, EGO_ABI_VERSION
 * stays 17).  The reference computes depth_map under no_grad (EgoNeRF.py:595-598), so its term adds a number and no gradient; this is the
 * term with its gradient, entering through alpha like the two terms above - the render's depth output stays non-differentiable.  With
 * w_i = alpha_i T_i, T_i = prod_{j<i} (1 - alpha_j + 1e-10), q_i = s(z_i), q_t = s(tail) (0 when tail is NULL):
 *   D = sum_i w_i q_i + (1 - sum_i w_i) q_t,    dD / dalpha_i = T_i (G_i - R_i),  G_i = q_i - q_t,
 *   R_{S-1} = 0, R_i = G_{i+1} alpha_{i+1} + (1 - alpha_{i+1} + 1e-10) R_{i+1}        (no division: alpha = 1 is harmless)
 * s = `space`: EGO_DIST_METRIC (identity: the reference's term; near_ / far_ unused), EGO_DIST_LOG or EGO_DIST_DISPARITY (the maps of
 * ego_ray_distortion; they need finite 0 < near_ < far_).  A ray is valid iff its target is finite and > 0 (the reference's mask is != 0;
 * NaN, inf and negative targets drop out as well); V = the number of valid rays, counted on the device; r = D - s(target):
 *   EGO_DEPTH_L2: value += (1 / V) sum_valid r^2,  g_alpha_i = (2 r / V) dD / dalpha_i
 *   EGO_DEPTH_L1: value += (1 / V) sum_valid |r|,  g_alpha_i = (sign(r) / V) dD / dalpha_i, 0 at r = 0
 * An invalid ray's gradient row is exactly 0; with V = 0 nothing is added to value and every gradient element is exactly 0.
 * alpha [N][alpha_stride], alpha_stride = S or S + 1 (an envmap's trailing ones column takes no part and gets the gradient 0), z [N][S],
 * target [N], tail [N] or NULL: float32 dev, all constant but alpha.  tail = the rays' last component reproduces the render's own
 * depth_map, which adds (1 - sum w) rays[..., -1] (EgoNeRF.py:597).  Outputs, each optional: `value`, a float64 device scalar zeroed by
 * the caller; g_alpha [N][alpha_stride], every element WRITTEN, must not overlap alpha; pred [N] = D of every ray, valid or not.
 * target may be NULL when only pred is asked for.  `workspace`: caller-owned, 8-byte aligned, ego_ray_depth_loss_workspace_bytes(N)
 * = 16 + 8 N bytes (V and one float64 term per ray), needed with value or g_alpha, overwritten, no need to clear it.  Value and gradient
 * are bit-reproducible, and value-only, gradient-only and joint calls return the same bits: every sum has a fixed order.  Refuses
 * S < 2, another alpha_stride, an unknown space or kind, near_ / far_ outside a space's domain, and null arguments; N == 0 is a no-op.
 * Up to three launches, no allocation, no synchronisation: it can be captured into a hipGraph. */
enum { EGO_DIST_METRIC = 3 /* s(z) = z; ego_ray_depth_loss only */ };
enum { EGO_DEPTH_L2 = 0, EGO_DEPTH_L1 = 1 };
int64_t ego_ray_depth_loss_workspace_bytes(int64_t N);
int ego_ray_depth_loss(const float* alpha, int32_t alpha_stride, const float* z, const float* target, const float* tail, int64_t N, int32_t S,
                       float near_, float far_, int32_t space, int32_t kind, void* workspace, double* value, float* g_alpha, float* pred,
                       void* stream);
/* The photometric term for real captures (csrc/ego_photo.hip; append-only addition, EGO_ABI_VERSION stays 17): train.py:261's
 * torch.mean((rgb_map - rgb_train) ** 2) with a per-image affine colour map, a per-ray weight and robust kinds.  With k = image[n]
 * (0 without image), c'_nc = gain[k][c] rgb_nc + bias[k][c] (c' = rgb without affine) and r_nc = c'_nc - target_nc:
 *   EGO_PHOTO_L2: rho = r^2      EGO_PHOTO_HUBER: rho = r^2 / 2 for |r| <= param, else param (|r| - param / 2)
 *   EGO_PHOTO_L1: rho = |r|      EGO_PHOTO_CHARBONNIER: rho = sqrt(r^2 + param^2) - param
 * A ray is valid iff its weight is finite and > 0 (weight NULL: 1), its three target channels are finite, and 0 <= image[n] < K when image
 * is given.  A non-finite rgb of a valid ray is not hidden: it makes the value non-finite, as the MSE would.  W = sum_valid w_n, counted
 * on the device:
 *   value   += (1 / 3W) sum_valid w_n sum_c rho(r_nc)
 *   g_rgb_nc = w_n rho'(r_nc) gain[k][c] / 3W, exactly 0 on an invalid ray; the L1 derivative is 0 at r = 0
 *   g_affine[k][c] = (sum_{n in k, valid} w_n rho'(r_nc) rgb_nc / 3W, the same sum without rgb_nc): d value / d (gain, bias), exactly 0
 *                    for an image no valid ray belongs to
 * With W = 0 nothing is added to value and every gradient element is exactly 0.  Without weight, image and affine, EGO_PHOTO_L2 is the
 * reference's MSE evaluated in float64.
 * rgb [N][3], target [N][3], weight [N] or NULL: float32 dev; image [N] int32 dev or NULL; affine [K][3][2] float32 dev (gain, bias) or
 * NULL (identity); all constant.  Outputs, each optional: `value`, a float64 device scalar zeroed by the caller; g_rgb [N][3] and g_affine
 * [K][3][2] float32, every element WRITTEN.  `workspace`: caller-owned, 8-byte aligned, ego_photo_loss_workspace_bytes(N, K) bytes
 * (K counts only when g_affine is asked for: pass 0 otherwise), overwritten, no need to clear it.  All arithmetic is float64; every sum has
 * a fixed order (per-block partials joined in index order; per image, one block per slice of 2048 rays scanning the slice's image indices,
 * the slices joined in slice order: N K index reads in all), no float atomics: repeated calls return the same bits, and so do value-only,
 * gradient-only and joint calls.  Refuses, before any launch: an unknown kind, a param that is not
 * finite and > 0 for HUBER / CHARBONNIER (unused otherwise), affine or g_affine without image, K < 1 with either, null rgb, target or
 * workspace, no output asked for.  N == 0 is a no-op.  At most three launches, no allocation, no synchronisation: it can be captured
 * into a hipGraph. */
enum { EGO_PHOTO_L2 = 0, EGO_PHOTO_L1 = 1, EGO_PHOTO_HUBER = 2, EGO_PHOTO_CHARBONNIER = 3 };
int64_t ego_photo_loss_workspace_bytes(int64_t N, int32_t K);
int ego_photo_loss(const float* rgb, const float* target, const float* weight, const int32_t* image, const float* affine, int64_t N, int32_t K,
                   int32_t kind, float param, void* workspace, double* value, float* g_rgb, float* g_affine, void* stream);
/* The weighted least-squares affine colour map per image and channel, in closed form: for each (k, c), over the valid rays of image k
 * (ego_photo_loss's rule; image NULL: one image, K must be 1), the (gain, bias) that minimise sum w (gain rgb + bias - target)^2, from the
 * float64 moments W_k, sum w c, sum w t, sum w c^2, sum w c t (one block per image, ego_photo_loss's scan over the whole batch).  An image with
 * W_k = 0 gets (1, 0).  A system is degenerate iff W sum w c^2 - (sum w c)^2 <= 1e-9 W sum w c^2 (all colours equal; a definition, not a
 * tolerance) and gets gain 1, bias mean_w(t) - mean_w(c).  Writes affine [K][3][2] float32 dev and, optionally, Wk [K] float64 dev.
 * Repeated calls return the same bits.  Refuses K < 1, image NULL with K != 1, null affine, null rgb or target with N > 0.  One launch. */
int ego_photo_fit(const float* rgb, const float* target, const float* weight, const int32_t* image, int64_t N, int32_t K, float* affine,
                  double* Wk, void* stream);
/* The structural term on patch batches (csrc/ego_patch_loss.hip; append-only addition, EGO_ABI_VERSION stays 17).  No reference counterpart:
 * its rgb_ssim (utils.py:104-152) is a metric on whole images without a gradient.  rgb, target [>= P ph pw][3] float32 dev hold P patches of
 * ph x pw pixels, row p ph pw + a pw + b = pixel (a, b) of patch p (ego_ray_batch_sample_patches' layout); weight [>= P ph pw] float32 dev
 * or NULL (1); rows behind the patches are not read.  With g = the normalised Gaussian taps of ego_rgb_ssim (utils.py:117-121), per patch,
 * channel and window origin (i, j), 0 <= i <= ph - fs, 0 <= j <= pw - fs, the window moments with weights g_a g_b over x = rgb, y = target:
 *   mux, muy, Exx, Eyy, Exy;  sxx = Exx - mux^2, syy = Eyy - muy^2, sxy = Exy - mux muy;  C1 = (k1 max_val)^2, C2 = (k2 max_val)^2
 *   A1 = 2 mux muy + C1, B1 = mux^2 + muy^2 + C1, A2 = 2 sxy + C2, B2 = sxx + syy + C2, S = A1 A2 / (B1 B2)
 * all sums and products float64 over the float32 inputs; the metric's rounding guards (its clamps of sxx, syy, sxy and its float32 squares)
 * are deliberately absent, so the term is smooth.  A window is valid iff every pixel under it has a finite weight > 0 and three finite target
 * channels (the weight is a gate, not a soft weight); a non-finite rgb under a valid window is not hidden.  M = the number of valid
 * (patch, window) pairs, counted on the device:
 *   *value = 1 - (1 / 3M) sum_valid S   (WRITTEN, not accumulated; 0 when M = 0)
 *   g_rgb[pixel] = -(1 / 3M) sum over the valid windows covering it of g_a g_b (dmu + 2 x dS/dExx + y dS/dExy),  dS/dExx = -S / B2,
 *   dS/dExy = 2 A1 / (B1 B2),  dmu = (A2 / B2)(2 muy B1 - 2 mux A1) / B1^2 + 2 mux S / B2 - 2 muy A1 / (B1 B2)
 * g_rgb [>= P ph pw][3] float32 dev: every element of its first P ph pw rows is WRITTEN, exactly 0 for a pixel under no valid window and
 * everywhere when M = 0; rows behind are not touched.  value (float64 dev) and g_rgb are each optional.  `workspace`: caller-owned, 8-byte
 * aligned, ego_patch_ssim_workspace_bytes(P, ph, pw) bytes (-1 for P < 0 or ph, pw outside 1..32; it does not know filter_size, which
 * ego_patch_ssim checks itself), overwritten, no need to clear it.  One block
 * per patch stages x and y in LDS, takes the moments separably (rows, then columns) and forms the gradient as the transposed separable filter
 * of the three coefficient fields in a fixed tap order; per-patch sums and counts are joined in index order, no atomics: value-only,
 * gradient-only, joint and repeated calls return the same bits.  Envelope: 1 <= filter_size <= 15, filter_size <= ph, pw <= 32.  Refuses,
 * before any launch: a shape outside the envelope, P < 0, a filter_sigma that is not finite and > 0, null rgb, target or workspace, no output
 * asked for.  P == 0 is a no-op.  At most three launches, no allocation, no synchronisation: it can be captured into a hipGraph. */
int64_t ego_patch_ssim_workspace_bytes(int64_t P, int32_t ph, int32_t pw);
int ego_patch_ssim(const float* rgb, const float* target, const float* weight, int64_t P, int32_t ph, int32_t pw, int32_t filter_size,
                   double filter_sigma, double max_val, double k1, double k2, void* workspace, double* value, float* g_rgb, void* stream);
/* coordinates.py:27-39 and :226-266 (up_sampling_VM): bilinear, align_corners=True, zero-padded resample of a table at
 * per-axis normalised positions xs [W2], ys [H2] (device) -> dst [H2][W2][C]. */
int ego_resample_table(const float* src, int32_t C, int32_t H, int32_t W, const float* xs, const float* ys, int32_t H2, int32_t W2,
                       float* dst, void* stream);
/* torch.optim.Adam step (train.py:182,311-313; no weight decay / amsgrad) over `count` tensors (host array of device
 * pointers), each with its own lr (train.py:328-329 decays lr per group); `step` counts from 1. */
typedef struct ego_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  float lr;
  int32_t reserved;
} ego_adam_tensor;
int ego_adam_step(const ego_adam_tensor* tensors, int32_t count, float beta1, float beta2, float eps, int32_t step, void* stream);
/* The same update with the step count and the learning-rate schedule ON THE DEVICE, so that a hipGraph capture of the whole
 * training step (forward + backward + this + ego_avgpool_field) can be replayed: clock = device double[4] {t, lr scale, scratch,
 * scratch}, initialised by the caller to {0, 1, 0, 0}.  Every call does t += 1, uses lr_i * scale / (1 - beta1^t) and
 * sqrt(1 - beta2^t), then scale *= lr_factor (train.py:328-329 multiplies every group's lr by lr_factor after each step). */
int ego_adam_step_graph(const ego_adam_tensor* tensors, int32_t count, float beta1, float beta2, float eps, double lr_factor,
                        double* clock, void* stream);

/* utils.py:104-152 rgb_ssim (renderer.py:160) on device images [H][W][3]: 'valid' separable Gaussian window in float64 over
 * float32 inputs.  sum (device double, may be NULL) accumulates the sum of the SSIM map — the caller divides by
 * (H-fs+1)(W-fs+1)3; ssim_map [(H-fs+1)][(W-fs+1)][3] may be NULL. */
int ego_rgb_ssim(const float* img0, const float* img1, int32_t H, int32_t W, double max_val, int32_t filter_size, double filter_sigma,
                 double k1, double k2, double* sum, float* ssim_map, void* stream);

/* v17: up to EGO_COPY_OUT_MAX float arrays device -> MAPPED host memory (hipHostMalloc / torch pinned memory: the device writes it through the
 * same pointer) in ONE launch of `workgroups` x 256 threads.  For renderer.py:39-53's `.cpu().numpy()` of every chunk's outputs: the runtime's
 * own device -> host copy is a kernel that fills the chip - next to it the following chunk's march took 260 us instead of 97, its shade 570
 * instead of 450 (tools/handover_timeline.sh) - while 8 MB over the host link need no more than a few dozen workgroups.  Ordered on `stream`
 * like any kernel; the host may read `dst` once the stream (or an event behind the call) has completed. */
#define EGO_COPY_OUT_MAX 8
int ego_copy_out(int32_t count, const float* const* src, float* const* dst, const int64_t* n_floats, int32_t workgroups, void* stream);

/* ---- backward of the separately callable stages (csrc/ego_stage_grad.hip): autograd of the reference's public stage methods, for losses
 * built from them (the sparsity term of train.py:266-272, a render loop composed of stages).  Coordinates receive no gradient (the reference
 * detaches them before grid_sample).  The forward entry points above are unchanged; these recompute what they need from the inputs.
 * Gradient tables are channel-last like the parameters and WRITTEN (no zero fill needed).  `workspace`: dev, 256-byte aligned, of the
 * size the matching *_workspace_bytes query returns (-1 = bad arguments). ---- */
/* autograd of F.grid_sample + relu + sum in compute_densityfeature (EgoNeRF.py:291-347), g = dL/d out [M].  coarse != 0:
 * compute_coarse_densityfeature (EgoNeRF.py:232-289) through the pooled tables into the FULL-resolution density gradients, i.e. the
 * AvgPool2d / AvgPool1d backward of EgoNeRF.py:124-133 (1/4 per plane texel, 1/2 per line texel; an odd last row / column gets nothing);
 * the relu masks come from sc->density_coarse, the snapshot the forward read.  16 components, coarse == 0: the sorted walk
 * (ego_scatter_sort + ego_scatter_density_sorted, bit-reproducible); otherwise ego_scatter_generic's float atomics. */
int64_t ego_density_feature_backward_workspace_bytes(const ego_scene* sc, int64_t M, int32_t coarse);
int ego_density_feature_backward(const ego_scene* sc, const float* c7n, int64_t M, int32_t coarse, const float* g, const ego_vm_grad* gdensity,
                                 void* workspace, int64_t workspace_bytes, void* stream);
/* autograd of compute_appfeature (EgoNeRF.py:349-413), g = dL/d out [M][app_dim]: the appearance table gradients (48 components: sorted
 * walk, bit-reproducible; otherwise float atomics) and gbasis [64][ldg >= 160]: row 32 grid + feature, column plane x n_comp + channel =
 * d(basis_mat_{yin,yang}.weight) (ego_weight_grad_det, fixed summation order). */
int64_t ego_app_feature_backward_workspace_bytes(const ego_scene* sc, int64_t M);
int ego_app_feature_backward(const ego_scene* sc, const float* c7n, int64_t M, const float* g, const ego_vm_grad* gapp, float* gbasis, int32_t ldg,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* autograd of MLPRender_Fea.forward (tensorBase.py:54-78) / MLPRender.forward (:107-129, fea_pe = 0) from the fp32 reference-layout weights
 * sc->mlp_w / mlp_b (not the packed blob), g_rgb = dL/d rgb [M][3].  d_feat [M][app_dim], d_viewdirs [M][3] (either may be NULL) through
 * both positional encodings; g1 [featureC][ld1 >= 160 ceil((mlp_in + 1) / 160)] = [d W1 | d b1], g2 [featureC][ld2 >= 160] = [d W2 | d b2],
 * g3 [32][ld3 >= 160] = [d W3 | d b3] in rows 0..2 (bias in column mlp_in / featureC; ego_weight_grad_det, fixed summation order). */
int64_t ego_mlp_fea_backward_workspace_bytes(const ego_scene* sc, int64_t M);
int ego_mlp_fea_backward(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, const float* g_rgb, float* d_feat, float* d_viewdirs,
                         float* g1, int32_t ld1, float* g2, int32_t ld2, float* g3, int32_t ld3, void* workspace, int64_t workspace_bytes,
                         void* stream);
/* autograd of SHRender (tensorBase.py:30-34, sh.py:87-112): d_viewdirs [M][3], d_features [M][27] (either may be NULL) */
int ego_sh_render_backward(const float* viewdirs, const float* features, int64_t M, const float* g_rgb, float* d_viewdirs, float* d_features,
                           void* stream);
/* autograd of feature2density (tensorBase.py:415-419): softplus(f + density_shift) with torch's threshold 20, or relu */
int ego_feature2density_backward(const ego_scene* sc, const float* feat, int64_t M, const float* g, float* d_feat, void* stream);
/* autograd of raw2alpha (tensorBase.py:22-27) over [N][S]: gradients g_alpha, g_weight [N][S], g_bg [N] (any may be NULL) -> d_sigma,
 * d_dist [N][S].  The cumprod backward as a per-ray reverse scan without division by 1 - alpha + 1e-10 (exact where it underflows). */
int ego_raw2alpha_backward(const float* sigma, const float* dist, const float* alpha, int64_t N, int32_t S, const float* g_alpha, const float* g_weight,
                           const float* g_bg, float* d_sigma, float* d_dist, void* stream);

/* ---- ray gradients (csrc/ego_ray_grad.hip; append-only additions, EGO_ABI_VERSION stays 17).  No reference counterpart:
 * EgoNeRF.forward detaches the coordinates before grid_sample, so there the positional part of d loss / d rays is zero by construction. ---- */
/* d loss / d viewdir of every sample through the head's first layer (tensorBase.py:68-75): with dx = W1^T dh1 restricted to the view columns,
 * d_view[m][j] = dx[app_dim + j] + sum_f 2^f (cos(2^f d_j) dx[sin column] - sin(2^f d_j) dx[cos column]), d = rays[m / S][3..5], W1 =
 * sc->mlp_w[0] (fp32, the reference's layout; the packed blob is not read).  dh1 [M][mlp_hidden] is the head backward's gradient at the first
 * hidden layer, relu mask applied: dh_layout 0 = row-major fp32 (ego_shade_backward_generic's; 16-byte aligned, dh_scale unused), 2 =
 * ego_shade_backward's scaled fp16 (dh_scale = row 1 of its dh_scale, [M]).  d_view [M][3] is written.  M = N S; M == 0 is a no-op; an RGB
 * head (no network: the gradient is zero, pass d_view = NULL to ego_ray_grad instead) and other bad arguments return EGO_E_BADARG before
 * anything is queued.  One launch, no atomics, no host synchronisation. */
int ego_view_grad(const ego_scene* sc, const float* rays, int32_t S, int64_t M, const void* dh1, int32_t dh_layout, const float* dh_scale,
                  float* d_view, void* stream);
/* g_rays [N][6] = d loss / d (origin, direction) of the training render, WRITTEN (not accumulated).  The sample distances z [N][S] are
 * constants, the chart of a sample is the forward's (coords [N][S][4], ego_march_density's coords_out; 16-byte aligned).  Per ray,
 *   g_o = sum_s J_s^T q_s,   g_d = sum_s z_s J_s^T q_s + sum_s d_view[s] + e_n:
 * q_s = d loss / d (r^, theta^, phi^) through both lookups - F.grid_sample's backward with respect to the grid (align_corners, zero padding:
 *   per axis the weights' derivatives are -/+ (n - 1) / 2 on the taps that are in range) - with dfeat [M] (ego_march_backward's; the per-plane
 *   relu mask of EgoNeRF.py:340,346 is applied here) and g_v = basis_g^T dfe re-derived per channel from dfe: [M][32] (ldfe 32,
 *   ego_shade_backward's) or [M][64] (ldfe 64, ego_shade_backward_generic's dfe64; the half of the sample's own grid is read).  Either may
 *   be NULL (that field contributes nothing).  The taps are re-gathered from the fp32 tables of sc->density / sc->app (n_comp a multiple of 4
 *   up to 48, app_dim <= 32); app16 is not read.
 * J_s = d (r^, theta^, phi^) / d xyz at xyz = o + z_s d for the chart coords.w names, the radius cell found as ego_normalize_coord finds it
 *   (fine_pass != 0: on sc->r_lut_fine where the scene has one).  A sample with r = 0, with q_s = 0 (NaN or out-of-range coordinates mask
 *   every tap) or a non-finite product contributes exactly 0.
 * d_view [M][3] (ego_view_grad's) or NULL.  e_n: the envmap's direction term, d (bg_weight sigmoid(bilinear(emission, dir))) / d dir
 *   through F.normalize, with ego_envmap_backward's clamp mask from rgb_raw; g_rgb, rgb_raw [N][3], bg_weight [N], env_map [N][3] - all
 *   four or none (NULL without an envmap).
 * d_xyz [M][3] optional (NULL in training): receives J_s^T q_s per sample.
 * A ray's samples are summed in a fixed order inside one wave: no atomics, two calls return the same bits.  Any N >= 0 (0: no-op), any
 * S >= 1, N S < 2^31; one launch, no host synchronisation. */
int ego_ray_grad(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* dfeat, const float* dfe, int32_t ldfe,
                 const float* d_view, const float* g_rgb, const float* rgb_raw, const float* bg_weight, const float* env_map, int64_t N, int32_t S,
                 int32_t fine_pass, float* d_xyz, float* g_rays, void* stream);

/* ---- ray geometry (csrc/ego_geometry.hip; append-only addition, EGO_ABI_VERSION stays 17).  No reference counterpart: the
 * reference's only geometric output is the expected depth sum_s w_s z_s. ---- */
/* Surface normal, accumulated weight and quantile depth of N rays from the samples of a march: z, weight [N][S] and coords [N][S][4]
 * (ego_march_density's z_out / weight / coords_out; coords 16-byte aligned, .w the chart the forward chose).
 *   f = the density feature of the full-resolution tables of sc->density, sum_i relu(sum_c P_c L_c) (EgoNeRF.compute_densityfeature; n_comp a
 *       multiple of 4 up to 48, any resolutions >= 2); g_s = grad_xyz f at o + d z_s in the chart coords.w names, the radius cell found on
 *       sc->r_lut as ego_normalize_coord finds it: what ego_ray_grad computes for dfeat = 1, dfe = NULL.
 *   n_s = -g_s / |g_s|, 0 where |g_s| is 0 or not finite (every plane dead, outside the grid, r = 0).
 *   normal [N][3] = sum_s w_s n_s; with normalize != 0 divided by its length (0 stays 0), without it its length is <= acc and says how well
 *       the ray's normals agree.
 *   acc [N] = sum_s w_s.
 *   z_quantile [N] = z of the first sample at which the running sum of w reaches `quantile` (in (0, 1); 0.5: the median depth); 0.0f for a
 *       ray that never reaches it.
 *   grad_out [N][S][3] = g_s.
 * Each output may be NULL, at least one must not be.  A sample with w_s == 0 exactly adds exactly nothing to normal and is not gathered
 * unless grad_out asks for it; normal has the same bits either way.  All sums run in one fixed order in float32 inside one wave: no atomics,
 * two calls return the same bits.  Any N >= 0 (0: no-op), any S >= 1, N S < 2^31; bad arguments return EGO_E_BADARG before anything is
 * queued.  One launch, no host synchronisation. */
int ego_ray_geometry(const ego_scene* sc, const float* rays, const float* z, const float* coords, const float* weight, int64_t N, int32_t S,
                     int32_t normalize, float quantile, float* normal, float* acc, float* z_quantile, float* grad_out, void* stream);

/* ---- triangle meshes (csrc/ego_mesh.hip; append-only addition, EGO_ABI_VERSION stays 17).  The reference meshes with
 * skimage's marching cubes on a Cartesian alpha volume (--export_mesh); this is the field on a lattice and an extractor on the device. ---- */
#define EGO_LATTICE_BOX 0
#define EGO_LATTICE_PANORAMA 1
/* A lattice of n[0] x n[1] x n[2] nodes, axis 0 fastest: node id = (i2 n[1] + i1) n[0] + i0, below 2^31; every n >= 2.
 *   box:      axes (x, y, z); position = fadd(origin, fmul((float)i, step)) per axis, every operation rounded once.
 *   panorama: axes (radius index, row, col), n = (number of radii, H, W), W >= 3; position = fadd(o, fmul(radii[i0], d)) with (o, d) the
 *             ego_erp_rays ray of pixel (row, col) of an H x W panorama with pose c2w, normalize = 1: the pixel centres, no node on a pole.
 *             radii: dev [n[0]], strictly increasing, > 0.  Axis 2 wraps: the cells of column W - 1 have column 0 as their far side (W
 *             cells along the axis); the two polar caps, half a pixel wide, stay open.
 * flip: 1 when (axis 0, axis 1, axis 2) is a left-handed frame (panorama: rows run down, columns clockwise seen from above), else 0. */
typedef struct ego_lattice {
  int32_t kind; /* EGO_LATTICE_* */
  int32_t n[3];
  float origin[3], step[3]; /* box */
  const float* radii;       /* panorama */
  int32_t H, W;
  float c2w[12]; /* 3x4 row-major */
  int32_t flip;
  int32_t reserved;
} ego_lattice;

/* values[node] = sigma at the node: ego_from_cartesian -> ego_normalize_coord -> ego_density_feature(coarse = 0) -> ego_feature2density in one
 * kernel, lane = node, on the full-resolution factored tables of sc->density (every n_comp ego_density_feature takes).  values: dev [count]. */
int ego_mesh_field(const ego_scene* sc, const ego_lattice* lat, float* values, void* stream);

/* The iso-surface value = level of any float32 array values [count] on the lattice: marching tetrahedra on the Kuhn decomposition.
 *   A cell's corners are the bit triples b (bit a = one step along axis a) over its low node; its six tetrahedra, for the axis
 *   permutations p = (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0) in this order, have the corners 000, e_p0, e_p0 + e_p1, 111.
 *   Every tetrahedron edge runs from a corner a to a corner b that contains it and is OWNED by the node at a, local index
 *   k = bits(b - a) - 1 in 0..6 (three axis edges, three face diagonals, the body diagonal); far nodes on a wrapping axis modulo W.
 *   A node is inside when value >= level (NaN: outside); an owned edge carries a vertex when exactly one end is inside, at
 *   pa + t (pb - pa), t = (level - fa) / (fb - fa) clamped to [0, 1], 0.5 when not finite, a = the owner, float32 operations rounded once.
 *   Vertex ids increase with (node id, k); faces are ordered by (cell id = id of its low node, tetrahedron, triangle), a tetrahedron
 *   giving 0, 1 or 2; (v1 - v0) x (v2 - v0) points to the outside (lower values).  tests/mesh_ref.py restates all of it in numpy.
 * ego_mesh_count classifies the nodes, marks every node's crossing owned edges, counts the triangles per cell, scans both counts
 *   (per-workgroup sums, one scan of the sums; the offsets are applied by ego_mesh_emit) and writes counts_dev[0] = V, counts_dev[1] = F
 *   (dev int64 [2]).  workspace: dev, 256-byte aligned, ego_mesh_workspace_bytes(lat) bytes (-1: bad lattice), about 6 bytes per node.
 * ego_mesh_emit, after the caller has read V and F back (the one host synchronisation of an extraction), writes vertices [V][3] float32 and
 *   faces [F][3] int32 from the same values, level and workspace; V and F below 2^31; V = F = 0 queues nothing.
 * No atomics: two calls return the same bits.  Bad arguments return EGO_E_BADARG before anything is queued. */
int64_t ego_mesh_workspace_bytes(const ego_lattice* lat);
int ego_mesh_count(const ego_lattice* lat, const float* values, float level, void* workspace, int64_t bytes, int64_t* counts_dev, void* stream);
int ego_mesh_emit(const ego_lattice* lat, const float* values, float level, const void* workspace, int64_t V, int64_t F, float* vertices,
                  int32_t* faces, void* stream);

/* out [M][3] = grad_xyz f of the density feature (ego_ray_geometry's f and g_s) at M arbitrary points xyz [M][3], the chart chosen as
 * ego_from_cartesian chooses it; with normalize != 0, -grad f / |grad f| instead.  0 where the gradient is 0 or not finite.  One 16-lane
 * row per point, a fixed summation order: two calls return the same bits.  Any M >= 0 (0: no-op); one launch, no host synchronisation. */
int ego_point_gradient(const ego_scene* sc, const float* xyz, int64_t M, int32_t normalize, float* out, void* stream);

typedef struct ego_render_args {
  int32_t n_coarse, n_fine;
  int32_t resampling, use_coarse_sample;
  const float* r_sched; /* dev [n_coarse] */
  const float* jitter;  /* dev [N][n_coarse] or NULL (eval) */
  const float* u;       /* dev [N][n_fine] or NULL (eval: linspace) */
  float near_;
  int32_t reserved;
  const float* z_coarse; /* dev [N][n_coarse] explicit distances of the first pass, or NULL.  Overrides r_sched / jitter: the
                          * exp_sampling=False path, TensorBase.sample_ray (tensorBase.py:308-327), whose per-ray schedule the
                          * host computes */
  void* marched;         /* v17: hipEvent_t or NULL.  Recorded on `stream` behind the LAST march launch, ahead of the shade: lets a caller
                          * start copies of the PREVIOUS call's outputs under this call's shade kernel (bound by instruction issue) instead
                          * of under its march (bound by the latency of its gathers: next to the runtime's copy kernel it took 260 us
                          * instead of 97, tools/handover_timeline.sh).  A call that passes it never takes the one-launch render
                          * (ego_render_forward_marches), which has no point between march and shade */
} ego_render_args;

/* Whole EgoNeRF.forward for N rays.  S_out = n_coarse (no resampling) | n_coarse+n_fine | n_fine.
 * workspace: dev scratch of ego_render_workspace_bytes(N, args) bytes.
 * Outputs: rgb_map [N][3], depth [N], alpha [N][S_out (+1 with envmap)], bg_map/env_map [N][3] (envmap only). */
int64_t ego_render_workspace_bytes(int64_t N, const ego_render_args* args);
int ego_render_forward(const ego_scene* sc, const ego_render_args* args, const float* rays, int64_t N, void* workspace,
                       float* rgb_map, float* depth, float* alpha, float* bg_map, float* env_map, void* stream);

/* How many samples the last ego_render_forward of N rays with these args on `workspace` sent through the appearance lookup and the
 * MLP: the live count on the compact path (ego_render_forward_compacts; the size of tensorBase.py:480-487's app_mask), 32 x the
 * shaded tiles, at most N S, on the tile paths, N S without skipping.  Written to *out_dev (device int64) on `stream` by one launch,
 * no host synchronisation.  EGO_E_BADARG if no ego_render_forward of this N and sample count has run on `workspace` in this process. */
int ego_render_shaded_samples(int64_t N, const ego_render_args* args, const void* workspace, int64_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGONERF_HIP_H */
