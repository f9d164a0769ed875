/*
 * sdp.h -- C ABI of libsdp.so, the MI355X (gfx950) implementation of the
 * Simultaneous-Diffusion-for-Pointclouds sampling hot path.
 *
 * Every pointer argument named x/grad/ref/... is a DEVICE pointer owned by the caller
 * unless documented otherwise; every call is enqueued on the caller's hipStream_t
 * (passed as void*) and never synchronises the device.  Return value: 0 = OK,
 * < 0 = error; sdp_last_error() gives a thread-local message for the last failure.
 * Handles are per device and not thread-safe: one handle per (device, thread).
 *
 * Reference interfaces replaced (paths relative to /root/reference/LiDARGen):
 *   sdp_net_*              scorenet(x, y) = NCSN_LiDAR_small.forward   models/ncsnv2.py:420-518
 *                          weight load    load_state_dict + EMAHelper  runners/ncsn_runner_kitti_simultaneous.py:472-489
 *   sdp_langevin_step      Langevin update                           models/KITTISampling.py:133-156,
 *   sdp_net_forward_langevin  scorenet + Langevin update in one call   models/KITTISampling.py:137-156
 *                                                                     models/__init__.py:236-259, :1397-1416
 *   sdp_consistency_merge  cross-view reprojection + correction      models/KITTISampling.py:160-490 (pose matrices),
 *                                                                     models/__init__.py:263-579 (origin offsets)
 *   sdp_net_forward_train  scores = scorenet(perturbed, labels) in train mode   losses/dsm.py:85
 *   sdp_dsm_loss           anneal_dsm_score_estimation_with_mask            losses/dsm.py:67-119
 *   sdp_net_backward       loss.backward()                                  runners/ncsn_runner_kitti_simultaneous.py:230
 *   sdp_net_backward_buckets  loss.backward() + DataParallel's gradient reduce  (kitti runner :104,481,230)
 *   sdp_adam_ema_step      optimizer.step() (Adam, losses/__init__.py:10-20) + EMAHelper.update (models/ema.py:16-21)
 *   sdp_optim_ema_step     optimizer.step() of Adam / RMSprop / SGD (get_optimizer, losses/__init__.py:3-13) + EMA
 *   sdp_range_project      point_cloud_to_range_image                       datasets/lidar_utils.py:54-347
 *   sdp_range_unproject    range image -> fused point cloud                 MeasureResults/SceneCompleter.py:43-70,
 *                                                                             105-121, 259-264
 *   sdp_view_transform     pose chain fromWorld @ (toWorld @ p)             datasets/kitti360_im_8Batch.py:146-190
 *   sdp_view_gather        scanPoints[index[index >= 0]]                    datasets/kitti360_im_simultenous_densification.py:186-203
 *   sdp_view_finalize      __getitem__ post-processing of the range images  datasets/kitti360_im_8Batch.py:221-304
 *   sdp_grid_subsample     voxel-grid subsampling, HOST memory, both methods   datasets/cpp_wrappers/cpp_subsampling/
 *                                                                             grid_subsampling{,_lidar}.cpp, wrapper.cpp:58-285
 *   sdp_voxel_grid         voxel-grid subsampling, DEVICE memory, barycenters  .../grid_subsampling/grid_subsampling.cpp:46-102
 *   sdp_cloud_nn           exact nearest neighbour within a radius, cloud to cloud   (no counterpart: MeasureResults/ scores
 *   sdp_cloud_nn_stats     Chamfer / precision / recall sums of one direction         images only, per-pixel MAE)
 *   sdp_voxel_iou          voxel occupancy / semantic confusion matrix of two clouds  MeasureResults/SceneCompleter.py:256-270
 *                                                                             (the cloud it hands to a metrics.iou it does not ship)
 */
#ifndef SDP_H
#define SDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDP_VERSION 100  /* 1.0.0 */

/* arithmetic used for the score network's convolutions (fp32 I/O and accumulation in all modes) */
enum sdp_precision {
  SDP_PREC_FP32 = 0,    /* v_mfma_f32_32x32x2_f32: exact fp32 products                         */
  SDP_PREC_FP32X3 = 1,  /* 3-pass bf16 split (hi*hi + hi*lo + lo*hi) on v_mfma_f32_16x16x32_bf16  */
                        /* (forward and data gradient; weight gradient on v_mfma_f32_32x32x16)   */
  SDP_PREC_BF16 = 2     /* single bf16 pass (fast, NOT within the fp32 parity tolerance)        */
};

typedef struct sdp_net_desc {
  int ngf;          /* 128 (NCSN_LiDAR_small config.model.ngf)                    */
  int channels;     /* 2 (depth, intensity)                                        */
  int H, W;         /* 64, 1024 (config.data.image_size / image_width)             */
  int num_classes;  /* 232 (length of the model's sigma buffer)                    */
  int precision;    /* enum sdp_precision                                          */
} sdp_net_desc;

typedef struct sdp_net sdp_net;

int sdp_version(void);
const char* sdp_last_error(void);

/* ---- score network (NCSN_LiDAR_small) ------------------------------------------------ */
int sdp_net_create(const sdp_net_desc* desc, sdp_net** out);
/* Copy one state_dict tensor (HOST float32, reference key and shape, e.g. "res1.0.conv1.weight"
 * [128,128,3,3] or "sigmas" [232]).  The library owns its copy after the call. */
int sdp_net_set_param(sdp_net* net, const char* key, const float* host_data, const int64_t* shape, int ndim);
/* Check every parameter was set and upload the device layouts (blocking; call once). */
int sdp_net_finalize(sdp_net* net);
int sdp_net_workspace_size(const sdp_net* net, int B, size_t* bytes);
/* out[B,2,H,W] = scorenet(x[B,2,H,W], labels[B]) ; labels: int64 device array indexing sigmas. */
int sdp_net_forward(sdp_net* net, const float* x, const int64_t* labels, float* out, int B,
                    void* workspace, size_t workspace_bytes, void* stream);
int sdp_net_destroy(sdp_net* net);
/* One annealed-Langevin step with the update fused into the score net's last kernel
 * (KITTISampling.py:137-156 in one call): grad = scorenet(x, labels) is computed and, in the same
 * epilogue, x <- x + step*g' + grad_ref*lik + noise*noise_scale exactly as sdp_langevin_step
 * (same float32 order, same Philox counters: bit-identical to sdp_net_forward followed by
 * sdp_langevin_step).  x [B,2,H,W] is read by the first layer and updated in place by the last.
 * grad_out (nullable) receives the scores; lik_out / absmax_bits as in sdp_langevin_step.     */
typedef struct {
  const float* ref;            /* [B,2,H,W] */
  const int32_t* mask;         /* [B,2,H,W] */
  const float* noise;          /* nullable: Philox4x32-10(seed, offset + i/4) */
  uint64_t seed, offset;
  float step_size, noise_scale, grad_ref;
  int nan_to_num;
  float* lik_out;              /* nullable */
  uint32_t* absmax_bits;       /* nullable */
  float* grad_out;             /* nullable */
} sdp_langevin_params;
int sdp_net_forward_langevin(sdp_net* net, float* x, const int64_t* labels, int B, const sdp_langevin_params* params,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Performance knob: run sdp_net_forward / sdp_net_forward_langevin as `ways` part-batch forwards on
 * that many streams (the caller's + the handle's own, joined before return; 1 = one launch per
 * layer, 0 = the default, 2).  Results are identical for every value; the
 * workspace size depends on it (query sdp_net_workspace_size after setting it).              */
int sdp_net_set_split(sdp_net* net, int ways);
/* Measurement hooks: when enabled, every conv launch of sdp_net_forward is bracketed by HIP
 * events on the forward's stream; sdp_net_profile_read synchronises on them and writes one
 * line per conv class: "class\tlaunches\ttotal_ms\tflops_per_launch\n". */
int sdp_net_profile_enable(sdp_net* net, int enable);
int sdp_net_profile_read(sdp_net* net, char* buf, size_t cap, int* n_launches);

/* ---- parameters as one device arena (training) ------------------------------------------
 * Every learnable parameter (state_dict keys minus the "sigmas" buffer), float32, each at a
 * 64-float aligned offset, in the order sdp_net_backward finishes their gradients (head first,
 * begin_conv last; sdp_net_param_info enumerates it).  sdp_net_bind_params copies the current values into a
 * caller-owned device arena of sdp_net_param_arena_floats floats and makes it the net's
 * parameter storage; after the caller changes it (optimizer), sdp_net_repack rebuilds the
 * packed conv weights on `stream`.  Gradient arenas use the same layout.                    */
int sdp_net_param_arena_floats(const sdp_net* net, size_t* n);
int sdp_net_param_count(const sdp_net* net, int* n);
int sdp_net_param_info(const sdp_net* net, int i, char* key, size_t cap, size_t* offset, size_t* numel);
int sdp_net_bind_params(sdp_net* net, float* arena, void* stream);
int sdp_net_repack(sdp_net* net, void* stream);

/* ---- DSM training (BASELINE config 5; precision fp32x3 or bf16) -------------------------
 * sdp_net_forward_train: out = scorenet(x, labels), keeping every tensor the backward needs
 * (the tape) in `workspace` (sdp_net_train_workspace_size bytes).  sdp_net_backward then writes
 * d loss/d parameters for d loss/d out = dscore into `grads` (a parameter-layout arena,
 * overwritten) -- same workspace and B, no other train-mode call on this net in between.   */
int sdp_net_train_workspace_size(sdp_net* net, int B, size_t* bytes);
/* bf16 precision only: 1 (the default) keeps the tape -- every activation and output gradient of
 * sdp_net_forward_train / sdp_net_backward -- in bf16 (half the bytes of every conv's operand and
 * epilogue streams, of the weight gradient's and of the adjoints'); 0 keeps it in float32.  The
 * parameters, the gradient arena, the statistics and the scores are float32 either way.  Takes effect
 * at the next sdp_net_train_workspace_size / sdp_net_forward_train (the workspace size depends on it). */
int sdp_net_set_tape(sdp_net* net, int bf16);
int sdp_net_forward_train(sdp_net* net, const float* x, const int64_t* labels, float* out, int B,
                          void* workspace, size_t workspace_bytes, void* stream);
int sdp_net_backward(sdp_net* net, const float* dscore, int B, void* workspace, size_t workspace_bytes,
                     float* grads, void* stream);
/* sdp_net_backward with gradient buckets for a data-parallel reduce overlapped with the backward
 * (replaces the implicit gradient reduce of torch.nn.DataParallel,
 * runners/ncsn_runner_kitti_simultaneous.py:104,481): bucket i is the arena range
 * [bucket_end[i-1], bucket_end[i]) (floats, increasing, <= sdp_net_param_arena_floats); events[i]
 * (hipEvent_t) is recorded on `stream` as soon as the launches that finish every gradient of that
 * range are enqueued, so a communication stream can wait on it while the backward goes on. */
int sdp_net_backward_buckets(sdp_net* net, const float* dscore, int B, void* workspace, size_t workspace_bytes,
                             float* grads, int n_buckets, const size_t* bucket_end, void* const* events,
                             void* stream);
/* loss = mean_b 1/2 * sum_i (mask*(score - target))^2 * n_img / sum(mask) * sigma_b^p with
 * target = -noise / sigma_b^2 (noise already scaled by sigma_b, as the reference passes it);
 * writes dscore = d loss / d score, loss[0], loss_per[b] (optional).  mask float32 0/1,
 * n_img = C*H*W, part: 2*B*64 floats of scratch.                                             */
int sdp_dsm_loss(const float* score, const float* noise, const float* mask, const float* used_sigma, int B,
                 int n_img, float anneal_power, float* dscore, float* loss, float* loss_per, float* part,
                 void* stream);
/* torch.optim.Adam step (weight_decay 0, amsgrad off) over n floats, step = 1, 2, ...; then
 * ema_shadow = (1 - ema_mu)*p + ema_mu*ema_shadow if ema_shadow is not NULL.                 */
int sdp_adam_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema_shadow,
                      size_t n, double lr, double beta1, double beta2, double eps, int step, double ema_mu,
                      void* stream);
/* optimizer.step() of every optimizer get_optimizer builds (losses/__init__.py:3-13), in torch's
 * per-element order, then the EMA update as above.  g <- g + weight_decay*p first (all kinds).
 *   SDP_OPTIM_ADAM    state0 exp_avg, state1 exp_avg_sq, state2 max_exp_avg_sq (amsgrad) or NULL;
 *                     betas (beta1, beta2)
 *   SDP_OPTIM_RMSPROP state0 square_avg; beta2 = alpha (torch default 0.99), eps (default 1e-8)
 *   SDP_OPTIM_SGD     state0 momentum_buffer (written as g on step 1); beta1 = momentum, dampening 0
 * step = 1, 2, ... (the optimizer's step count after this step).                            */
enum sdp_optim_kind { SDP_OPTIM_ADAM = 0, SDP_OPTIM_RMSPROP = 1, SDP_OPTIM_SGD = 2 };
int sdp_optim_ema_step(int kind, float* params, const float* grads, float* state0, float* state1, float* state2,
                       float* ema_shadow, size_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, double ema_mu, void* stream);
/* (hyperparameters are host doubles -- the Python floats torch.optim and EMAHelper compute with:
 *  1 - beta, 1 - mu and the bias corrections are formed in double and rounded once)          */

/* ---- Langevin update ------------------------------------------------------------------ *
 * x <- x + step*g' + grad_ref*lik + noise*noise_scale   (float32, reference evaluation order)
 *   g'  = nan_to_num(grad) if nan_to_num else grad;  lik = -mask*(x - ref)
 *   noise = noise_or_null[i] if given, else N(0,1) from Philox4x32-10(seed, counter = offset + i/4)
 * Optional outputs: lik_out (the step's grad_likelihood, used by the denoise step) and
 * absmax_bits: atomicMax of |x_new[:,0]| float bits (the merge's tooHigh input).          */
int sdp_langevin_step(float* x, const float* grad, const float* ref, const int32_t* mask,
                      const float* noise_or_null, uint64_t seed, uint64_t offset,
                      float step_size, float noise_scale, float grad_ref, int nan_to_num,
                      int B, int C, int HW, float* lik_out, uint32_t* absmax_bits, void* stream);
/* x <- x + a*g + b*lik   (denoise: a = sigma_L^2, b = grad_ref) ; x <- x + b*(-mask*(x-ref)) if g == NULL */
int sdp_axpy_step(float* x, const float* g, float a, const float* lik, const int32_t* mask,
                  const float* ref, float b, int n, void* stream);

/* ---- cross-view consistency merge ----------------------------------------------------- */
enum sdp_merge_variant { SDP_MERGE_POSES = 0, SDP_MERGE_ORIGINS = 1 };

typedef struct sdp_merge_params {
  int variant;            /* enum sdp_merge_variant                                        */
  int setting;            /* 5 (kitti min-depth filter) / 7 (AllForOne controlled average) */
  float sigma;            /* current sigma (float32 from the sigma array)                  */
  float allowance;        /* metres (10)                                                   */
  float cc;               /* correlation coefficient                                       */
} sdp_merge_params;

int sdp_merge_workspace_size(int n_src, int n_out, int H, int W, size_t* bytes);   /* any aB <= n_src */
/* the same for megabatches of exactly aB views (the pair records scale with n_out * aB * H * W) */
int sdp_merge_workspace_bytes(int n_src, int aB, int n_out, int H, int W, size_t* bytes);
/*
 * x_all   : [n_src,2,H,W] current images of every source view (device, float32)
 * toWorld : [n_src,4,4] float64 (POSES) ; fromWorld : [n_src,4,4] float64 (POSES)
 * origins : [aB,3] float32 view origins (ORIGINS variant; models/__init__.py:224-231)
 * exist   : [aB,H,W] uint8 (existMask[:aB]) ; sky : [n_src,H,W] uint8 ; refmask : [n_src,2,H,W] int32
 * Views are grouped into megabatches of aB consecutive indices.  Output views are
 * [o_begin, o_begin+n_out); their images in x_all are corrected in place.
 * absmax_bits : device word holding max|x[:,0]| bits over ALL views of the step (tooHigh).
 * new_images  : optional [n_out,2,H,W] float32 output (the reference's newImages).
 */
int sdp_consistency_merge(float* x_all, int n_src, int aB, int o_begin, int n_out, int H, int W,
                          const double* toWorld, const double* fromWorld, const float* origins,
                          const uint8_t* exist, const uint8_t* sky, const int32_t* refmask,
                          const sdp_merge_params* params, const uint32_t* absmax_bits,
                          float* new_images, void* workspace, size_t workspace_bytes, void* stream);
/* The same merge for multi-rank runs: the stream waits for absmax_event (a hipEvent_t
 * recorded after the cross-rank all_reduce(MAX) of absmax_bits, or NULL) only right before the final
 * correction pass, the merge's one reader of that word -- so the all_reduce on another stream runs
 * beside the projection, binning and resolve passes instead of before them. */
int sdp_consistency_merge_ev(float* x_all, int n_src, int aB, int o_begin, int n_out, int H, int W,
                             const double* toWorld, const double* fromWorld, const float* origins,
                             const uint8_t* exist, const uint8_t* sky, const int32_t* refmask,
                             const sdp_merge_params* params, const uint32_t* absmax_bits,
                             float* new_images, void* workspace, size_t workspace_bytes, void* stream,
                             void* absmax_event);

/* ---- point cloud -> range image (data front end; datasets/lidar_utils.py:54-347) --------
 * points: DEVICE float64 [N][stride] (x, y, z[, intensity]); origin: HOST float64 [3].
 * Outputs (DEVICE, [H][W], already flipped in both axes like the reference): depth float64
 * (maxRange 2057.701 where empty), intensity float64 (optional, needs has_intensity),
 * obfuscation u8, sky u8 (all 0, as the reference clears it; both NULL skips the row-sequential
 * sky/obfuscation scan), index int64 (optional, -1 empty).
 * The nearest point per pixel wins; equal depths keep the lowest point index.               */
int sdp_range_project_workspace_size(int H, int W, size_t* bytes);
int sdp_range_project(const double* points, int N, int stride, int has_intensity, const double* origin,
                      int H, int W, double* depth, double* intensity, uint8_t* obfuscation, uint8_t* sky,
                      int64_t* index, void* workspace, size_t workspace_bytes, void* stream);

/* ---- range image -> point cloud (MeasureResults/SceneCompleter.py:43-70, 105-121, 259-264) ----
 * The inverse of sdp_range_project for the samplers' images: x DEVICE float32 [B][C][H][W]
 * (channel 0 the log-depth code, channel 1 the intensity; C = 1 or 2) becomes a compacted cloud of
 * float64 rows (x, y, z, intensity) -- views in order, pixels row-major inside a view: numpy's
 * cloud[mask] per view, concatenated (SceneCompleter.py:261-264).  Pixel (i, j) lies at distance
 * rd = f32(2^f32(|code|*6)) - 1 (float32, 2^v rounded once from float64: the merge's convention,
 * KITTISampling.py:164-166 -- SceneCompleter's float32 np.power is not correctly rounded) in the
 * direction (cos az cos el, sin az cos el, sin el), el = (H-1-i)*vA + vMin, az = (W-1-j)*hA + hMin,
 * float64, with the constants of
 *   SDP_GEOM_DATASET  datasets/lidar_utils.py:100-114 and SceneCompleter.py:57-70 (sdp_range_project;
 *                     vMin = radians(3 - 28)) -- the images the datasets render and the runners save;
 *   SDP_GEOM_SAMPLER  models/KITTISampling.py:29-102 (sdp_consistency_merge; vMin =
 *                     ((H*-25)//28)*vA + vA/2, 0.36 bin above the dataset's).
 * Placement: origins DEVICE f64 [B][3] added to each point, OR poses DEVICE f64 [B][4][4] row-major
 * applied as (pose @ [x y z 1])[:3] (products summed left to right, as sdp_view_transform), or both
 * NULL = the sensor frame.  A pixel is kept iff rd > min_range (float32 compare; a NaN code fails
 * it) and keep_view[b][i][j] and keep_shared[i][j] (uint8, each optional) are non-zero
 * (SceneCompleter.py:259-260: existVals, realDistance > 1.5, not sky).
 * Outputs (DEVICE): points [n][4] (capacity B*H*W rows; rows >= n are not written), pixel (optional
 * int32 [n], the flat index b*H*W + i*W + j of each row), offsets int64 [B+1] (view b owns rows
 * [offsets[b], offsets[b+1]); offsets[B] = n).  Three launches (count, scan, scatter) and no
 * atomics: the rows are bit-identical from run to run.  B * (H*W rounded up to a multiple of
 * 256) must stay below 2^31.                                                                  */
enum sdp_unproject_geometry { SDP_GEOM_DATASET = 0, SDP_GEOM_SAMPLER = 1 };
int sdp_range_unproject_workspace_size(int B, int H, int W, size_t* bytes);
int sdp_range_unproject(const float* x, int B, int C, int H, int W, int geometry,
                        const double* origins, const double* poses,
                        const uint8_t* keep_view   /* [B][H][W] or NULL */,
                        const uint8_t* keep_shared /* [H][W]    or NULL */,
                        float min_range,
                        double* points /* capacity B*H*W rows of 4 */, int32_t* pixel /* or NULL */,
                        int64_t* offsets /* [B+1] */,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- KITTI-360 view rendering (the datasets' __getitem__) --------------
 * sdp_view_transform: points DEVICE float32 [n][4] (x, y, z, intensity, the .bin layout);
 *   m1, m2 HOST float64 row-major 4x4 or NULL.  out DEVICE float64 [n][4] =
 *   (m2 @ (m1 @ [x y z 1]))[:3], intensity -- kitti360_im_8Batch.py:146-190 with m1 = toWorld
 *   of the scan's pose and m2 = fromWorld of the goal pose; NULL, NULL = float64 widening.
 * sdp_view_gather: the densification subsample scanPoints[index[index >= 0]] after
 *   index[:, :blank_cols] = -2 (kitti360_im_simultenous_densification.py:186-203).  index DEVICE
 *   int64 [H][W] (sdp_range_project output), points DEVICE float32 [N][4]; out DEVICE float64
 *   [<= H*W][4] in row-major pixel order; *count (DEVICE int) = number written.
 * sdp_view_finalize: kitti360_im_8Batch.py:221-304 (variant SDP_VIEW_8BATCH),
 *   kitti360_im_AllForOne.py:253-353 (SDP_VIEW_ALLFORONE), kitti360_im_simultenous_
 *   densification.py:230-339 (SDP_VIEW_DENSIFICATION; first_view = numberInBatch == 0).
 *   Inputs are sdp_range_project outputs of the view and of the goal scan ([H][W], DEVICE;
 *   intensity / goal_intensity only with channels == 2); roll = the random_roll column shift
 *   or -1.  Outputs DEVICE: real, goal float64 [channels][H][W], notmask u8 [channels][H][W]
 *   (np.logical_not(mask)), notsky u8 [H][W] (np.logical_not(sky) after the 3-row shift).
 *   SDP_VIEW_COMPLETION: kitti360_im_SceneCompletion.py:388-513 -- channel 2 of real is the
 *   depth code again and its mask is all ones (the reference concatenates (real, real) and
 *   (mask, ones)); goal_depth / goal_intensity / goal may be NULL (no goal scan).            */
enum sdp_view_variant { SDP_VIEW_8BATCH = 0, SDP_VIEW_ALLFORONE = 1, SDP_VIEW_DENSIFICATION = 2, SDP_VIEW_COMPLETION = 3 };
int sdp_view_transform(const float* points, int64_t n, const double* m1, const double* m2, double* out, void* stream);
int sdp_view_gather(const int64_t* index, int H, int W, int blank_cols, const float* points, double* out, int* count,
                    void* stream);
int sdp_view_finalize(const double* depth, const double* intensity, const uint8_t* obfuscation, const uint8_t* sky,
                      const double* goal_depth, const double* goal_intensity, int H, int W, int channels, int roll,
                      int variant, int first_view, double* real, uint8_t* notmask, uint8_t* notsky, double* goal,
                      void* stream);

/* ---- §8(f)-3: voxel-grid subsampling: sdp_grid_subsample on HOST memory (no stream), sdp_voxel_grid
 * on DEVICE memory (below) ----------------------------------------------------------------------
 * sdp_grid_subsample replaces the CPython modules grid_subsampling.compute (method 0,
 *   "barycenters": grid_subsampling.cpp:46-102) and grid_subsampling_lidar.compute (method 1:
 *   grid_subsampling_lidar.cpp:46-120), wrapper.cpp:58-285.  points float32 [n][3], features
 *   float32 [n][fdim] or NULL, classes int32 [n][ldim] or NULL, voxel size sample_dl.  Outputs
 *   (capacity n rows each): out_points [m][3], out_features [m][fdim], out_classes [m][ldim];
 *   *out_n = m, in the reference's voxel order (see csrc/grid_subsampling.cpp).             */
int sdp_grid_subsample(const float* points, int64_t n, const float* features, int fdim, const int32_t* classes,
                       int ldim, float sample_dl, int method, float* out_points, float* out_features,
                       int32_t* out_classes, int64_t* out_n);

/* ---- voxel-grid subsampling on the DEVICE (method 0, "barycenters": grid_subsampling.cpp:46-102) ----
 * The same float32 arithmetic in the same order as sdp_grid_subsample with method 0, so every output
 * bit equals the host's; the rows come in ASCENDING VOXEL KEY (the host returns std::unordered_map
 * order: the two agree as sets), and a majority label with equal votes is the SMALLEST label value (the
 * host keeps the first maximum in hash order).  Inputs (DEVICE): points float32 [n][stride], stride 3
 * or 4, xyz first; features float32 [n][fdim] or NULL; classes int32 [n][ldim] or NULL.  A point with a
 * non-finite coordinate is skipped everywhere: no key, no vote, inverse = -1.  Outputs (DEVICE, capacity
 * n rows each; rows >= m are not written): out_points [m][3], out_features [m][fdim], out_classes
 * [m][ldim]; optional (NULL = skip) out_keys int64 [m] (ix + nx*iy + nx*ny*iz), out_counts int32 [m],
 * out_order int32 [points used] (the stable key-sorted permutation of the used point indices),
 * out_inverse int32 [n] (the output row of every point).  info int64 [5] = {m, nx, ny, nz, points used}:
 * m = 0 when no point is finite; m = -1 when the grid has more than 2^40 cells (nx*ny*nz > 2^40) --
 * then nothing but info is written.  Count / scan / scatter passes on `stream` (a stable 8-bit radix
 * sort of (key, point index), segment heads, per-voxel sums in ascending point index), no host
 * synchronisation, no floating-point atomics: bit-identical from run to run.  Point indices and rows
 * are int32: 1 <= n <= 2^30.  workspace: 16-byte aligned, sdp_voxel_grid_workspace_size(n) bytes.   */
int sdp_voxel_grid_workspace_size(int64_t n, size_t* bytes);
int sdp_voxel_grid(const float* points, int64_t n, int stride, const float* features, int fdim, const int32_t* classes,
                   int ldim, float sample_dl, float* out_points, float* out_features, int32_t* out_classes,
                   int64_t* out_keys /* or NULL */, int32_t* out_counts /* or NULL */, int32_t* out_order /* or NULL */,
                   int32_t* out_inverse /* or NULL */, int64_t* info /* [5] */,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Measurement hook (tools/voxel_bench.py): events = HOST array of 7 hipEvent_t that every later
 * sdp_voxel_grid of this thread records on its stream -- before the first kernel, then after the bounds,
 * the keys, the sort, the segment heads, the reduction and the labels (+ info); NULL switches it off.   */
int sdp_voxel_grid_stage_events(void* const* events);

/* ---- cloud-to-cloud distances on the DEVICE (csrc/cloud_nn.hip) ----
 * sdp_cloud_nn: for every query point the EXACT nearest target point within max_dist.  Inputs (DEVICE): q
 * float64 [nq][qstride], t float64 [nt][tstride], xyz first, stride 3 or 4; max_dist R > 0; cell c of the
 * acceleration grid with R/8 <= c <= R; center float64 [3] or NULL (zeros), finite: the grid runs on
 * float32(t - center).  Outputs (DEVICE): nn_d2 float64 [nq], nn_idx int32 [nq].
 *   d2(i,j) = ((qx-tx)*(qx-tx) + (qy-ty)*(qy-ty)) + (qz-tz)*(qz-tz) in float64, every operation rounded once,
 *   from the ORIGINAL coordinates.  Query i matches j* = argmin_j d2(i,j) over the targets with finite
 *   coordinates and d2(i,j) <= R*R (the rounded float64 product); among equal d2 the smallest j.  Then
 *   nn_d2[i] = d2(i,j*), nn_idx[i] = j*; a query without such a target, or with a non-finite coordinate, gets
 *   +inf and -1.  The result does not depend on cell or center, and two calls give identical bits.
 * The targets are put on a cell grid with sdp_voxel_grid's machinery (float32 keys, stable radix sort, segment
 * heads); each query visits the cells around its own in rings of growing Chebyshev distance up to
 * K = ceil((R + slack) / c), slack = 6 * 2^-23 * (max |float32 target coordinate| + R + 2c) covering every
 * float32 rounding of the cell assignment, and stops early once no unvisited ring can hold a nearer point
 * (derivation: the file header).  info int64 [8] = {occupied cells, nx, ny, nz, targets
 * used, K, brute flag, 0} (brute flag 1: the grid origin rounded above the targets' lower bound on an axis,
 * the cell keys are unusable and every query scanned all targets -- still exact, O(nq nt)); info[0] = -1 when the grid has more than 2^40 cells and -2 when the slack pushes K
 * beyond 9 (cell too small for the float32 grid at these coordinates: choose a center near the cloud or a
 * larger cell) -- then nothing but info is written.  max_dist / cell > 8 fails at the call.  nq = 0 or nt = 0
 * is valid.  0 <= nq, nt <= 2^30.  No host synchronisation, no floating-point atomics.
 * workspace: 16-byte aligned, sdp_cloud_nn_workspace_size(nq, nt) bytes.                                   */
int sdp_cloud_nn_workspace_size(int64_t nq, int64_t nt, size_t* bytes);
int sdp_cloud_nn(const double* q, int64_t nq, int qstride, const double* t, int64_t nt, int tstride, double max_dist,
                 double cell, const double* center /* or NULL */, double* nn_d2, int32_t* nn_idx, int64_t* info /* [8] */,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Measurement hook (tools/cloud_nn_bench.py): events = HOST array of 3 hipEvent_t that every later sdp_cloud_nn
 * of this thread records on its stream -- before the first kernel, after the grid build, after the queries;
 * NULL switches it off.                                                                                     */
int sdp_cloud_nn_stage_events(void* const* events);
/* sdp_cloud_nn_stats: the sums of one direction.  nn_d2 [n] from sdp_cloud_nn, q [n][qstride] its queries
 * (DEVICE), thresholds = HOST array of nthr <= 8 doubles in [0, max_dist] (beyond max_dist nothing was searched:
 * such a threshold fails).  out (DEVICE) float64 [5 + nthr] = {n_finite (queries with finite coordinates),
 * n_matched (nn_d2 < inf), sum_d = sum sqrt(d2), sum_d2, max_d (0 when nothing matched), cnt_k = #{d2 <=
 * tau_k*tau_k (rounded product)}} over the matched.  float64 throughout, correctly rounded sqrt, partial sums of
 * 256 points in a fixed tree and then one workgroup over the partials in a fixed order: bit-identical from run
 * to run, no atomics.   workspace: 16-byte aligned, sdp_cloud_nn_stats_workspace_size(n) bytes.              */
int sdp_cloud_nn_stats_workspace_size(int64_t n, size_t* bytes);
int sdp_cloud_nn_stats(const double* nn_d2, const double* q, int qstride, int64_t n, const double* thresholds, int nthr,
                       double max_dist, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- voxel occupancy and semantic IoU between two clouds on the DEVICE (csrc/voxel_iou.hip) ----
 * sdp_voxel_iou puts cloud A (the truth) and cloud B (the prediction) on ONE fixed grid and counts, per pair of
 * voxel states, the voxels of the grid: the confusion matrix that completion IoU and per-class IoU come from.
 *   Grid: origin float64 [3] (HOST) the low corner, voxel > 0 a float64 size, dims = (nx, ny, nz) (HOST int64 [3]),
 *     each >= 1, nx*ny*nz <= 2^40.
 *   Cell of a point: per axis i = floor((p - origin) / voxel) in float64 -- one subtraction, one IEEE division, one
 *     floor, each rounded once; no reciprocal, no FMA.  Cell key = ix + nx*iy + nx*ny*iz.
 *   A point is USED iff its three coordinates are finite, 0 <= i < n on every axis (tested on the floored double
 *     before any integer conversion: NaN, +-inf and 1e300 drop out), its label lies in [0, C) and its cell is valid.
 *   Labels: a_labels / b_labels int32 [n] (DEVICE) or NULL = every point has label 0; C = num_classes in [1, 64].
 *     A point whose label is outside [0, C) is not used; such points are counted (info[4], info[5]) whatever their
 *     coordinates.  The label of an occupied voxel is the label most of its used points carry; among equal counts
 *     the SMALLEST label value (sdp_voxel_grid's device rule).
 *   valid: DEVICE uint8 [nz][ny][nx] (key order) or NULL = every cell valid.  A cell with 0 takes no part anywhere
 *     and the points in it are not used.  A mask requires nx*ny*nz <= 2^31.
 *   Result: confusion int64 [(C+1)*(C+1)] (DEVICE), row = state in A, column = state in B; state 0 = empty, state
 *     1 + c = occupied with majority label c.  confusion[0][0] = valid cells - |A u B|, so the matrix sums to the
 *     number of valid cells.
 *   Optional outputs (DEVICE, NULL = skip; capacity na resp. nb rows, rows >= m are not written): the occupied
 *     cells of each side in ascending key, a_cells int64 [m_a], their majority labels a_cell_labels int32 [m_a] and
 *     their used-point counts a_cell_counts int32 [m_a]; the same for B.
 *   info int64 [8] (DEVICE) = {m_a, m_b, points used a, points used b, a points with a bad label, b points with a
 *     bad label, |A n B|, valid cells}.
 * Inputs (DEVICE): a float64 [na][astride], b float64 [nb][bstride], xyz first, stride 3 or 4; 0 <= na, nb <= 2^30,
 * an empty cloud is valid.  Bad dims, voxel <= 0 or not finite, a non-finite origin, C outside [1, 64], a mask with
 * more than 2^31 cells and a grid of more than 2^40 cells fail the call (sdp_last_error) and write nothing.
 * Per cloud: compaction of the used points in point order, a stable radix sort of the keys cell * 64 + label with
 * exactly ceil((ceil(log2(cells)) + 6) / 8) passes, segment heads by cell, one thread per voxel for the longest
 * label run.  Then every cell of A is searched in B's cells and every cell of B in A's; workgroups count their
 * pairs in LDS and one workgroup adds the partials in a fixed order.  All on `stream`, no host synchronisation, no
 * workgroup waits for another; the only atomics are integer LDS adds whose sums do not depend on their order:
 * every count is exact and two calls give identical bits.
 * workspace: 16-byte aligned, sdp_voxel_iou_workspace_size(na, nb, num_classes) bytes.                          */
int sdp_voxel_iou_workspace_size(int64_t na, int64_t nb, int num_classes, size_t* bytes);
int sdp_voxel_iou(const double* a, int64_t na, int astride, const int32_t* a_labels /* or NULL */,
                  const double* b, int64_t nb, int bstride, const int32_t* b_labels /* or NULL */,
                  const double* origin /* HOST [3] */, double voxel, const int64_t* dims /* HOST [3] */,
                  int num_classes, const uint8_t* valid /* DEVICE or NULL */,
                  int64_t* confusion /* DEVICE [(C+1)*(C+1)] */,
                  int64_t* a_cells, int32_t* a_cell_labels, int32_t* a_cell_counts,   /* each optional, capacity na */
                  int64_t* b_cells, int32_t* b_cell_labels, int32_t* b_cell_counts,   /* each optional, capacity nb */
                  int64_t* info /* DEVICE [8] */, void* workspace, size_t workspace_bytes, void* stream);
/* Measurement hook (tools/voxel_iou_bench.py): events = HOST array of 6 hipEvent_t that every later sdp_voxel_iou
 * of this thread records on its stream -- before the first kernel, then after the keys, the sorts, the segment
 * heads, the votes and the comparison; NULL switches it off.                                                    */
int sdp_voxel_iou_stage_events(void* const* events);

#ifdef __cplusplus
}
#endif
#endif
