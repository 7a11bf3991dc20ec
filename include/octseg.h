/* octseg.h -- C ABI of liboctseg_hip.so, the MI355X (gfx950) engine behind the OCT segmentation
 * hot path: encoder-decoder forward + backward + Dice loss + optimizer step.
 *
 * The reference (ViacheslavDanilov/oct_segmentation) has no FFI: its seam is Python.  Each entry
 * point below names the reference call it sits under (paths relative to the reference repo):
 *
 *   octseg_plan_create / _destroy      smp.create_model(arch, encoder_name, in_channels, classes)
 *                                      src/models/smp/model.py:38-44
 *   octseg_plan_set_dropout            the nn.Dropout2d inside smp's FPN decoder (arch "fpn") / the nn.Dropout of DeepLabV3+'s
 *                                      ASPP.project (arch "deeplabv3plus"): its keep pattern, injected
 *   octseg_plan_set_drop_connect       efficientnet_pytorch's drop_connect on the id skips of MBConv blocks (encoders "efficientnet-b*")
 *   octseg_plan_param_info / bn_info   the nn.Module parameter / buffer tree behind state_dict()
 *                                      (load_from_checkpoint, src/predict.py:39-48)
 *   octseg_net_forward                 OCTSegmentationModel.forward (normalize=1, model.py:65-71) and
 *                                      .predict's bare self.model(x) (normalize=0, model.py:192)
 *   octseg_dice_forward                smp.losses.DiceLoss(MULTILABEL_MODE, from_logits=True)
 *                                      (model.py:55,81,115) + smp.metrics.get_stats (utils.py:19-23)
 *   octseg_plan_set_loss               the choice of criterion at model.py:55 (the reference always builds DiceLoss; north_star also
 *                                      names BCE): Dice | torch.nn.functional.binary_cross_entropy_with_logits | their sum
 *   octseg_net_backward                loss.backward() that Lightning runs after training_step
 *                                      (model.py:73-95, train.py:130-133)
 *   octseg_net_train_step              training_step + loss.backward() as one call, optionally one replayed hipGraph (model.py:73-95)
 *   octseg_net_backward_sliced         the same under DDP: gradient buckets handed out while the backward still runs
 *                                      (train.py:122-133, devices > 1)
 *   octseg_optim_step                  configure_optimizers -> SGD|RMSprop|RAdam|Adam.step()
 *                                      (model.py:150-181)
 *   octseg_augment                     OCTDataset.get_img_augmentation applied in __getitem__ (dataset.py:119-123,160-207)
 *   octseg_ingest_image                OCTDataset.__getitem__'s cv2.resize of the uint8 BGR frame + to_tensor_shape (dataset.py:108-110,125) and
 *                                      preprocessing_img's cvtColor(RGB2BGR) + cv2.resize on the predict path (data/utils.py:159-166)
 *   octseg_ingest_mask                 the mask lines of __getitem__: cv2.resize(INTER_NEAREST), channel select, bool -> float, HWC -> CHW
 *                                      (dataset.py:111-118,125)
 *   octseg_mask_assemble               the per-frame epilogue of segment(): threshold, cv2 INTER_NEAREST resize to output_size,
 *                                      write into mask[:, :, CLASS_ID - 1] (src/predict.py:92-100, data/utils.py:16-33)
 *   octseg_vote_assemble               (no reference counterpart) the same epilogue voted by M members, the folds of
 *                                      src/data/convert_int_to_cv.py:73-93 and flipped / rotated views: mask, mean probability, dissent map, counts
 *   octseg_logit_histogram             (no reference counterpart) per frame and class, the 256-bin histogram of the predicted probability over
 *                                      the truth-negative and over the truth-positive pixels: every threshold's tp / fp / fn / tn by suffix sums
 *   octseg_render_results              save_results: closing, ring, blur, two alpha pastes per class into the frame, the flat colour mask
 *                                      (src/data/utils.py:195-235, get_img_mask_union_pil src/models/smp/utils.py:203-213)
 *   octseg_epoch_panels                log_predict_model_on_epoch, the per-epoch image | ground truth | prediction strips and the two W&B label
 *                                      maps (src/models/smp/model.py:208-271, called from on_validation_epoch_end, model.py:134-148)
 *   octseg_stack_measure               the measurements of the app's get_analysis: set pixels per slice and class, and the ray walk of
 *                                      calculate_object_thickness per slice, class and degree (src/app/tools/analysis.py:60-130,189,199-200)
 *   octseg_stack_polar / octseg_frames_unwrap
 *                                      (no reference counterpart) the rays of calculate_object_thickness walked to their end: first entry, first
 *                                      exit, last set step, set steps and runs per slice, class and degree; the polar label map and frame view
 *   octseg_stack_moments / octseg_moment_origins / octseg_stack_polar_at
 *                                      (no reference counterpart) raw moments to second order, bounding box and crack perimeter of every mask
 *                                      plane; its centroid as a pixel; the polar profile walked from that pixel: lumen area and diameters
 *   octseg_stack_components / octseg_stack_cleanup / octseg_components_scratch_bytes
 *                                      MaskProcessor.smooth_mask / .remove_artifacts, which process_pair runs over every annotated object
 *                                      (src/data/mask_processor.py:5-37, src/data/convert_int_to_cv.py:191-199)
 *   octseg_stack_contour_counts / octseg_stack_contours / octseg_contours_scratch_bytes
 *                                      (no reference counterpart) the crack contours of every mask plane: closed integer polygons along pixel
 *                                      sides with holes, areas, perimeters, bounds and the owning component; not cv2.findContours
 *   octseg_stack_boundary / octseg_stack_distance / octseg_pair_distance_counts / _keys / _min / octseg_distance_scratch_bytes
 *                                      (no reference counterpart) exact squared Euclidean distance maps of the mask planes, the directed
 *                                      boundary-distance lists behind HD / HD95 / ASSD, the smallest distance between two classes
 *   octseg_volume_boundary / octseg_volume_distance / octseg_volume_pair_distance_counts / _keys / _min / octseg_volume_distance_scratch_bytes
 *                                      (no reference counterpart) the same over the volume the slices form, slice_step pixels apart: the
 *                                      6-neighbour boundary, exact 3-D squared distance maps in bands of rows, the volumetric HD / HD95 / ASSD
 *                                      lists per pair of channels, the smallest distance across slices with its voxel
 *   octseg_stack_signed_distance / octseg_signed_blend / octseg_signed_distance_scratch_bytes
 *                                      (no reference counterpart) signed squared distance maps of the mask planes and the blend of two of them
 *                                      by integer weights: slices interpolated between their neighbours, gaps bridged, stacks resampled
 *   octseg_stack_skeleton / octseg_skeleton_scratch_bytes
 *                                      (no reference counterpart) the centreline of every mask plane by Guo and Hall's parallel thinning and its
 *                                      census: set and skeleton pixels, end, junction and isolated points, passes
 *   octseg_stack_prune / octseg_prune_scratch_bytes
 *                                      (no reference counterpart) that centreline pruned: spurs removed, ends trimmed, a component that would
 *                                      vanish restored; tips, end and junction points, orthogonal and diagonal links (the arc length)
 *   octseg_volume_components / octseg_volume_cleanup / octseg_lesions_scratch_bytes
 *                                      (no reference counterpart) the connected components of a mask stack across its slices: labels, the 32
 *                                      largest lesions per class with their extents, the per-slice area profile, the flicker filter
 *   octseg_volume_match / octseg_match_scratch_bytes
 *                                      (no reference counterpart) predicted against annotated lesions: both stacks' ranked lesions, the 33 x 33
 *                                      table of shared voxels by lesion rank per class, per-slice |P & T|, |P|, |T|
 *   octseg_volume_normalize            cv2.normalize(slice, None, 0, 255, NORM_MINMAX, CV_8U) + cvtColor(BGR2RGB) of every slice of a DICOM's
 *                                      pixel_array (src/data/convert_dicoms.py:71-81, src/app/tools/analysis.py:167-177)
 *   octseg_resize_pil_u8               data_processing's Image.open(p).resize(output_size), Pillow's default BICUBIC (src/data/utils.py:187)
 *   octseg_plan_set_frozen_bn / octseg_plan_cam_target / octseg_net_backward_seeded / octseg_cam_maps
 *                                      CAMProcessor.extract_activation_map / overlay_activation_map over pytorch-grad-cam on model.eval()
 *                                      (src/models/cam_processor.py:83-98, src/models/visualize_activation_maps.py:102-199)
 *   octseg_plan_set_graph              (serving option, no reference counterpart) eval forwards of predict()
 *                                      (model.py:183-200) replayed as one hipGraph
 *   octseg_plan_params_changed         optimizer.step() / load_state_dict() side effect: weight images are stale
 *   octseg_conv2d_* / _convT_*         torch conv2d / conv_transpose2d primitives, exported so the
 *                                      parity tests can pin every kernel against torch CPU in isolation
 *   octseg_profile_* / octseg_debug_*  measurement aids of bench.py and tools/ (HIP-event brackets per launch, one-stream
 *                                      mode, s_memtime stamps in -DOCTSEG_STAMP builds); no reference counterpart
 *
 * Conventions: every function returns 0 on success or a negative octseg_status; the message of the
 * last failure on the calling thread is octseg_last_error().  Nothing throws across the ABI.  The
 * caller owns every buffer (device pointers, plain sizes); the library only enqueues kernels on the
 * caller's hipStream_t (passed as void*) and never synchronises or allocates in hot calls.  Plans
 * are thread-compatible (no concurrent calls on one plan).
 */
#ifndef OCTSEG_H
#define OCTSEG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  OCTSEG_OK = 0,
  OCTSEG_BAD_SHAPE = -1,        /* e.g. H or W not divisible by 32 (smp check_input_shape) */
  OCTSEG_BAD_DTYPE = -2,
  OCTSEG_UNSUPPORTED_ARCH = -3, /* unknown arch / encoder name */
  OCTSEG_HIP_ERROR = -4,
  OCTSEG_BAD_ARG = -5
} octseg_status;

/* OCTSEG_F16: IEEE half storage + v_mfma_f32_32x32x16_f16, the serving dtype of the ensemble path (reference src/predict.py; BASELINE
 * config #5).  Eval forwards only: octseg_net_forward(train = 1) and the backward entry points return OCTSEG_BAD_DTYPE for it. */
typedef enum { OCTSEG_F32 = 0, OCTSEG_BF16 = 1, OCTSEG_F16 = 2 } octseg_dtype;

typedef struct {
  const char* arch;     /* "unet" | "unetplusplus" | "linknet" | "fpn" | "deeplabv3plus" | "deeplabv3" | "pspnet" (case-insensitive) */
  const char* encoder;  /* "resnet18" | "resnet34" | "resnet50" | "resnet101" | "resnet152" | "timm-regnetx_002" | "timm-regnetx_064" |
                           "timm-regnety_120" | "efficientnet-b0" | "efficientnet-b5" | "efficientnet-b7" (smp encoder names) */
  int classes;          /* output channels */
  int batch, height, width;
  int dtype;            /* octseg_dtype: storage/MFMA input type of activations (accumulate is f32) */
} octseg_net_desc;

typedef struct octseg_plan octseg_plan;

/* kinds of parameter layout inside the flat fp32 parameter arena */
enum {
  OCTSEG_P_CONV = 0,   /* [R][S][O][I]  <- torch Conv2d weight [O][I][R][S]           */
  OCTSEG_P_CONVT = 1,  /* [R][S][O][I]  <- torch ConvTranspose2d weight [I][O][R][S]  */
  OCTSEG_P_STEM = 2,   /* [O][KP], k=(r*7+s)*3+ci zero padded to KP <- [O][3][7][7]   */
  OCTSEG_P_VEC = 3     /* bias / BN weight / BN bias, [O]                              */
};
typedef struct {
  char name[128];      /* state_dict key relative to the smp model, e.g. "encoder.layer1.0.conv1.weight" */
  int kind;
  int R, S, O, I, KP;
  size_t offset;       /* element offset into the parameter (and gradient) arena */
  size_t numel;
} octseg_param_info;
typedef struct {
  char name[128];      /* module path, e.g. "encoder.bn1"; buffers are <name>.running_mean / running_var */
  int C;
  size_t mean_offset, var_offset; /* element offsets into the buffer arena */
} octseg_bn_info;

int octseg_version(void);
const char* octseg_last_error(void);

int octseg_plan_create(const octseg_net_desc* desc, octseg_plan** out);
int octseg_plan_destroy(octseg_plan* plan);
size_t octseg_plan_workspace_bytes(const octseg_plan* plan);
size_t octseg_plan_param_numel(const octseg_plan* plan);   /* fp32 elements of the param / grad arenas */
size_t octseg_plan_buffer_numel(const octseg_plan* plan);  /* fp32 elements of the BN buffer arena */
int octseg_plan_num_params(const octseg_plan* plan);
int octseg_plan_param_info(const octseg_plan* plan, int index, octseg_param_info* out);
int octseg_plan_num_bn(const octseg_plan* plan);
int octseg_plan_bn_info(const octseg_plan* plan, int index, octseg_bn_info* out);
double octseg_plan_fwd_macs(const octseg_plan* plan);      /* conv multiply-accumulates of one forward */
/* multiply-accumulates a TRAINING step executes per pass: out3 = {forward, data gradient, weight gradient}.  Equal to fwd_macs unless the
 * plan runs the decoder's (nearest x2, concat, 3x3) layers as a 4x4 stride-2 transposed conv over the low-resolution map plus a 3x3 over the
 * skip channels (OCTSEG_TIED): the same function of the same weights in 16 instead of 36 products per source pixel. */
int octseg_plan_exec_macs(const octseg_plan* plan, double* out3);
/* test hook: workspace byte offsets of the raw output (NHWC, plan dtype) of conv layer `conv_name`
 * (module path, e.g. "decoder.blocks.0.conv1.0") and of its gradient; dims = {N,H,W,C}. */
int octseg_plan_find_tensor(const octseg_plan* plan, const char* conv_name, size_t* act_off,
                            size_t* grad_off, int* dims);

/* Measurement hooks (bench.py): between _start and _stop every MFMA conv launch and every BatchNorm sweep is bracketed
 * by HIP events on its launch stream.  _stop synchronises the device and fills out[12]:
 * out[3k+0..2] = {milliseconds, algorithmic work, launches} for k = 0 conv forward, 1 conv data-gradient, 2 weight
 * gradient (work = FLOPs) and k = 3 the HBM-bound BatchNorm sweeps bn_act / bn_bwd_reduce / bn_bwd_apply (work = bytes
 * every tensor they read or write once). */
int octseg_profile_start(void);
int octseg_profile_stop(double* out);

/* The forward packs the fp32 parameters into the kernels' weight images (bf16 / f32, LDS-slab order) and
 * reuses them on later calls with the same (params, workspace) pointers.  Call this after anything that
 * changes the parameter arena in place: optimizer.step(), load_state_dict(), an all-reduce of parameters. */
int octseg_plan_params_changed(octseg_plan* plan);

/* arch "fpn" (smp FPN, one of the reference's sweep architectures: configs/tune.yaml:9-18 through smp.create_model, model.py:38-44):
 * the Dropout2d(0.2) behind the merge needs a keep pattern in training -- device float [batch][128] of 0 / 1, caller-owned, read by the
 * next training forward AND its backward (kept channels are scaled by 1 / (1 - 0.2), torch's Dropout2d).  Eval forwards ignore it. */
/* arch "deeplabv3plus" (smp DeepLabV3Plus at its defaults: encoder_output_stride 16, decoder_channels 256, atrous rates (12, 24, 36);
 * same sweep, same call): the keep pattern is per ELEMENT of ASPP.project's output -- device float [batch][H/16][W/16][256] (NHWC) of
 * 0 / 1, kept elements scaled by 1 / (1 - 0.5).  A training forward with batch 1 fails like torch does ("Expected more than 1 value per
 * channel when training": the pooled ASPP branch's BatchNorm).
 * arch "deeplabv3" (smp DeepLabV3 at its defaults: output stride 8, dense ASPP): as "deeplabv3plus" with [batch][H/8][W/8][256].
 * arch "pspnet" (smp PSPNet at its defaults: encoder_depth 3, psp_out_channels 512, upsampling 8): Dropout2d(0.2) behind the fuse conv,
 * device float [batch][512] of 0 / 1.  Its parameter table still lists encoder.layer3 / layer4 (smp keeps them in state_dict): they
 * never run and their gradients are zero. */
int octseg_plan_set_dropout(octseg_plan* plan, const float* keep_dev);

/* encoder "efficientnet-b0" | "-b5" | "-b7" (efficientnet_pytorch through smp's EfficientNetEncoder; reference sweep configs/tune.yaml:25-28):
 * every MBConv block with an identity skip applies drop_connect in training -- x / (1 - rate) * floor(1 - rate + U[0, 1)) per sample, rate =
 * 0.2 * block index / blocks.  The caller draws the decisions and hands over the FACTORS: device float [octseg_plan_num_drop_connect()][batch]
 * of 0 or 1 / (1 - octseg_plan_drop_connect_rate(i)), caller-owned, read by the next training forward AND its backward.  Eval ignores it. */
int octseg_plan_set_drop_connect(octseg_plan* plan, const float* factors_dev);
int octseg_plan_num_drop_connect(const octseg_plan* plan);
float octseg_plan_drop_connect_rate(const octseg_plan* plan, int index);

/* Serving path (reference: src/models/smp/predict.py segment(), model.py:183-200 predict()): enable = 1 makes every
 * eval-mode octseg_net_forward of this plan run as a hipGraph -- the first call with a given argument set runs
 * eagerly, the second is captured, later ones replay it (one launch instead of ~400) for as long as the pointers,
 * the stream and the normalisation constants stay the same.  Keep the image / logits in persistent buffers. */
int octseg_plan_set_graph(octseg_plan* plan, int enable);

/* image: NCHW f32 [B,3,H,W]; logits: NCHW f32 [B,classes,H,W]; mean/std: 3 host floats (normalize=1).
 * train=1: batch statistics, running buffers updated, activations kept for backward -- and `image` itself must stay valid and
 * unchanged until that backward has been enqueued: the stem's weight gradient gathers the frame again instead of saving an im2col copy. */
int octseg_net_forward(octseg_plan* plan, const float* params, float* buffers, void* workspace,
                       const float* image, float* logits, int normalize, const float* mean,
                       const float* stdv, int train, void* stream);

/* Training augmentation on the GPU (reference src/models/smp/dataset.py:160-207: HorizontalFlip, ShiftScaleRotate, RandomCrop +
 * PadIfNeeded, GaussNoise, Perspective, RandomBrightnessContrast, HueSaturationValue).  The host draws the per-frame
 * decisions and parameters (oct_segmentation_amd/augment.py mirrors the reference's probabilities and ranges) and passes
 * OCTSEG_AUG_NPARAM floats per frame: [0..8] inverse homography (output pixel -> source pixel), [9] contrast alpha,
 * [10] brightness beta (x 255), [11] noise sigma, [12] seed bits, [13..15] hue / saturation / value shifts in OpenCV
 * 8-bit units, [16] flags (bit 0: HSV shift on), [20..28] inverse homography output pixel -> frame after crop + pad,
 * [29..32] crop window [x_lo, y_lo, x_hi, y_hi) in that frame (outside = padding = 0).  One bilinear gather of the image (constant-0 border), one nearest
 * gather per mask channel, photometric ops on the pixel, result clipped and rounded to the uint8 grid. */
#define OCTSEG_AUG_NPARAM 36
int octseg_augment(const float* img, const float* mask, float* img_out, float* mask_out, const float* params, int B,
                   int classes, int H, int W, void* stream);

/* Serving epilogue (reference src/predict.py:92-100): out[n][y][x][out_ch] = sigmoid(logits[n][ch]) > 0.5 after a nearest
 * resize from H x W to out_h x out_w.  logits: NCHW f32 [N,classes,H,W]; out: NHWC f32 [N,out_h,out_w,out_channels] (the
 * reference's 4-channel mask stack, channel = CLASS_ID - 1).  row_index[out_h] / col_index[out_w]: device int32 source
 * index of every output row / column -- the host mirror fills them with OpenCV's INTER_NEAREST rule (resizeNN:
 * min(floor(i * (1 / (out / in))), in - 1), what the reference's cv2.resize call computes); null = floor((i + 0.5) * H / out_h). */
int octseg_mask_assemble(const float* logits, int N, int classes, int H, int W, int ch, float* out, int out_h, int out_w,
                         int out_channels, int out_ch, const int* row_index, const int* col_index, void* stream);

/* Voted serving epilogue (no reference counterpart: the reference trains five folds per class, src/data/convert_int_to_cv.py:73-93, and serves
 * one; DESIGN.md section 5k, pinned to tests/vote_ref.py): ONE mask from M member networks -- folds, and every fold on flipped / rotated views of
 * the frame -- with the map of where they disagree.  One launch per (batch of frames, output class).
 *
 * Members: logits / classes / ch / view are HOST arrays [M], 1 <= M <= OCTSEG_VOTE_MAX_MEMBERS; they travel to the kernel in its argument, by
 * value (no table upload, no synchronisation).  logits[m]: device f32 NCHW [N][classes[m]][Hm][Wm], of which channel ch[m] votes; view[m] in 0..7.
 * View code v = a + 2 b + 4 t.  The view of a frame X[H][W] is made in this order: transpose if t (needs H == W), reverse the rows if b, reverse
 * the columns if a (torch: Y = X.transpose(-1, -2) if t; Y = Y.flip(-2) if b; Y = Y.flip(-1) if a) -- the eight codes are the dihedral group D4.
 * A member's logits live in ITS VIEW's coordinates; H, W are the extents of the un-viewed frame, a member with t is [N][classes][W][H] (the
 * same extents).  The kernel undoes the view while it reads: for the source pixel (sy, sx) of the un-viewed frame, (p, q) = t ? (sx, sy) : (sy, sx),
 * (Ht, Wt) = t ? (W, H) : (H, W), and the member is read at (b ? Ht - 1 - p : p, a ? Wt - 1 - q : q) with row length Wt.
 * Resize: exactly octseg_mask_assemble's rule -- row_index[out_h] / col_index[out_w] device int32 tables that index the un-viewed frame, null =
 * floor((i + 0.5) * H / out_h); indices are clamped on the device.
 *
 * Per output pixel, with s_m = the engine's one fp32 sigmoid of member m's logit (the one behind octseg_mask_assemble and the Dice kernel):
 *   votes = #{m : s_m > 0.5f};
 *   mode OCTSEG_VOTE_SOFT:     pbar = (s_0 + s_1 + ... + s_{M-1}) / (float)M, the sum in f32 in member order; mask = pbar > 0.5f;
 *   mode OCTSEG_VOTE_MAJORITY: mask = 2 * votes > M -- a tie is NOT set; pbar as above for the optional output;
 *   dissent = mask ? M - votes : votes, the number of members whose own threshold differs from the written mask.
 * Outputs, channel-last like the stack, written at channel out_ch only (other channels are left untouched):
 *   out     f32   [N][out_h][out_w][out_channels], 0.0 / 1.0; required;
 *   prob    f32   same shape, pbar; nullable;
 *   dissent uint8 same shape; nullable;
 *   stats   int32 [N][4], nullable: over the output pixels of each frame, the number set, disputed (0 < votes < M), disputed and set, and the sum
 *           of dissent.  Integers only, so they are exact and reproducible; cleared on the stream by the call, then one atomic per workgroup.
 * With M == 1 and view 0, out equals octseg_mask_assemble's bit for bit.
 * Enqueue only (one clear of stats, one launch).  Refused before any HIP call, octseg_last_error() naming the offending member: a null required
 * pointer or member pointer, mode not 0 / 1: OCTSEG_BAD_ARG; M outside 1..64, an extent <= 0, more than 65535 frames, ch[m] outside
 * [0, classes[m]), out_ch outside [0, out_channels), view[m] outside 0..7, a t view with H != W: OCTSEG_BAD_SHAPE. */
#define OCTSEG_VOTE_MAX_MEMBERS 64
#define OCTSEG_VOTE_SOFT 0
#define OCTSEG_VOTE_MAJORITY 1
int octseg_vote_assemble(const float* const* logits, const int* classes, const int* ch, const int* view, int M, int N, int H, int W, int mode,
                         float* out, int out_h, int out_w, int out_channels, int out_ch, const int* row_index, const int* col_index, float* prob,
                         uint8_t* dissent, int* stats, void* stream);

/* Logit histograms (no reference counterpart: the reference scores per-class DSC at the one threshold 0.5, src/models/smp/utils.py:13-36; DESIGN.md
 * section 5l, pinned to tests/curves_ref.py): per frame and class, how many pixels fall into each of OCTSEG_CURVE_BINS probability bins, counted
 * once over the truth-negative and once over the truth-positive pixels.  One streaming pass over logits and target; every threshold's confusion
 * counts, and from them ROC, precision-recall, reliability and the DSC-optimal cut, follow on the host from 2 KB per frame and class.
 *
 *   logits  device f32 NCHW [N][classes][H][W];
 *   target  device f32 NCHW [N][classes][H][W], octseg_dice_forward's target: a pixel is POSITIVE iff its value is != 0;
 *   hist    device int32 [N][classes][2][OCTSEG_CURVE_BINS], label-major: hist[n][c][0][j] counts the truth-negative pixels of frame n, class c in
 *           bin j, hist[n][c][1][j] the truth-positive ones.  The call clears it on the stream, then launches once; required.
 *
 * Bin rule, per pixel, all in f32:
 *   p   = the engine's one fp32 sigmoid of the logit z (the one behind octseg_mask_assemble, octseg_vote_assemble and the Dice kernel):
 *         e = expf(-|z|); p = z >= 0 ? 1 / (1 + e) : e / (1 + e);
 *   bin = clamp((int)ceilf(p * 256.0f) - 1, 0, 255).  The product is by a power of two and therefore exact.
 * Bin j holds p in (j / 256, (j + 1) / 256], and p == 0 falls into bin 0.  A pixel is predicted at threshold k / 256, k = 1 .. 255, iff
 * bin >= k, which is exactly p > k / 256 in f32: tp(k) = sum of hist[n][c][1][j] over j >= k, fp(k) the same of hist[n][c][0], fn and tn the
 * sums over j < k.  At k = 128 this is the engine's `sigmoid > 0.5f` pixel for pixel: z = +-0 and |z| = 1e-9 give p == 0.5 exactly, bin 127,
 * not set.  k = 0 (every pixel set) and k = 256 (none) follow from the row totals; a row's 512 counts sum to H * W.
 * Integers only: the counts are exact and do not depend on the order in which workgroups finish.
 *
 * Enqueue only; logits and target are read, never written, and may be any 4-byte-aligned device addresses.  Every refusal happens before any HIP
 * call, launches nothing and leaves hist untouched.  Null pointer: OCTSEG_BAD_ARG; N, classes, H or W <= 0, H * W >= 2^31, or N * classes > 65535
 * (one launch takes a plane per grid row): OCTSEG_BAD_SHAPE. */
#define OCTSEG_CURVE_BINS 256
int octseg_logit_histogram(const float* logits, const float* target, int N, int classes, int H, int W,
                           int* hist, void* stream);

/* Input half of the pipeline (reference src/models/smp/dataset.py:108-127, src/data/utils.py:159-166): the decoded uint8 arrays go to the
 * device as they are and come out as the float32 NCHW batch octseg_net_forward takes.  Integer arithmetic from host-made tables: the result
 * EQUALS cv2.resize's (OpenCV 4.8.1), no tolerance.
 *
 * octseg_ingest_image: src uint8 [B][src_h][src_w][3] (HWC), out f32 [B][3][dst_h][dst_w], values 0..255 = cv2.resize(frame, (dst_w, dst_h)) with
 * the default INTER_LINEAR; swap_rb != 0 writes source channel 2 - c to plane c (an RGB source becomes BGR planes).
 * xtab: device int32 [4][dst_w], ytab: device int32 [4][dst_h]; per output coordinate d: tab[0][d] = first tap's source index, tab[1][d] = the
 * second tap's (both already clipped to the source axis), tab[2][d] / tab[3][d] = their coefficients, cvRound(c * 2048).  The horizontal table
 * zeroes the fraction where the left tap leaves the row, the vertical one keeps it (resize.cpp resize_ / resizeGeneric_Invoker); the host
 * mirror builds both (oct_segmentation_amd/ingest.py from predict.cv2_linear_coeffs).  Horizontal pass s[x0] * a0 + s[x1] * a1 in int32, vertical
 * pass (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, clipped to 0..255.  When src_w == 2 * dst_w and src_h == 2 * dst_h
 * cv::resize switches to INTER_AREA: the taps of the tables are used, the coefficients are not, and the sample is (a + b + c + d + 2) >> 2.
 * Taps outside the source are clamped on the device: tables that are not a resize's give wrong samples, never a stray read.
 *
 * octseg_ingest_mask: src uint8 [B][src_h][src_w][src_channels] (the reference's 4-channel TIFF), channel_ids: device int32 [C] source channel
 * of every output plane (CLASS_IDS[name] - 1; not checkable on the host, ids outside [0, src_channels) are clamped on the device),
 * row_index [dst_h] / col_index [dst_w]: device int32 source index of every output row / column (resizeNN's rule, as for octseg_mask_assemble;
 * required here), out f32 [B][C][dst_h][dst_w] = src[b][row_index[y]][col_index[x]][channel_ids[c]] != 0 ? 1 : 0.
 *
 * Both: out must not overlap src; enqueue only.  Null pointer: OCTSEG_BAD_ARG; B, C, src_channels or an extent <= 0: OCTSEG_BAD_SHAPE. */
int octseg_ingest_image(const uint8_t* src, int B, int src_h, int src_w, int swap_rb, float* out, int dst_h, int dst_w, const int* xtab,
                        const int* ytab, void* stream);
int octseg_ingest_mask(const uint8_t* src, int B, int src_h, int src_w, int src_channels, const int* channel_ids, int C, float* out, int dst_h,
                       int dst_w, const int* row_index, const int* col_index, void* stream);
/* Measurement aid: 0 (default) = the shipped ingest kernels, 1 = their one-thread-per-output-pixel gather forms (tools/bench_ingest.py times
 * one beside the other).  Same results. */
int octseg_debug_set_ingest_variant(int variant);

/* Output half of the pipeline: save_results (reference src/data/utils.py:195-235) with get_img_mask_union_pil (src/models/smp/utils.py:203-213)
 * and the class colours / ids of src/data/utils.py:16-43, for a whole batch in ONE launch.
 * stack: f32 [N][H][W][stack_channels], values 0 / 1 (what octseg_mask_assemble writes; any value != 0 counts as set); frames: uint8
 * [N][H][W][3] RGB, the frame already at output size; class_channels: device int32 [C] stack channel of every class (CLASS_IDS[name] - 1; ids
 * outside [0, stack_channels) are clamped on the device, as in octseg_ingest_mask); class_rgb: device uint8 [C][3]; alpha_table: device uint8
 * [257]; overlay / color_mask: uint8 [N][H][W][3], must not overlap the inputs.  Per frame, for class c = 0..C-1 IN ORDER, m0 = stack[..., ch_c] != 0:
 *   m    = erode^it(dilate^it(m0)), it = close_iterations, element = cv2.getStructuringElement(MORPH_ELLIPSE, (5, 5)) (row widths 1,5,5,5,1);
 *   ring = dilate(m, ellipse(7, 7)) and not erode(m, ellipse(7, 7)) (row widths 1,5,7,7,7,5,1).  OpenCV's morphology border: positions outside
 *          the frame do not take part -- 0 for every dilation, 1 for every erosion, at every one of the iterated stages;
 *   k    = sum over the 5 x 5 window of (1,4,6,4,1) x (1,4,6,4,1) * m with BORDER_REFLECT_101 = 256 * cv2.GaussianBlur(m, (5, 5), 0), an integer 0..256;
 *   overlay = paste(paste(overlay, rgb_c, alpha_table[k]), rgb_c, ring ? ring_alpha : 0), starting from frames, with PIL's
 *          paste(in, col, a) = ((t >> 8) + t) >> 8, t = in * (255 - a) + col * a + 128 per channel;
 *   color_mask = rgb_c where m0 is set (the RAW mask), starting from (128, 128, 128); later classes overwrite earlier ones.
 * The host mirror (oct_segmentation_amd/postprocess.py) fills alpha_table[k] = uint8(k / 256 * 64 * 0.85 * 255) and ring_alpha = uint8(255 * 0.85 * 255)
 * with the reference's float64 order of operations and numpy's wrapping cast (alpha_table[256] = 48, ring_alpha = 231).  Integer arithmetic
 * throughout: both outputs EQUAL the reference's, no tolerance.
 * Enqueue only.  Null pointer: OCTSEG_BAD_ARG; N, H, W, C, stack_channels <= 0, C > 16 or close_iterations outside 1..3: OCTSEG_BAD_SHAPE. */
int octseg_render_results(const float* stack, const uint8_t* frames, int N, int H, int W, int stack_channels, const int* class_channels,
                          const uint8_t* class_rgb, int C, const uint8_t* alpha_table, int ring_alpha, int close_iterations, uint8_t* overlay,
                          uint8_t* color_mask, void* stream);

/* The per-epoch sample dump of the training loop: log_predict_model_on_epoch (reference src/models/smp/model.py:208-271, called from
 * on_validation_epoch_end, model.py:134-148, when epoch % img_save_interval == 0) with the class colours / ids of src/data/utils.py:16-45, for a
 * group of N frames that share a ground-truth source size, in ONE launch.
 * frames: f32 [N][3][S][S], BGR planes of the frame already at input size, integer values 0..255 (what octseg_ingest_image writes: model.py:214-215);
 * logits: f32 [N][C][S][S], the un-normalised forward of those frames (model.py:223-226, 192); gt: uint8 [N][src_h][src_w][src_channels], the RAW
 * samples of the 4-channel TIFF at its own size (model.py:216); row_index [S] / col_index [S]: device int32 source index of every output row /
 * column (resizeNN's rule, as for octseg_ingest_mask; required: model.py:217-221 is cv2.resize INTER_NEAREST); gt_channels: device int32 [C], the
 * source channel of every class (CLASS_IDS[name] - 1; ids outside [0, src_channels) are clamped on the device, as in octseg_ingest_mask);
 * class_rgb: device uint8 [C][3]; class_ids: device uint8 [C] (CLASS_IDS[name]).
 * panels: uint8 [N][S][3 * S][3], RGB interleaved -- per row the frame with its planes reversed to RGB, then the ground-truth colour mask, then
 * the prediction's: decoded as RGB this is what cv2.imwrite of the reference's BGR hstack (model.py:241-248) decodes to.  Both colour masks
 * start (128, 128, 128); for class c = 0..C-1 IN ORDER (model.py:234-239) the ground truth takes class_rgb[c] where
 * gt[n][row_index[y]][col_index[x]][gt_channels[c]] == 255 -- exactly 255, not != 0 -- and the prediction where sigmoid(logits[n][c][y][x]) > 0.5,
 * the same fp32 sigmoid as octseg_mask_assemble and the Dice kernel; later classes overwrite earlier ones.
 * labels: uint8 [N][2][S][S] or null (skipped): plane 0 the prediction, plane 1 the ground truth, class_ids[c] where the colour mask took
 * class c's colour, 0 elsewhere (wandb_mask_inference / wandb_mask_ground_truth, model.py:232-239).
 * Comparisons and integer moves only: the outputs EQUAL the reference's, no tolerance.  Outputs must not overlap inputs.  Enqueue only.
 * Null pointer (but labels): OCTSEG_BAD_ARG; N, S, C, src_h, src_w or src_channels <= 0, or C > 16: OCTSEG_BAD_SHAPE. */
int octseg_epoch_panels(const float* frames, const float* logits, const uint8_t* gt, int N, int S, int C, int src_h, int src_w, int src_channels,
                        const int* row_index, const int* col_index, const int* gt_channels, const uint8_t* class_rgb, const uint8_t* class_ids,
                        uint8_t* panels, uint8_t* labels, void* stream);

/* The device part of the app's get_analysis (src/app/tools/analysis.py:133-250) for a pullback of N slices.  stack: f32 [N][H][W][stack_channels]
 * (what octseg_mask_assemble writes; any value != 0 counts as set, as in octseg_render_results).  counts: int32 [N][stack_channels], the number of
 * set pixels (np.nonzero, analysis.py:199-200; a class is present in a slice iff 0 < count < H * W, np.unique at analysis.py:189).
 * radii: int32 [N][stack_channels][360], the ray walk of calculate_object_thickness (analysis.py:60-130) without trigonometry on the device:
 *   ray_pix: device int32 [360][R], linear pixel index y * W + x of step r = 1 .. R of the ray at `angle` degrees, made by the host as
 *            x = int(W / 2 + r * cos(radians(angle))), y = int(H / 2 + r * sin(radians(angle))) in CPython's double arithmetic (ids outside
 *            [0, H * W) are clamped on the device: a wrong table gives wrong samples, never a stray read); may be null when R == 0;
 *   ray_len: device int32 [360], the number of leading steps inside the frame (clamped to [0, R] on the device); later steps are never read.
 * With v[r] = stack[n][ray_pix[angle][r - 1]][c] != 0 for r = 1 .. ray_len[angle]: f = the first r with v[r] set -- none: radius 0 (the
 * reference's radii are >= 1, so 0 means "no object on this ray"); g = the first r > f with v[r] clear: radius g - 1 -- none: radius
 * ray_len[angle].  A gap before the object is skipped, the first gap after it ends the ray, leaving the frame ends it found or not; the
 * walk starts at step 1 (the centre is sampled only where truncation brings a later step back to it).  Integer results: they EQUAL the reference's, no tolerance.  The host mirror
 * (oct_segmentation_amd/analysis.py) makes the table and turns counts and radii into the app's dict.
 * Enqueue only (one clear of counts, two launches).  Null pointer: OCTSEG_BAD_ARG; N, H, W, stack_channels <= 0, stack_channels > 16, R < 0 or
 * H * W >= 2^31: OCTSEG_BAD_SHAPE. */
int octseg_stack_measure(const float* stack, int N, int H, int W, int stack_channels, const int* ray_pix, const int* ray_len, int R, int* counts,
                         int* radii, void* stream);

/* The polar plaque profile: the rays of calculate_object_thickness (reference src/app/tools/analysis.py:60-130; the rays from the frame centre
 * are the A-lines of a catheter-centred frame) walked to their END.  The reference's walk -- and radii of octseg_stack_measure -- stops at
 * the first exit, which for anything but the lumen is the distance of the object's far edge, not its thickness; no reference counterpart
 * states where an object begins on the ray or what lies behind it.  stack, ray_pix, ray_len, R: as for octseg_stack_measure, but
 * stack_channels <= 8 (the label map keeps one bit per class in a byte).  With len = min(max(ray_len[angle], 0), R) and
 * v[r] = stack[n][ray_pix[angle][r - 1]][c] != 0 for r = 1 .. len, prof: int32 [N][stack_channels][360][5] =
 *   0 IN    the first r with v[r]; 0 if none (steps start at 1);
 *   1 OUT   g - 1 for the first clear step g > IN; len if the run reaches the ray's end; 0 if none.  By definition the value
 *           octseg_stack_measure writes to radii;
 *   2 LAST  the last r with v[r]; 0 if none;
 *   3 HITS  the number of r with v[r];
 *   4 RUNS  the number of maximal runs of set steps.
 * map (may be NULL): uint8 [N][360][R], entry [n][angle][r - 1] has bit c set iff class c is set at step r; entries past ray_len[angle] are
 * written as 0, so the caller need not clear the buffer.  R == 0 (a 1 x 1 frame): the profiles are zero and the map has no entries.
 * octseg_frames_unwrap: the same table as a nearest gather of uint8 frames [N][H][W][channels], channels = 1 or 3, into out uint8
 * [N][360][R][channels], zeros past ray_len[angle]: the polar view of the frame that the label map lines up with.
 * Integer results, no tolerance.  The host mirror (oct_segmentation_amd/polar.py) turns prof into arcs, thicknesses and the cap-over-lipid
 * report.  Enqueue only (one launch each; none for octseg_frames_unwrap with R == 0).  Null pointer (ray_pix may be null only with R == 0),
 * N, H, W, stack_channels <= 0, stack_channels > 8, channels not 1 / 3, R < 0 or H * W >= 2^31: OCTSEG_BAD_ARG.  Nothing is launched and no
 * output is touched then. */
int octseg_stack_polar(const float* stack, int N, int H, int W, int stack_channels, const int* ray_pix, const int* ray_len, int R,
                       int* prof, unsigned char* map /* may be NULL */, void* stream);
int octseg_frames_unwrap(const unsigned char* frames, int N, int H, int W, int channels, const int* ray_pix, const int* ray_len, int R,
                         unsigned char* out, void* stream);

/* Lumen geometry (no reference counterpart; DESIGN.md section 5m, pinned to tests/shape_ref.py).  octseg_stack_measure and octseg_stack_polar
 * walk from the frame centre (W / 2, H / 2); the catheter is rarely at the lumen's centre, and a ray from the frame centre through a lumen does
 * not measure a lumen diameter.  The reference's own thickness is taken from the object's centroid (calculate_thickness_contour,
 * src/app/tools/analysis.py:21-57), but along cv2.findContours' traversal, which nothing here can pin: the three calls below are the nearest
 * independently definable thing -- moments, the centroid as a pixel, and the same five integers per ray from that pixel -- and are NOT that
 * function.  stack: device f32 [N][H][W][channels], any value != 0 is set; a plane is one (slice, channel) pair.
 *
 * octseg_stack_moments: mom int64 [N][channels][OCTSEG_MOMENT_FIELDS], 8-byte aligned, over the set pixels (x, y) of the plane, x the column:
 *    0 M00  sum of 1        3 M20  sum of x * x      6 XMIN  smallest x; W on an empty plane     10 EDGES  the crack perimeter: the number of
 *    1 M10  sum of x        4 M11  sum of x * y      7 XMAX  largest x; -1 on an empty plane               (set pixel, 4-neighbour) pairs whose
 *    2 M01  sum of y        5 M02  sum of y * y      8 YMIN  smallest y; H on an empty plane               neighbour is clear or outside the frame
 *                                                    9 YMAX  largest y; -1 on an empty plane     11        0
 * The call initialises mom on the stream (one launch), then makes one streaming pass over the stack (one launch; float4 loads for 4 channels on
 * a 16-byte aligned base, dword loads otherwise).  Everything is integer, so the result does not depend on the order of the additions and
 * EQUALS the restatement.  Bounds: channels <= 16, H <= OCTSEG_SHAPE_MAX_EXTENT, W <= OCTSEG_SHAPE_MAX_EXTENT, H * W < 2^31: a plane has fewer
 * than 2^31 pixels and each adds less than 2^30 to a second moment, so every field stays below 2^61 and well inside an int64.
 *
 * octseg_moment_origins: origins int32 [N][channels][3] = x, y, AT.  With M = the moments of the plane itself (ref_channel < 0) or of channel
 * ref_channel of the same slice (then every channel of a slice gets the same x, y): x = (2 * M10 + M00) / (2 * M00), y = (2 * M01 + M00) /
 * (2 * M00) in integer arithmetic -- the centroid rounded to the nearest pixel, halves up; AT = 1 iff THIS channel is set at (x, y) (a ring's
 * centroid is not on the ring).  M00 == 0: (-1, -1, 0).  mom is what octseg_stack_moments wrote for the same stack.  One launch of one thread
 * per plane, no host synchronisation; ref_channel >= channels is refused.
 *
 * octseg_stack_polar_at: prof int32 [N][channels][360][5] = IN, OUT, LAST, HITS, RUNS exactly as octseg_stack_polar defines them, and
 * len int32 [N][channels][360], over the steps r = 1 .. len of
 *   pixel(r) = (origins[n][c][0] + ray_off[angle][r - 1][0], origins[n][c][1] + ray_off[angle][r - 1][1])      (x, y; origins' third entry is not read)
 *   ray_off: device int32 [360][R][2], made by the host as (floor(r * cos(radians(angle)) + 0.5), floor(r * sin(radians(angle)) + 0.5)) in
 *            CPython's double arithmetic for r = 1 .. R: the NEAREST pixel.  The reference's int(cx + r * cos) truncates the sum, so its step
 *            pattern depends on the centre it is added to and cannot be a table of offsets; this is a stated deviation.  May be null when R == 0.
 * A ray ends at its first step outside the frame (or after R steps): len is the number of steps inside, and OUT == len means the frame (or the
 * table) cut the first run.  An origin outside [0, W) x [0, H) -- the (-1, -1) of an empty plane -- gives a zero profile and len 0.  The device
 * does no trigonometry, adds in 64 bits and gathers only pixels inside the frame: a wrong table gives wrong samples, never a stray read.
 * channels <= 8, as octseg_stack_polar.  Where all channels of a slice share an origin one gather serves them all.  One launch.
 *
 * Integer results, no tolerance.  The host mirror (oct_segmentation_amd/shape.py) makes the table and turns the integers into the shape table and
 * the lumen report.  Enqueue only.  Null pointer (ray_off may be null only with R == 0), N, H, W, channels <= 0, channels > 16 (8 for
 * octseg_stack_polar_at), H or W > OCTSEG_SHAPE_MAX_EXTENT, H * W >= 2^31, mom not 8-byte aligned, ref_channel >= channels, R < 0:
 * OCTSEG_BAD_ARG.  Nothing is launched and no output is touched then. */
#define OCTSEG_MOMENT_FIELDS 12
#define OCTSEG_SHAPE_MAX_EXTENT 32768
int octseg_stack_moments(const float* stack, int N, int H, int W, int channels, long long* mom, void* stream);
int octseg_moment_origins(const float* stack, const long long* mom, int N, int H, int W, int channels, int ref_channel /* < 0: own */,
                          int* origins, void* stream);
int octseg_stack_polar_at(const float* stack, int N, int H, int W, int channels, const int* origins, const int* ray_off, int R, int* prof,
                          int* len, void* stream);

/* Mask clean-up (reference src/data/mask_processor.py:5-37: MaskProcessor.smooth_mask and .remove_artifacts, run by process_pair,
 * src/data/convert_int_to_cv.py:191-199), on connected components by pixel count (DESIGN.md section 5g states how that differs from
 * cv2.contourArea over RETR_TREE contours).  stack: device f32 [N][H][W][channels], any value != 0 is set; a plane is one (slice, channel) pair.
 * scratch: device, scratch_bytes >= octseg_components_scratch_bytes(N * channels, H, W) (0 for extents the calls refuse), 8-byte aligned.
 *
 * octseg_stack_components: the 8-connected foreground components of every plane.  Optional outputs (null = skipped, at least one):
 *   labels int32 [N][channels][H][W]: 1 + y * W + x of the component's first pixel in raster order, background 0;
 *   ncomp  int32 [N][channels]: the number of components;
 *   top    int32 [N][channels][8][6]: the 8 largest, area descending then first pixel ascending; columns area, first_pixel (y * W + x), x0, y0,
 *          x1, y1 (inclusive bounding box); rows beyond ncomp are zero.
 *
 * octseg_stack_cleanup: out f32 [N][H][W][channels] (0.0 / 1.0, must not alias stack) =
 *   smooth_k >= 2: smooth_mask's chain erode, dilate, dilate, erode, dilate with cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), anchor k / 2,
 *     the element not reflected, outside the frame not taking part (smooth_k 0 or 1: skipped; the reference's k = max(int(0.005 * min(H, W)), 1));
 *   keep > 0: t = the keep-th largest area of the plane (0 with fewer components); components with area >= t stay, ties at t all stay (the
 *     reference's `area in sorted_areas`); min_area additionally drops components with area < min_area; keep = 0: no rank filter;
 *   fill_holes != 0: every background pixel of the kept mask that is not 4-connected to the frame border through background is set
 *     (scipy.ndimage.binary_fill_holes; what drawContours(FILLED) of outer contours does).
 * ncomp / top (optional) describe the kept components after the filter and before the fill, in the layout above.
 * Enqueue only, nothing is allocated.  Null stack / scratch / out, no output requested, scratch too small or misaligned, negative keep / min_area, out ==
 * stack: OCTSEG_BAD_ARG; N, H, W <= 0, channels outside 1..16, H * W >= 2^31 - 1, smooth_k outside 0..7: OCTSEG_BAD_SHAPE.  Nothing is launched then. */
size_t octseg_components_scratch_bytes(int planes, int H, int W);
int octseg_stack_components(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, int* labels, int* ncomp,
                            int* top, void* stream);
int octseg_stack_cleanup(const float* stack, int N, int H, int W, int channels, int smooth_k, int keep, int min_area, int fill_holes, void* scratch,
                         size_t scratch_bytes, float* out, int* ncomp, int* top, void* stream);

/* Mask outlines (no reference counterpart: the reference draws skimage.measure.find_contours and ranks cv2.findContours, neither of which can
 * be pinned here; what is restated are the definitions of DESIGN.md section 5n, pinned to scipy.ndimage.label and matplotlib.path by
 * tests/contours_ref.py).  stack: device f32 [N][H][W][channels], any value != 0 is set, outside the frame is clear; a plane is one (slice,
 * channel) pair.  Pixel (y, x) covers the square [x, x + 1] x [y, y + 1]; VERTICES are the lattice points (x, y), 0 <= x <= W, 0 <= y <= H.
 *
 * CRACK EDGES.  A set pixel (y, x) has a directed edge on each side whose neighbour is clear:
 *   top    (y-1, x) clear: (x, y)     -> (x+1, y)    E = 0        bottom (y+1, x) clear: (x+1, y+1) -> (x, y+1)  W = 2
 *   right  (y, x+1) clear: (x+1, y)   -> (x+1, y+1)  S = 1        left   (y, x-1) clear: (x, y+1)   -> (x, y)    N = 3
 * so the set pixel is on the edge's right.  The id of an edge is ((y_s * (W + 1) + x_s) * 4 + dir) of its start vertex, unique in a plane.
 * The SUCCESSOR of an edge is the edge that starts where it ends; at a vertex where two diagonal pixels are set and the other two clear there are
 * two, and the successor is the one of the OTHER pixel: a turn from dir to (dir + 3) % 4.  The foreground is therefore 8-connected and the
 * background 4-connected, as octseg_stack_components and the hole fill have it.  The edges of a plane fall into disjoint cycles: the CONTOURS.
 * The LEADER of a contour is its edge with the smallest id: the E edge on top of the component's first pixel in raster order for an outer
 * contour, an S edge for a hole.  The VERTEX LIST holds the start vertices of the edges whose predecessor has another direction, in cycle order
 * from the leader's start vertex, closed implicitly; its length is even and at least 4.  Contours are ordered by plane (n * channels + c), then by
 * leader id.  Not OpenCV's border following: those vertices are pixel centres in an order nothing here can pin.
 *
 * octseg_stack_contour_counts: counts int64 [N][channels][2], 8-byte aligned = the crack edges of the plane (field EDGES of octseg_stack_moments)
 *   and the sum of its contours' vertex counts.  One memset and one pass over the stack; no scratch.
 * octseg_stack_contours: traces every plane.
 *   ncont    int32 [N][channels]: the contours of the plane;
 *   table    int32 [contour_capacity][OCTSEG_CONTOUR_FIELDS], one row per contour of the call, rows beyond the total left alone:
 *     0 plane (n * channels + c)    3 area   1/2 sum (x_i * y_i+1 - x_i+1 * y_i) over the vertex list, in pixels: > 0 for an outer contour (the
 *     1 first vertex (row of           component's pixels with its holes filled), < 0 for a hole (minus its pixels); a plane's areas sum to its set pixels
 *       `vertices`)                 4 edges  the cycle length = the crack perimeter      5..8 x0, y0, x1, y1  the vertex-lattice bounds
 *     2 vertex count                9 label  1 + y * W + x of the first pixel in raster order of the 8-connected component that owns the set pixel
 *                                            beside the leader: the contour's own component; for a hole, the component that encloses it
 *   vertices int32 [vertex_capacity][2] = x, y, contour after contour.
 *   overflow int32, cleared by the caller: set to 1 when the call has more edges than edge_capacity (then nothing is traced and ncont is zero),
 *     more contours than contour_capacity or more vertices than vertex_capacity (then the rows and vertices that fit are complete and the others
 *     are not stored): never a store past a buffer.  A call has at most edges / 4 contours and, by octseg_stack_contour_counts, known totals.
 *   scratch: device, 8-byte aligned, scratch_bytes >= octseg_contours_scratch_bytes(N * channels, H, W, edge_capacity) (0 for what the call refuses).
 * Everything is integer and every output is a function of the stack alone: two runs are bit-equal, and results EQUAL the restatement's.
 * Enqueue only, nothing is allocated, the stack is not modified.  Null pointer, scratch too small or misaligned, counts not 8-byte aligned, a
 * capacity <= 0 or >= 2^31: OCTSEG_BAD_ARG; N, H, W <= 0, channels outside 1..16, H * W >= 2^31 - 1, (H + 1) * (W + 1) >=
 * OCTSEG_CONTOUR_MAX_VERTICES (an edge id fits 31 bits), N * channels * (H + 1) * (W / 64 + 1) >= 2^31: OCTSEG_BAD_SHAPE.  Every refusal happens
 * before any HIP call: nothing is launched and no output is touched then. */
#define OCTSEG_CONTOUR_FIELDS 10
#define OCTSEG_CONTOUR_MAX_VERTICES (1 << 29)
int octseg_stack_contour_counts(const float* stack, int N, int H, int W, int channels, long long* counts, void* stream);
size_t octseg_contours_scratch_bytes(int planes, int H, int W, long long edge_capacity);
int octseg_stack_contours(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, long long edge_capacity,
                          long long contour_capacity, long long vertex_capacity, int* ncont, int* table, int* vertices, int* overflow,
                          void* stream);

/* Lesions in 3-D (no reference counterpart: the app's get_analysis groups slices by class presence only; DESIGN.md section 5j, pinned to
 * scipy.ndimage.label with an explicit 3 x 3 x 3 structure by tests/lesions_ref.py).  stack: device f32 [N][H][W][channels], any value != 0 is set.  A
 * VOLUME is one channel of the stack, slices along N in the order given; channels are independent.  Inside a slice voxels are 8-connected.  across:
 *   OCTSEG_ACROSS_OVERLAP  between adjacent slices only the same pixel connects (scipy structure S: S[1] = 1, S[0][1][1] = S[2][1][1] = 1, else 0);
 *   OCTSEG_ACROSS_FULL     the full 3 x 3 x 3 structure (26-connected).
 * The label of a lesion is 1 + n * H * W + y * W + x of its first voxel in raster order; background is 0.
 * scratch: device, scratch_bytes >= octseg_lesions_scratch_bytes(channels, N, H, W) (0 for extents the calls refuse), 8-byte aligned.
 *
 * octseg_volume_components: optional outputs (null = skipped, at least one):
 *   labels  int32 [channels][N][H][W];
 *   nles    int32 [channels]: the number of lesions;
 *   top     int32 [channels][32][8]: the 32 largest, voxels descending then first voxel ascending; columns voxels, first_voxel (n * H * W + y * W + x),
 *           z0, z1, y0, y1, x0, x1 (inclusive bounds; z0 = first_voxel / (H * W)); rows beyond nles are zero;
 *   profile int32 [channels][32][N]: the set pixels of ranked lesion r in slice n, zero outside z0..z1 and for rows beyond nles.
 *
 * octseg_volume_cleanup: out f32 [N][H][W][channels] (0.0 / 1.0, must not alias stack) = the lesions for which all three hold:
 *   voxels >= t, t = the keep-th largest voxel count of the channel (0 with fewer lesions; ties at t all stay; keep = 0: no rank filter);
 *   voxels >= min_voxels;
 *   z1 - z0 + 1 >= min_slices (min_slices = 2 removes what shows in one slice only: the flicker filter).
 * nles / top (optional) describe the kept lesions, in the layout above.
 * Enqueue only, nothing is allocated, the stack is not modified.  Null stack / scratch / out, scratch too small or misaligned, no output requested,
 * out == stack, negative keep / min_voxels, min_slices < 1, unknown across: OCTSEG_BAD_ARG; N, H, W <= 0, channels outside 1..16,
 * N * H * W >= 2^31 - 1: OCTSEG_BAD_SHAPE.  Every refusal happens before any HIP call: nothing is launched and no output is touched then. */
#define OCTSEG_ACROSS_OVERLAP 0
#define OCTSEG_ACROSS_FULL 1
size_t octseg_lesions_scratch_bytes(int channels, int N, int H, int W);
int octseg_volume_components(const float* stack, int N, int H, int W, int channels, int across, void* scratch, size_t scratch_bytes, int* labels,
                             int* nles, int* top, int* profile, void* stream);
int octseg_volume_cleanup(const float* stack, int N, int H, int W, int channels, int across, int keep, int min_voxels, int min_slices, void* scratch,
                          size_t scratch_bytes, float* out, int* nles, int* top, void* stream);

/* Predicted against annotated lesions (no reference counterpart: the reference scores pixel overlap only; DESIGN.md section 5o, pinned to
 * tests/match_ref.py, which is proved against sklearn's contingency_matrix).  pred, truth: device f32 [N][H][W][channels] with the same extents, any
 * value != 0 is set; they may be the same buffer and neither is modified.  Channels are independent.  For a channel and a SIDE (0 = pred, 1 = truth)
 * the lesions, their labels and their ranked list are exactly those of octseg_volume_components above with the same `across`: the 32 largest by
 * voxels descending, then first voxel ascending.  The RANK of a set voxel is 0..31 if its lesion is ranked and 32 ("rest") if its lesion is beyond
 * the 32 listed; a clear voxel has no rank.
 *   nles    int32 [channels][2]: the number of lesions per side;
 *   top     int32 [channels][2][32][8] (optional): the rows of octseg_volume_components' top for each side, bounding boxes included;
 *   overlap int32 [channels][33][33]: overlap[i][j] = the voxels whose pred rank is i and whose truth rank is j.  The table sums to |P & T| of the
 *           channel; row i < 32 sums to at most top[c][0][i][0], the remainder of the lesion lies over truth background (columns alike);
 *   frames  int32 [channels][N][3] (optional): |P & T|, |P|, |T| set pixels of slice n.
 * Everything is integer and a function of the two stacks alone: two runs are bit-equal, results EQUAL the restatement's, no tolerance.  overlap and
 * frames are cleared inside the call.
 * scratch: device, 8-byte aligned, scratch_bytes >= octseg_match_scratch_bytes(channels, N, H, W) (0 for extents the call refuses), which is, with
 * V = channels * N * H * W, al(v) = v rounded up to 256 and W64 = ceil(W / 64):
 *   4 * al(4 * V)                                             parent of either side; voxel counts and last slices, used by one side after the other
 *   + al(4 * channels * N * ceil(H / 2) * ceil(W / 2))        the lesion list, likewise shared
 *   + 2 * al(4 * channels)                                    the lesion counter and the threshold
 *   + 2 * al(4 * channels * 32)                               the ranked roots of either side
 *   + al(4 * channels * 2) + al(4 * channels * 2 * 32 * 8)    nles and top side by side, before they are interleaved
 *   + 2 * al(8 * channels * N * H * W64)                      the bit planes of either side
 * (about 17.3 bytes per voxel and channel, against 2 x 13.3 for two octseg_volume_components calls' worth).
 * Enqueue only, nothing is allocated.  Null pred / truth / scratch / nles / overlap, scratch too small or not 8-byte aligned, unknown across:
 * OCTSEG_BAD_ARG; N, H, W <= 0, channels outside 1..16, N * H * W >= 2^31 - 1: OCTSEG_BAD_SHAPE.  Every refusal happens before any HIP call:
 * nothing is launched, no output is touched, and octseg_last_error names the argument. */
size_t octseg_match_scratch_bytes(int channels, int N, int H, int W);
int octseg_volume_match(const float* pred, const float* truth, int N, int H, int W, int channels, int across, void* scratch, size_t scratch_bytes,
                        int* nles, int* top, int* overlap, int* frames, void* stream);

/* Boundary distances (no reference counterpart: the reference scores overlap only; what is restated here are the definitions of DESIGN.md
 * section 5i, pinned to scipy.ndimage by tests/distance_ref.py).  stack / src / dst: device f32 [N][H][W][channels], any value != 0 is set; a plane
 * is one (slice, channel) pair.  A PART of a plane is 0 the set pixels, 1 the clear pixels inside the frame, or 2 the boundary
 *   b = m & ~erode(m) with the 4-neighbour cross, the outside of the frame counting as clear, so that a set pixel on the frame edge is boundary
 *   (scipy: m & ~binary_erosion(m, generate_binary_structure(2, 1), border_value=0)).
 * The squared distance of pixel (y, x) to a target part T is d2 = min over (y', x') in T of (y - y')^2 + (x - x')^2, pixel centre to pixel centre,
 * exact in int32 (scipy: rint(distance_transform_edt(~T)^2)); 0 on T itself; OCTSEG_DIST_NONE when T is empty.  Integer arithmetic only: results
 * EQUAL the restatement's, no tolerance.
 * scratch: device, 8-byte aligned, scratch_bytes >= octseg_distance_scratch_bytes(N, H, W, channels_a, channels_b, pairs) (one-stack calls:
 * channels_a = channels, channels_b = 0, pairs = 0; 0 is returned for extents the calls refuse).
 *
 * octseg_stack_boundary: out f32 [N][H][W][channels] (0.0 / 1.0, must not alias stack) = the boundary of every plane.
 * octseg_stack_distance: d2 int32 [N][channels][H][W] = the squared distance of every pixel to part `to` of its own plane.
 * The pair calls take a device list pairs int32 [npairs][2] = (channel of src, channel of dst); for every slice n and pair p, segment
 * s = n * npairs + p, the QUERY pixels are part src_part of src's plane and the TARGET is part dst_part of dst's plane (src and dst may be the same
 * stack).  Channel numbers outside their stack are clamped on the device.
 * octseg_pair_distance_counts: counts int32 [N][npairs][2] = query pixels, target pixels; overlap (may be NULL) int32 [N][npairs][3] =
 *   |a & b|, |a|, |b| of the two planes' SET pixels whatever the parts, so that Dice and IoU come from the same call.
 * octseg_pair_distance_keys: for every query pixel of segment s one int64 key = (first_segment + s) << 32 | d2 is stored into
 *   keys[offsets[s] + slot], offsets device int64 [N * npairs] (the caller's running sum of the query counts), the slots of a segment handed out
 *   by an integer atomic in no fixed order: sort the keys.  A position outside 0 .. capacity - 1 is NOT stored and sets *overflow (device int32,
 *   cleared by the caller) to 1: never a store past the buffer.
 * octseg_pair_distance_min: out uint64 [N][npairs] = the minimum over the segment's query pixels of d2 << 32 | (y * W + x): the smallest squared
 *   distance and, among the pixels that attain it, the first in raster order; all ones for a segment without query pixels.
 * Enqueue only, nothing is allocated.  Null pointer (overlap excepted), scratch too small or misaligned, a part outside 0..2, capacity <= 0, out ==
 * stack: OCTSEG_BAD_ARG; N, H, W <= 0, H or W above 4096 (so that d2 < 2^25 and a column distance fits 16 bits), channels outside 1..16, npairs <= 0,
 * segment numbers reaching 2^31: OCTSEG_BAD_SHAPE.  Nothing is launched then. */
#define OCTSEG_DIST_NONE 0x7fffffff
size_t octseg_distance_scratch_bytes(int N, int H, int W, int channels_a, int channels_b, int pairs);
int octseg_stack_boundary(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, float* out, void* stream);
int octseg_stack_distance(const float* stack, int N, int H, int W, int channels, int to, void* scratch, size_t scratch_bytes, int* d2, void* stream);
int octseg_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                                int src_part, int dst_part, void* scratch, size_t scratch_bytes, int* counts, int* overlap /* may be NULL */,
                                void* stream);
int octseg_pair_distance_keys(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                              int src_part, int dst_part, void* scratch, size_t scratch_bytes, long long first_segment, const long long* offsets,
                              long long* keys, long long capacity, int* overflow, void* stream);
int octseg_pair_distance_min(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                             int src_part, int dst_part, void* scratch, size_t scratch_bytes, unsigned long long* out, void* stream);

/* Surface distances of the VOLUME (no reference counterpart; DESIGN.md section 5p, pinned to scipy.ndimage by tests/distance3d_ref.py).  The stack
 * f32 [N][H][W][channels], any value != 0 set, is read per channel as a volume of N slices; voxel (z, y, x) is pixel (y, x) of slice z.
 * slice_step: an integer s >= 1, the distance between neighbouring slices in pixels.  The squared distance between two voxels is
 *   (s dz)^2 + dy^2 + dx^2, voxel centre to voxel centre, in int32; only integers are accepted, rational spacing is out of scope.
 * The 3-D BOUNDARY is b = m & ~erode(m) with the 6-neighbour cross, everything outside the volume clear
 *   (scipy: m & ~binary_erosion(m, generate_binary_structure(3, 1), border_value=0)): every set voxel of the first and of the last slice is boundary,
 *   and with N <= 2 every set voxel is.  There is no "open ends" variant.
 * A PART is 0 the set voxels, 1 the clear voxels inside the volume, or 2 the 3-D boundary.  The TARGET of a distance is the part taken over the
 * whole volume of one channel: d2(z, y, x) = min over the target's voxels (scipy: rint(distance_transform_edt(~T, sampling=(s, 1, 1))^2)), 0 on the
 * target, OCTSEG_DIST_NONE everywhere when the part is empty in the whole volume -- that is not decided per slice.  Integer arithmetic only: results
 * EQUAL the restatement's, no tolerance.
 * scratch: device, 8-byte aligned.  octseg_volume_distance_scratch_bytes(N, H, W, channels_a, channels_b, pairs, rows) = the bytes a call needs that
 * maps the volume in BANDS of `rows` rows of all slices (1 <= rows <= H; rows = 0: octseg_volume_boundary and the counts, which take no distance);
 * one-stack calls: channels_b = 0, pairs = 0; 0 is returned for arguments the calls refuse.  The bit planes of the whole volume (1/8 byte per voxel
 * and plane, four sets at most) plus 6 bytes per voxel of the band and target channel.  octseg_volume_distance and the keys / min calls take the most
 * rows that fit scratch_bytes and work band after band; the result does not depend on the banding.  A scratch below the one-row need is refused with
 * the bytes needed in octseg_last_error.
 *
 * octseg_volume_boundary: out f32 [N][H][W][channels] (0.0 / 1.0, must not alias stack) = the 3-D boundary.
 * octseg_volume_distance: d2 int32 [N][channels][H][W] = the squared distance of every voxel to part `to` of its own channel's volume.
 * The pair calls take pairs int32 [npairs][2] = (channel of src, channel of dst) as octseg_pair_distance_* do, clamped on the device; a SEGMENT is a
 * pair p, not a (slice, pair): the QUERY voxels are part src_part of src's channel over all slices, the TARGET part dst_part of dst's channel.
 * octseg_volume_pair_distance_counts: counts int64 [npairs][2] = query voxels, target voxels; overlap (may be NULL) int64 [npairs][3] =
 *   |a & b|, |a|, |b| of the two channels' SET voxels whatever the parts.
 * octseg_volume_pair_distance_keys: one int64 key = (first_segment + p) << 32 | d2 per query voxel at keys[offsets[p] + slot], offsets device int64
 *   [npairs], slots in no fixed order: sort the keys.  A position outside 0 .. capacity - 1 is NOT stored and sets *overflow (device int32, cleared
 *   by the caller) to 1: never a store past the buffer.
 * octseg_volume_pair_distance_min: out uint64 [npairs] = the minimum over the pair's query voxels of d2 << 32 | (z * H * W + y * W + x): the
 *   smallest squared distance and, among the voxels that attain it, the first in raster order; all ones without a query voxel.
 * Enqueue only, nothing is allocated.  Null pointer (overlap excepted), scratch too small or misaligned, a part outside 0..2, capacity <= 0, out ==
 * stack, slice_step < 1 or slice_step * (N - 1) > 32767 (so that d2 < 2^30 + 2^25 stays below OCTSEG_DIST_NONE), N * H * W > 2^32 (the packed
 * minimum's voxel index): OCTSEG_BAD_ARG; N, H, W <= 0, H or W above 4096, channels outside 1..16, npairs <= 0, N * npairs or a segment number
 * reaching 2^31: OCTSEG_BAD_SHAPE.  Nothing is launched then. */
size_t octseg_volume_distance_scratch_bytes(int N, int H, int W, int channels_a, int channels_b, int pairs, int rows);
int octseg_volume_boundary(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, float* out, void* stream);
int octseg_volume_distance(const float* stack, int N, int H, int W, int channels, int to, int slice_step, void* scratch, size_t scratch_bytes, int* d2,
                           void* stream);
int octseg_volume_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs,
                                       int npairs, int src_part, int dst_part, void* scratch, size_t scratch_bytes, long long* counts,
                                       long long* overlap /* may be NULL */, void* stream);
int octseg_volume_pair_distance_keys(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs,
                                     int npairs, int src_part, int dst_part, int slice_step, void* scratch, size_t scratch_bytes,
                                     long long first_segment, const long long* offsets, long long* keys, long long capacity, int* overflow,
                                     void* stream);
int octseg_volume_pair_distance_min(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                                    int src_part, int dst_part, int slice_step, void* scratch, size_t scratch_bytes, unsigned long long* out,
                                    void* stream);

/* Slices interpolated from signed distance maps (no reference counterpart; shape-based interpolation after Raya and Udupa, DESIGN.md section 5s,
 * pinned to scipy.ndimage by tests/interp_ref.py).  A plane is one (slice, channel) pair of the f32 stack [N][H][W][channels], any value != 0 set.
 * The SIGNED SQUARED DISTANCE sd2, int32 in the layout [N][channels][H][W] that octseg_stack_distance writes:
 *   at a set pixel    +d2 to the nearest clear pixel of the plane, so >= 1;
 *   at a clear pixel  -d2 to the nearest set pixel, so <= -1;
 *   on an empty plane -OCTSEG_DIST_NONE everywhere, on a full plane +OCTSEG_DIST_NONE everywhere; never 0
 *   (= where(m, stack_distance(to = clear), -stack_distance(to = set))).
 * The BLEND of planes a and b with integer weights 0 <= wa, wb <= 32767, not both 0: with s = sign(sd2) * sqrt(|sd2|), +-infinity for
 * OCTSEG_DIST_NONE, a pixel is set iff wa * s_a + wb * s_b > 0.  The decision is made in integers only:
 *   a weight of 0 removes its side and the other side's sign decides;
 *   equal signs: that sign decides;
 *   opposite signs, both finite: set iff wP^2 * |sd2_P| > wQ^2 * |sd2_Q| in int64 (below 2^55), P the positive and Q the negative side;
 *   opposite signs, exactly one infinite: its sign decides;  both infinite: set iff wP > wQ;
 *   a tie is clear.
 * A PLAN is device int32 [M][6], rows (channel, out_slice, lo, hi, w_lo, w_hi): row r writes plane (out_slice, channel) of out f32
 * [N_out][H][W][channels] as 0.0 / 1.0, the blend of planes (lo, channel) and (hi, channel) of sd2 (K slices) with weights w_lo and w_hi.  Planes
 * that no row names are not touched; two rows that name one plane race (the wrappers refuse them).  Every number of a row is clamped on the device
 * into its range: a wrong plan gives a wrong plane, never a stray access.  made (may be NULL) int32 [M] = the set pixels of each written plane.
 * scratch: device, 8-byte aligned, scratch_bytes >= octseg_signed_distance_scratch_bytes(N, H, W, channels) (two sets of bit planes, 4 bytes per
 * pixel and channel, the flags; 0 is returned for extents the calls refuse).
 * Enqueue only, nothing is allocated, nothing synchronises.  Null pointer (made excepted), scratch too small or misaligned, sd2 == stack, out ==
 * sd2: OCTSEG_BAD_ARG; extents <= 0, H or W above 4096, channels outside 1..16, M <= 0: OCTSEG_BAD_SHAPE.  Nothing is launched then.
 * Out of scope: extrapolation, registration between slices (objects that do not overlap vanish), non-integer weights. */
size_t octseg_signed_distance_scratch_bytes(int N, int H, int W, int channels);
int octseg_stack_signed_distance(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, int* sd2, void* stream);
int octseg_signed_blend(const int* sd2, int K, int H, int W, int channels, const int* plan, int M, float* out, int N_out, int* made /* may be NULL */,
                        void* stream);

/* Centrelines by thinning (no reference counterpart: the reference measures thickness along rays only; DESIGN.md section 5q, pinned by
 * tests/skeleton_ref.py).  stack: device f32 [N][H][W][channels], any value != 0 is set; a plane is one (slice, channel) pair and every pixel
 * outside the frame is clear.  Neighbours of pixel (y, x), clockwise from north:
 *   P2 (y-1, x)  P3 (y-1, x+1)  P4 (y, x+1)  P5 (y+1, x+1)  P6 (y+1, x)  P7 (y+1, x-1)  P8 (y, x-1)  P9 (y-1, x-1)
 * The SKELETON of a plane is Guo and Hall's two-sub-iteration parallel thinning (1989, algorithm A1).  With booleans as 0 / 1:
 *   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)
 *   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
 *   m  = sub-iteration 0: (P6 | P7 | !P9) & P8        sub-iteration 1: (P2 | P3 | !P5) & P4
 *   a set pixel is deleted iff  C == 1  and  2 <= min(N1, N2) <= 3  and  m == 0
 * Every deletion of a sub-iteration is decided on the plane as it stood when the sub-iteration began, then applied at once.  A PASS is
 * sub-iteration 0 then sub-iteration 1; thinning ends after the first pass in which neither deletes anything; `passes` is the number of passes that
 * deleted at least one pixel (0 for an empty or already thin plane).  The result is unique: results EQUAL the restatement's.  It keeps the number
 * of 8-connected components and of holes; a 2 x 2 square thins to one pixel.
 * octseg_stack_skeleton: out (may be NULL) f32 [N][H][W][channels], 0.0 / 1.0, must not alias stack = the skeleton of every plane;
 *   census (may be NULL) int32 [N][channels][6] = set pixels, skeleton pixels, END points (skeleton pixels with exactly one of their 8 neighbours on
 *   the skeleton), JUNCTION pixels (three or more), ISOLATED pixels (none), passes.  One workgroup thins one plane in one launch: from LDS when
 *   the plane's H * ceil(W / 64) words fit it (up to 1024 x 1024 and beyond: 20478 words), else, or with flags bit 0 (OCTSEG_SKEL_GLOBAL) at any size,
 *   over images in scratch; both give the same result.  The width of an object at its centreline is not computed here: it is
 *   octseg_pair_distance_keys with src = out, dst = stack, src_part 0, dst_part 1 (the squared distance to the nearest clear pixel inside the frame).
 * scratch: device, 8-byte aligned, scratch_bytes >= octseg_skeleton_scratch_bytes(N, H, W, channels) (three sets of bit planes, 1/8 byte per pixel
 * and plane each; 0 is returned for extents the call refuses).
 * Enqueue only, nothing is allocated.  Null stack or scratch, out and census both NULL, out == stack, scratch too small or misaligned, flag bits
 * other than bit 0: OCTSEG_BAD_ARG; N, H, W <= 0, H or W above 4096, channels outside 1..16, N * channels * 6 reaching 2^31: OCTSEG_BAD_SHAPE.
 * Nothing is launched then. */
#define OCTSEG_SKEL_GLOBAL 1
size_t octseg_skeleton_scratch_bytes(int N, int H, int W, int channels);
int octseg_stack_skeleton(const float* stack, int N, int H, int W, int channels, int flags, void* scratch, size_t scratch_bytes,
                          float* out /* [N][H][W][channels] 0.0 / 1.0, may be NULL */, int* census /* [N][channels][6], may be NULL */, void* stream);

/* Centreline pruning (no reference counterpart; DESIGN.md section 5r, pinned by tests/prune_ref.py).  skel: device f32 [N][H][W][channels], any
 * value != 0 is set; a plane is one (slice, channel) pair, every pixel outside the frame is clear, P2 .. P9 are the neighbours above.  The input is
 * meant to be a skeleton (octseg_stack_skeleton's out); any plane is legal and the rules hold for any plane.  Only integers and booleans appear.
 * A set pixel is a TIP when one of these holds (the eight end-point structuring elements of morphological pruning, Gonzalez and Woods):
 *   orthogonal form, for one of the four orthogonal directions d: the neighbour at d is set and the five neighbours other than d and d's two
 *   adjacent diagonals are all clear --
 *     north  P2 & ~(P4|P5|P6|P7|P8)      east   P4 & ~(P6|P7|P8|P9|P2)      south  P6 & ~(P8|P9|P2|P3|P4)      west   P8 & ~(P2|P3|P4|P5|P6)
 *   diagonal form: no orthogonal neighbour is set and exactly one diagonal neighbour is set.
 * An isolated pixel is not a tip.  A tip is not the census's END point ("exactly one neighbour"): a one-pixel stub standing on a row has three
 * neighbours, is a tip, and is no END.
 *   erode(X, n)    repeats X <- X \ tips(X) n times, all tips of a pass decided on X as the pass found it; it stops early at the first pass
 *                  without a tip
 *   grow(D, n, A)  repeats D <- D | (dil8(D) & A) n times, dil8 the 3 x 3 dilation
 * For a plane A and integers spur >= 0, trim >= 0:
 *   X = erode(A, spur)
 *   Y = X | grow(tips(X), spur, A)        (spur == 0: Y = A)
 *   Z = erode(Y, trim)
 *   R = the union of the 8-connected components of A that meet Z
 *   out = Z | (A & ~R)
 * A side branch of at most spur pixels goes away, longer branches and the main ends are regrown to their full length, trim then takes that many
 * pixels off every end that is left, and a component that this would erase is returned whole and unpruned.  out is a subset of A with the same
 * numbers of 8-connected components and of holes; a ring has no tip and is returned as it is; (0, 0) is the identity.
 * LINKS are counted on out: orth = the pairs of 4-adjacent set pixels; diag = the pairs of diagonally adjacent set pixels whose two common
 * 4-neighbours are both clear (otherwise the two orthogonal links already connect them): w & E, w & S, w & SE & ~E & ~S, w & SW & ~W & ~S.  The
 * length along the centreline is orth + sqrt(2) * diag, computed in float64 on the host.
 * octseg_stack_prune: out (may be NULL) f32 [N][H][W][channels], 0.0 / 1.0, must not alias skel; census (may be NULL) int32 [N][channels][9] =
 *   0 input pixels, 1 output pixels, 2 tips of the output, 3 END points of the output (exactly one of the 8 neighbours set), 4 JUNCTION pixels
 *   (three or more), 5 ISOLATED pixels (none), 6 orth links, 7 diag links, 8 restored pixels |A & ~R|.  One workgroup prunes one plane in one
 *   launch: from LDS when the plane's padded bit image fits it (as for octseg_stack_skeleton), else, or with flags bit 0 (OCTSEG_PRUNE_GLOBAL) at
 *   any size, over images in scratch; both give the same result.
 * scratch: device, 8-byte aligned, scratch_bytes >= octseg_prune_scratch_bytes(N, H, W, channels) (four sets of bit planes, 1/8 byte per pixel
 * and plane each; 0 is returned for extents the call refuses).
 * Enqueue only, nothing is allocated.  Null skel or scratch, out and census both NULL, out == skel, scratch too small or misaligned, flag bits
 * other than bit 0, spur or trim outside 0..8192 (an interface bound that keeps every loop count small): OCTSEG_BAD_ARG; N, H, W <= 0, H or W
 * above 4096, channels outside 1..16, N * channels * 9 reaching 2^31: OCTSEG_BAD_SHAPE.  Nothing is launched then. */
#define OCTSEG_PRUNE_GLOBAL 1
size_t octseg_prune_scratch_bytes(int N, int H, int W, int channels);
int octseg_stack_prune(const float* skel, int N, int H, int W, int channels, int spur, int trim, int flags, void* scratch, size_t scratch_bytes,
                       float* out /* [N][H][W][channels] 0.0 / 1.0, may be NULL */, int* census /* [N][channels][9], may be NULL */, void* stream);

/* The arithmetic between a DICOM's pixel_array and the frames the pipeline takes (reference src/data/convert_dicoms.py:71-81, repeated in
 * src/app/tools/analysis.py:167-177): per slice cv2.normalize(img, None, alpha=0, beta=255, norm_type=NORM_MINMAX, dtype=CV_8U), then
 * cvtColor(BGR2RGB).  src: device [S][H][W][C], uint8 (src_dtype 0) or uint16 (src_dtype 1, 2-byte aligned), C = 1 or 3.
 * minmax: device uint32 [S][2], scratch AND output: the call sets it to (0xffffffff, 0), then holds the minimum and maximum of every slice over
 * ALL its channels (minMaxIdx on a multi-channel Mat without an index request).  dst: uint8 [S][H][W][3], must not overlap src.  The
 * pair is read back on the device, no host synchronisation.  Per slice, in double:
 *   scale = 255 * (smax - smin > DBL_EPSILON ? 1 / (smax - smin) : 0),  shift = 0 - smin * scale,  a = (float)scale,  b = (float)shift;
 * per sample dst = saturate_cast<uchar>(rint(x * a + b)), the product and the sum EACH rounded to float32 (OpenCV 4.8.1's baseline convertTo;
 * its AVX2 build fuses them and can differ by one grey level on a rounding tie -- this form is the one fixed here), rint half to even.
 * A constant slice comes out 0, a slice spanning 0..255 unchanged.  swap_rb != 0 reverses the three channels; C = 1 is written to three equal
 * channels.  Parity with cv2 itself is not pinned (cv2 is not installed where this project runs); the tests hold the kernel to a numpy
 * restatement of the lines above, exactly.
 * Enqueue only (three launches).  Null pointer: OCTSEG_BAD_ARG; src_dtype not 0 / 1: OCTSEG_BAD_DTYPE; S, H, W <= 0, C not 1 / 3, or a source or
 * destination frame of 2^31 bytes or more: OCTSEG_BAD_SHAPE.  Nothing is launched then. */
int octseg_volume_normalize(const void* src, int src_dtype, int S, int H, int W, int C, int swap_rb, unsigned* minmax, uint8_t* dst, void* stream);

/* Image.resize((ow, oh)) of Pillow for 8-bit frames with its default filter, BICUBIC (reference src/data/utils.py:187: data_processing), for a
 * batch: ImagingResample's two passes (Resample.c), horizontal first, from host tables (oct_segmentation_amd/pullback.py pil_resample_table =
 * precompute_coeffs + normalize_coeffs_8bpc).  src: uint8 [S][H][W][C], C = 1 (mode L) or 3 (RGB); dst: uint8 [S][oh][ow][C]; tmp: uint8
 * [S][H][ow][C], read and written only when both axes change (may be null otherwise).  Per axis: bounds device int32 [out][2] = first source
 * index and tap count of every output index, kk device int32 [out][ksize] = the taps' coefficients at 22 fractional bits.  Per output sample
 *   ss = (1 << 21) + sum over t < count of src[first + t] * kk[t]  in 32-bit arithmetic,  out = clamp(ss >> 22, 0, 255), arithmetic shift
 * (bicubic taps overshoot: the clamp is live).  An axis whose output length equals its input length is skipped and its tables may be null, as
 * Pillow skips it; with both skipped dst is a copy of src.  Bounds outside the source and counts beyond ksize or the source's end are clamped
 * on the device: a wrong table gives wrong samples, never a stray read.  Integer arithmetic: the result EQUALS Pillow's, no tolerance.
 * Enqueue only (a launch per resampled axis).  Null src / dst, null tmp when both axes change, null tables of a resampled axis: OCTSEG_BAD_ARG;
 * S, H, W, oh, ow <= 0, C not 1 / 3, ksize <= 0 for a resampled axis, or a source, intermediate or destination frame of 2^31 bytes or more:
 * OCTSEG_BAD_SHAPE.  Nothing is launched then. */
int octseg_resize_pil_u8(const uint8_t* src, int S, int H, int W, int C, uint8_t* tmp, uint8_t* dst, int oh, int ow, const int* xbounds,
                         const int* xkk, int xksize, const int* ybounds, const int* ykk, int yksize, void* stream);

/* Class activation maps (reference src/models/cam_processor.py:83-98 and src/models/visualize_activation_maps.py:102-199 over the
 * pytorch-grad-cam package; restated in DESIGN.md section 5e, parity with the package itself is not pinned).
 *
 * octseg_plan_set_frozen_bn(plan, 1): the reference explains a model in eval().  Training-path forwards of the plan (octseg_net_forward with
 * train = 1) then keep activations and ReLU masks as in training but read every BatchNorm from its running statistics: no buffer is written, a
 * batch of one value per channel is accepted.  Built for unet | unetplusplus | linknet | manet over the ResNets in f32 / bf16; every other
 * pair returns OCTSEG_UNSUPPORTED_ARCH (f16: OCTSEG_BAD_DTYPE) and octseg_last_error() says why.  Use a plan of its own for this.
 * octseg_plan_cam_target: workspace byte offsets of the output of encoder.layer4's last block (the reference's target layer, after the residual
 * add and the ReLU) and of its gradient, NHWC in the plan dtype; dims = {N, h, w, K}.
 * octseg_net_backward_seeded: backward of such a forward from dL/dlogits (device NCHW f32 [batch][classes][H][W], e.g. a mask on one class
 * plane: the reference's SemanticSegmentationTarget) down to the target tensor's gradient.  Data gradients only: no weight, bias or BatchNorm
 * parameter gradient is launched, no gradient arena is read or written.
 *
 * octseg_cam_maps: A, G device NHWC [N][h][w][K] of `dtype` (f32 | bf16; K a multiple of 8) -> maps f32 [N][S][S].  method: 0 GradCAM,
 * 1 HiResCAM, 2 GradCAMElementWise, 3 GradCAMPlusPlus, 4 XGradCAM, 5 LayerCAM.  Per frame: the method's raw map, max(., 0), (x - min) / (1e-7 +
 * max), cv2.resize(INTER_LINEAR) to S x S in float32, max(., 0), the same scaling again.  scratch: octseg_cam_scratch_bytes(N, h, w, K) device bytes.
 * Optional outputs (null = skipped), all enqueued behind the maps on the same stream:
 *   bin      uint8 [N][S][S] = (map > threshold) * 255;
 *   counts   int32 [N][3] = tp, pred, true of (map > threshold) read through row_index [gt_h] / col_index [gt_w] (device int32, the source index
 *            of every ground-truth row / column: cv2's INTER_NEAREST rule, as for octseg_ingest_mask; clamped on the device) against
 *            gt uint8 [N][gt_h][gt_w], any value != 0 counting as set;
 *   overlay  uint8 [N][S][S][3] BGR = show_cam_on_image(frame / 255, map, use_rgb=False, image_weight): frames f32 [N][3][S][S] BGR planes
 *            0..255, jet_bgr device uint8 [256][3] the colour table in BGR (the host mirror builds it, oct_segmentation_amd/cam.py),
 *            o = (1 - image_weight) * jet[uint8(255 * map)] / 255 + image_weight * frame / 255, divided by its maximum over the frame,
 *            times 255, truncated.
 * Enqueue only.  Null A / G / scratch / maps or a requested output without its inputs: OCTSEG_BAD_ARG; bad extents: OCTSEG_BAD_SHAPE. */
int octseg_plan_set_frozen_bn(octseg_plan* plan, int on);
int octseg_plan_cam_target(const octseg_plan* plan, size_t* act_off, size_t* grad_off, int* dims);
int octseg_net_backward_seeded(octseg_plan* plan, const float* params, void* workspace, const float* dlogits, void* stream);
size_t octseg_cam_scratch_bytes(int N, int h, int w, int K);
int octseg_cam_maps(int dtype, const void* A, const void* G, int N, int h, int w, int K, int method, int S, void* scratch, float* maps,
                    float threshold, uint8_t* bin, const uint8_t* gt, int gt_h, int gt_w, const int* row_index, const int* col_index, int* counts,
                    const float* frames, const uint8_t* jet_bgr, double image_weight, uint8_t* overlay, void* stream);

/* octseg_cam_overlay: the overlay of octseg_cam_maps for maps that exist already (f32 [N][S][S], used as they are); scratch: 16 * N device bytes. */
int octseg_cam_overlay(const float* maps, const float* frames, const uint8_t* jet_bgr, int N, int S, double image_weight, uint8_t* overlay,
                       void* scratch, void* stream);

/* Criterion evaluated by octseg_dice_forward / octseg_net_train_step and differentiated by the backward entry points.
 * OCTSEG_LOSS_DICE (default) = smp.losses.DiceLoss(MULTILABEL_MODE, from_logits=True), the reference's (model.py:55);
 * OCTSEG_LOSS_BCE = torch.nn.functional.binary_cross_entropy_with_logits(logits, target) (reduction 'mean' over every element);
 * OCTSEG_LOSS_DICE_BCE = their unweighted sum.  All three come out of the ONE pass over logits / target that also counts tp/fp/fn/tn. */
typedef enum { OCTSEG_LOSS_DICE = 0, OCTSEG_LOSS_BCE = 1, OCTSEG_LOSS_DICE_BCE = 2 } octseg_loss_kind;
int octseg_plan_set_loss(octseg_plan* plan, int kind);

/* loss: device f32 scalar; stats: device int64 [B][classes][4] = tp, fp, fn, tn (nullable). */
int octseg_dice_forward(octseg_plan* plan, void* workspace, const float* logits, const float* target,
                        float* loss, long long* stats, void* stream);

/* Must follow octseg_net_forward(train=1) + octseg_dice_forward on the same workspace.
 * grads (fp32 arena, same layout as params) is overwritten with d(grad_scale * loss)/dparams. */
int octseg_net_backward(octseg_plan* plan, const float* params, float* grads, void* workspace,
                        const float* logits, const float* target, float grad_scale, void* stream);

/* Forward (train) + Dice + backward in ONE call (reference: training_step + loss.backward(), src/models/smp/model.py:73-95 under Lightning).
 * Same launches as octseg_net_forward(train = 1) -> octseg_dice_forward -> octseg_net_backward.  octseg_plan_set_train_graph(plan, 1):
 * the call is captured into a hipGraph on its second use with an unchanged argument set (every pointer, the stream, the constants) and
 * replayed afterwards -- one launch per step instead of ~800 (keep image / target / logits / loss / stats in persistent buffers).
 * Not available together with the sliced (data-parallel) backward. */
int octseg_net_train_step(octseg_plan* plan, const float* params, float* grads, float* buffers, void* workspace, const float* image,
                          const float* target, float* logits, float* loss, long long* stats, int normalize, const float* mean,
                          const float* stdv, float grad_scale, void* stream);
int octseg_plan_set_train_graph(octseg_plan* plan, int enable);

/* Data-parallel variant (reference: torch DDP's bucketed gradient all-reduce overlapped with backward, which Lightning installs for
 * src/models/smp/train.py:122-133 when more than one GPU is visible).  Same launches; the gradient arena is cut into
 * `nslices` contiguous parameter-aligned ranges and cb(user, k, begin, end) -- element offsets into grads -- is called on the
 * calling host thread as soon as the last launch writing into slice k is enqueued; comm_stream (not the compute stream) has by
 * then been made to wait for those launches, so the collective the callback enqueues there overlaps the rest of the backward.
 * Slices are reported exactly once each, in completion order (decoder / head ranges first). */
typedef void (*octseg_slice_cb)(void* user, int slice, size_t begin, size_t end);
int octseg_net_backward_sliced(octseg_plan* plan, const float* params, float* grads, void* workspace, const float* logits,
                               const float* target, float grad_scale, void* stream, int nslices, void* comm_stream,
                               octseg_slice_cb cb, void* user);

/* kind: 0 SGD, 1 Adam, 2 RMSprop, 3 RAdam (torch defaults for everything not listed).
 * state_m / state_v: fp32 arenas of numel elements (may be NULL when unused by the kind). */
int octseg_optim_step(int kind, float* params, const float* grads, float* state_m, float* state_v,
                      size_t numel, float lr, float weight_decay, int step, float grad_scale,
                      void* stream);

/* Deterministic-reduction mode (also OCTSEG_DETERMINISTIC=1 in the environment): weight gradients without split-K atomics, Dice sums and
 * bias gradients by one workgroup per output -- two runs of the same step give bit-identical losses and gradients (the default mode
 * orders its floating-point atomics by arrival).  Slower; for tests and debugging (torch.use_deterministic_algorithms' counterpart). */
int octseg_set_deterministic(int on);

/* diagnostic hook: with a library built with -DOCTSEG_STAMP, octseg_conv2d_forward adds per-phase cycle
 * sums of the tap loop into dev_buf[6] (u64, device); a no-op in the shipped build. */
int octseg_debug_set_stamp(unsigned long long* dev_buf);
/* Measurement aid: on = 1 runs every launch of forward and backward on the caller's stream, one after the other
 * (no forward lanes, no weight-gradient side stream), so that per-kernel durations are those of the kernels alone. */
int octseg_debug_set_serial(int on);

/* ---- single-op entry points (NHWC device tensors of `dtype`; weights fp32 in arena layout) ---- */
/* y[N,OH,OW,Cout] = conv(x[N,H,W,Cin], w[R][S][Cout][Cin]) (+bias);  transposed=1: ConvTranspose2d
 * 4x4 s2 p1 with w[R][S][Cout][Cin].  scratch: device bytes >= octseg_conv2d_scratch_bytes(). */
size_t octseg_conv2d_scratch_bytes(int dtype, int N, int H, int W, int Cin, int Cout, int R, int S);
int octseg_conv2d_forward(int dtype, const void* x, const float* w, const float* bias, void* y, int N,
                          int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                          int transposed, void* scratch, void* stream);
int octseg_conv2d_backward_data(int dtype, const void* dy, const float* w, void* dx, int N, int H, int W,
                                int Cin, int Cout, int R, int S, int stride, int pad, int transposed,
                                void* scratch, void* stream);
int octseg_conv2d_backward_weight(int dtype, const void* x, const void* dy, float* dw, int N, int H,
                                  int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                  int transposed, void* stream);

/* ---- single-layer door to the conv kernels' fused operand and epilogue paths (csrc/conv_api.cpp; wrappers in convops.py) ----
 * One call = the launches of ONE conv layer pass, with the descriptors the plan builds for it: the lazy BatchNorm affine + ReLU of every
 * source, nearest-x2 reads, channel concatenation, the eval fold (wscale, bias, relu_out), the BatchNorm statistics slab, several
 * data-gradient destinations with accum / pool, the head's NCHW f32 store.  The routing is launch_conv's / launch_wgrad's own.
 *   geometry   N, virtual input H x W (after `up`), R in {1, 3} (4 with transposed = ConvTranspose2d k4 s2 p1), stride 1 | 2, pad <= R / 2;
 *              OH x OW = (H + 2 pad - R) / stride + 1 (transposed: 2H x 2W)
 *   sources    nsrc <= 5 tensors T[N][H >> up][W >> up][C], concatenated in order (sum of C = Cin); scale / shift f[C] (both or neither):
 *              relu?(x * scale + shift) rounded to T on load, padding stays 0; relu only with the affine
 *   w          f[R][R][Cout][Cin] (arena layout); forward and data gradient pack it into `scratch` (>= octseg_conv2d_scratch_bytes())
 *   forward    wscale f[Cout] (folded into the packed image as launch_pack_all folds it for eval), bias f[Cout], relu_out (needs bias, excludes
 *              stat_slab); stat_slab f[slab_row0 + rows][Cout][2] = per row (sum y, sum y^2) of the f32 y (bias included) before the storage
 *              rounding, rows = octseg_conv_layer_slab_rows(); dst[0] = T[N][OH][OW][Cout] (+ accum), or head = 1: f32 NCHW [N][Cout][OH][OW]
 *   data grad  dy T[N][OH][OW][Cout]; dst[i] = gradient of source i: T[N][H][W][C_i] (+ accum), or pool = 1 (an `up` source at stride 1):
 *              T[N][H / 2][W / 2][C_i], every 2x2 quad summed in the epilogue.  A stride-2 1x1 layer covers one pixel parity only: accum = 1
 *              over a zeroed tensor, as the plan does it
 *   weight grad  the same sources (affine included), dy, and dW f[R][R][Cout][Cin] ACCUMULATED with atomics onto what is there
 * Refused before any launch: a null required or misaligned (16 B) pointer, scale without shift, relu without the affine, pool elsewhere than
 * stated, relu_out with stat_slab or without bias, bias with stat_slab where the launch would go to gemm1x1 (the plan never builds it),
 * a slab / accum / transposed layer in head mode, forward-only fields in a gradient mode, a scratch too small: OCTSEG_BAD_ARG; more than 5
 * sources, extents that do not match H >> up, C / Cout not whole 16-byte vectors (4 f32, 8 bf16 / f16; a head's Cout is free), unsupported
 * geometry: OCTSEG_BAD_SHAPE; f16 in a gradient mode: OCTSEG_BAD_DTYPE. */
#define OCTSEG_CONV_MAX_SRC 5
typedef enum { OCTSEG_CONV_FORWARD = 0, OCTSEG_CONV_BACKWARD_DATA = 1, OCTSEG_CONV_BACKWARD_WEIGHT = 2 } octseg_conv_mode;
/* octseg_conv_layer_route: forward / data gradient launches ...; -1 = a launch without taps (nothing runs) */
typedef enum { OCTSEG_ROUTE_THIN = 0, OCTSEG_ROUTE_GEMM1X1, OCTSEG_ROUTE_CONV3X3P, OCTSEG_ROUTE_MFMA16, OCTSEG_ROUTE_MFMA11,
               OCTSEG_ROUTE_MFMA_WIDEN,
               /* octseg_tied_layer_route only: conv_mfma's masked loops over per-source tap subsets (ConvArgs::taps_per_src), by tile */
               OCTSEG_ROUTE_MFMA11_MASKED, OCTSEG_ROUTE_MFMA16_MASKED } octseg_conv_route;
/* ... weight gradient launches (CONVT16: the four parities of a ConvTranspose2d in one launch) */
typedef enum { OCTSEG_WROUTE_THIN = 0, OCTSEG_WROUTE_WGRAD1X1, OCTSEG_WROUTE_CONVT16, OCTSEG_WROUTE_MFMA } octseg_wgrad_route;
typedef struct {
  const void* ptr; const float* scale; const float* shift;
  int C, H, W, up, relu;          /* H, W: stored extents */
} octseg_conv_src;
typedef struct { void* ptr; int accum, pool; } octseg_conv_dst;
typedef struct {
  int N, H, W, Cin, Cout, R, stride, pad, transposed;
  int nsrc;
  octseg_conv_src src[OCTSEG_CONV_MAX_SRC];
  const float* w; const float* wscale; const float* bias;
  int relu_out;
  float* stat_slab; int slab_row0;
  int head;
  octseg_conv_dst dst[OCTSEG_CONV_MAX_SRC];
  const void* dy; float* dW;
  void* scratch; size_t scratch_bytes;
} octseg_conv_layer_desc;
int octseg_conv_layer_op(int mode, int dtype, const octseg_conv_layer_desc* desc, void* stream);
/* which kernel each launch of that call runs (route_per_launch: at least 4 ints), and the slab rows of a forward; nothing is launched */
int octseg_conv_layer_route(int mode, int dtype, const octseg_conv_layer_desc* desc, int* route_per_launch, int* nlaunch);
int octseg_conv_layer_slab_rows(int dtype, const octseg_conv_layer_desc* desc, int* rows);

/* ---- the tied decoder layer (csrc/conv_api.cpp; wrappers in convops.py) ----
 * One call = one pass of a (nearest x2, concat, 3x3 stride 1 pad 1) decoder layer through the tied decomposition of the plan (OCTSEG_TIED, DESIGN.md
 * section 7.7), bf16 only.  The descriptor is the one above with R = 3, stride = 1, pad = 1: src[0] the `up` source (Ca channels, stored
 * at H / 2 x W / 2), src[1..] the skip sources at full resolution (Cs channels together; none: Cs = 0); wscale, bias, relu_out, the slab and
 * head stay unset.  The weight images (4x4 image of sums of 3x3 taps over the Ca slice, forward and data gradient; the 3x3 image of the skip
 * slice) are packed into `scratch` by launch_pack_all with the plan's pack jobs; scratch >= octseg_tied_layer_scratch_bytes().
 *   FORWARD          what tied_forward() runs without its statistics sweep: the skip slice's 3x3 stores dst[0] = T[N][H][W][Cout] (rule 'staged'),
 *                    the four parity launches of the 4x4 stride-2 kernel add to it, each T(f32(T(partial)) + old); Cs = 0: each stores its pixels
 *   BACKWARD_DATA    dst[0] = T[N][H / 2][W / 2][Ca]: T(y), or T(f32(T(y)) + old) with accum, y = the WHOLE sum of the low-resolution gradient
 *                    (one masked launch over dy's four parity planes, or the 16-tap stride-2 launch): nothing is pooled, dst[0].pool = 0;
 *                    dst[i] = T[N][H][W][C_i] (+ accum) of the skip sources from the skip slice's 3x3 data gradient
 *   BACKWARD_WEIGHT  dW f[3][3][Cout][Cin] += the fold of the 4x4 image's gradient (wgrad_convt16 or four parity launches) and the skip slice's;
 *                    wg_target = split-K width (0: the full width; octseg_side_wgs(): the plan's narrowing on its side stream)
 * Refused before any launch: what octseg_conv_layer_op refuses in pointers and fused fields, a set wscale / relu_out / slab / head / pool,
 * accum on a forward, a scratch too small, wg_target < 0: OCTSEG_BAD_ARG; a layer the plan would not tie (tie_eligible: Ca >= 64, Cs = 0 or
 * >= 32, Cout >= 32, all in whole vectors, only src[0] upsampled, no bias): OCTSEG_BAD_SHAPE; f32 and f16: OCTSEG_BAD_DTYPE.
 * FORWARD and BACKWARD_DATA upload the four-entry job table and wait for that copy on `stream` before they enqueue the launches. */
int octseg_tied_layer_op(int pass, int dtype, const octseg_conv_layer_desc* desc, int wg_target, void* stream);
/* route_per_launch: at least 6 ints, in launch order (forward: skip, four parities; data gradient: the up slice's launch, skip; weight gradient:
 * CONVT16 or four parities, skip; the pack, clear and fold launches are not listed) */
int octseg_tied_layer_route(int pass, int dtype, const octseg_conv_layer_desc* desc, int wg_target, int* route_per_launch, int* nlaunch);
size_t octseg_tied_layer_scratch_bytes(int dtype, const octseg_conv_layer_desc* desc);   /* 0: refused (octseg_last_error says why) */
int octseg_side_wgs(void);

/* ---- single-launch door to the stem kernels (csrc/stem_api.cpp; wrappers in convops.py) ----
 * One call = one launch over the NCHW f32 frame img f[N][3][H][W], normalised on the fly when normalize = 1: every kernel sees the frame as
 * T(f32(f32(raw - mean[c]) * f32(1 / stdv[c]))), zero outside (the padding is applied AFTER the normalisation).  OH x OW = H / 2 x W / 2.
 *   IM2COL   launch_stem_im2col: col T[N][OH][OW][KP], column k = (r * ksize + s) * 3 + c holds pixel (2 oy - pad + r, 2 ox - pad + s) of channel
 *            c, columns >= 3 ksize^2 are zero.  (ksize, pad, KP) = (7, 3, 160) ResNet, (3, 1, 32) RegNet, (3, 0, 32) EfficientNet; every dtype.
 *            The f32 and deterministic paths run the stem as this launch + a 1x1 layer of KP input channels (octseg_conv_layer_op).
 *   FORWARD  thin.hip's 7x7 stride-2 pad-3 conv 3 -> 64 straight from the frame (bf16, f16): w f[64][160] with k as above (columns >= 147 are
 *            never read); y T[N][OH][OW][64] = T(conv (+ bias, relu_out)); training: stat_slab f[slab_row0 + rows][64][2] = per row (sum y,
 *            sum y^2) of the f32 y, rows = octseg_stem_slab_rows() (one per workgroup); eval: wscale f[64] (W * wscale in f32, then rounded to
 *            T), bias f[64], relu_out (needs bias, excludes stat_slab)
 *   WGRAD    thin.hip's weight gradient (bf16, not in deterministic mode): dy T[N][OH][OW][64]; dW f[64][160] ACCUMULATED with atomics onto
 *            what is there; columns 147..159 receive +0
 * Refused before any launch: a null required or misaligned (16 B) pointer, relu_out without bias or with stat_slab, a negative slab_row0,
 * weight-gradient fields in a forward and the reverse, normalize with a non-positive std, WGRAD in deterministic mode: OCTSEG_BAD_ARG;
 * odd or empty H / W, another (ksize, pad, KP), 2^31 elements or more: OCTSEG_BAD_SHAPE; f32 in FORWARD / WGRAD, f16 in WGRAD: OCTSEG_BAD_DTYPE. */
typedef enum { OCTSEG_STEM_IM2COL = 0, OCTSEG_STEM_FORWARD = 1, OCTSEG_STEM_WGRAD = 2 } octseg_stem_stage;
typedef struct {
  int N, H, W;
  const float* img;
  int normalize; float mean[3], stdv[3];
  int ksize, pad, KP; void* col;                        /* IM2COL */
  const float* w; const float* wscale; const float* bias; int relu_out;
  void* y; float* stat_slab; int slab_row0;             /* FORWARD */
  const void* dy; float* dW;                            /* WGRAD */
} octseg_stem_desc;
int octseg_stem_op(int stage, int dtype, const octseg_stem_desc* desc, void* stream);
int octseg_stem_slab_rows(int N, int H, int W);         /* thin_stem_rows: slab rows a FORWARD writes (0: empty frame) */

/* ---- single-op door to the NHWC sweep kernels (BatchNorm finalize / apply / backward, pools, resamplers, gates, gradient plumbing) ----
 * One call = one launcher of csrc/kernels.h on `stream` (bn_bwd_finalize etc. included: the caller chains reduce -> finalize -> apply).
 * ptrs: device pointers, in the order listed per op (NULL where an operand is optional), every one 16-byte aligned; iargs / fargs: the
 * op's integer / float arguments in the order listed.  T = `dtype`; f = float32 whatever the dtype.  The counts must match the op.
 * Refused before any launch: unknown op, wrong counts, a null required or misaligned pointer: OCTSEG_BAD_ARG; f16 on a training-only sweep
 * (marked "train"): OCTSEG_BAD_DTYPE; an empty tensor, C not a multiple of the 16-byte vector (4 f32, 8 bf16 / f16), odd H or W for the
 * 2x pools and the parity permute, k < 1, rows < 1: OCTSEG_BAD_SHAPE.  Buffer sizes are the caller's contract (oct_segmentation_amd/sweeps.py
 * derives every one of them from the tensors' shapes). */
typedef enum {
  OCTSEG_SWEEP_BN_FINALIZE_TRAIN = 0,   /* ptrs slab f[rows][C][2], gamma, beta, running_mean, running_var, scale, shift, mean, rstd (f[C]),
                                           part (double[32768]), counters (64 zeroed uint32); iargs rows, C; fargs count, momentum, eps */
  OCTSEG_SWEEP_BN_FINALIZE_SMALL,       /* train. ptrs y T[count][C], gamma, beta, running_mean, running_var, scale, shift, mean, rstd; iargs count
                                           (<= 1024), C; fargs momentum, eps */
  OCTSEG_SWEEP_BN_FINALIZE_EVAL,        /* ptrs gamma, beta, running_mean, running_var, scale, shift; iargs C; fargs eps */
  OCTSEG_SWEEP_BN_FINALIZE_FROZEN,      /* ptrs gamma, beta, running_mean, running_var, scale, shift, mean, rstd, coef f[C][2]; iargs C; fargs eps */
  OCTSEG_SWEEP_BN_ACT,                  /* ptrs y, scale?, shift?, res?, rscale?, rshift?, post?, out, maskbits? (a byte per vector); iargs npix, C, relu */
  /* the four BatchNorm-backward launchers share one pointer list: g, y, out?, maskbits?, scale, shift, mean, rstd, gamma, slab f[rows][C][2],
   * dgamma, dbeta, coef f[C][2], dy, part (double[32768]), counters (64 zeroed uint32), res_grad?; iargs npix, C, mask (0 | 1 | 2), rows,
   * res_store.  Each needs the operands its launcher reads or writes (SMALL: no slab / part / counters; REDUCE: g .. rstd and slab;
   * FINALIZE: slab, dgamma, dbeta, coef, part, counters; APPLY: g .. gamma, coef, dy); dy may alias g. */
  OCTSEG_SWEEP_BN_BWD_SMALL,            /* train; npix <= 1024 */
  OCTSEG_SWEEP_BN_BWD_REDUCE,           /* train */
  OCTSEG_SWEEP_BN_BWD_FINALIZE,
  OCTSEG_SWEEP_BN_BWD_APPLY,            /* train */
  OCTSEG_SWEEP_MASKED_ACCUM,            /* train. ptrs dst, g, out_mask?; iargs numel, store */
  OCTSEG_SWEEP_POOL2X2_ACCUM,           /* train. ptrs dst T[N][H][W][C], src T[N][2H][2W][C]; iargs N, H, W, C, store */
  OCTSEG_SWEEP_UP2_FILL,                /* ptrs in T[N][H][W][C], out T[N][2H][2W][C]; iargs N, H, W, C */
  OCTSEG_SWEEP_RELU,                    /* ptrs in, mask?, out; iargs numel */
  OCTSEG_SWEEP_ADD2,                    /* ptrs a, b, out; iargs numel */
  OCTSEG_SWEEP_DROP_ELEM,               /* ptrs in, keep? f[numel], out; iargs numel; fargs mscale */
  OCTSEG_SWEEP_MERGE_DROP,              /* ptrs a0, a1, a2, a3, m? f[N][C], out; iargs N, HW, C; fargs mscale */
  OCTSEG_SWEEP_DROP_BWD,                /* ptrs gout, m? f[N][C], gin; iargs N, HW, C; fargs mscale */
  OCTSEG_SWEEP_CHANNEL_SUM,             /* train. ptrs g T[npix][Cstride], out f[C] (accumulated); iargs npix, Cstride, C (any C >= 1) */
  OCTSEG_SWEEP_TENSOR_STATS,            /* train. ptrs y T[npix][C], slab f[rows][C][2]; iargs npix, C, rows */
  OCTSEG_SWEEP_MAXPOOL_FWD,             /* ptrs in T[N][H][W][C], out T[N][H/2][W/2][C], idx? (a byte per output element); iargs N, H, W, C */
  OCTSEG_SWEEP_MAXPOOL_BWD_IDX,         /* train. ptrs idx, gout T[N][H/2][W/2][C], gin T[N][H][W][C]; iargs N, H, W, C, store */
  OCTSEG_SWEEP_BILINEAR_RESIZE,         /* ptrs in T[N][IH][IW][C], out T[N][OH][OW][C]; iargs N, IH, IW, OH, OW, C */
  OCTSEG_SWEEP_BILINEAR_RESIZE_ADJOINT, /* train. ptrs gout T[N][OH][OW][C], gin T[N][IH][IW][C]; iargs N, IH, IW, OH, OW, C */
  OCTSEG_SWEEP_BILINEAR_ADJOINT,        /* train. ptrs gout T[N][H up][W up][C], gin T[N][H][W][C]; iargs N, H, W, C, up (>= 2) */
  OCTSEG_SWEEP_BIN_MEAN,                /* ptrs in T[N][H][W][C], out T[N][k][k][C]; iargs N, H, W, C, k */
  OCTSEG_SWEEP_BIN_MEAN_BWD,            /* train. ptrs gout T[N][k][k][C], gin T[N][H][W][C]; iargs N, H, W, C, k, accum */
  OCTSEG_SWEEP_IMAGE_SUM,               /* ptrs in T[N][HW][C], out T[N][C]; iargs N, HW, C; fargs div */
  OCTSEG_SWEEP_IMAGE_BCAST,             /* ptrs in T[N][C], out T[N][HW][C]; iargs N, HW, C, accum; fargs scale */
  OCTSEG_SWEEP_SE_GATE,                 /* ptrs in T[N][HW][C], s T[N][C], out, s2? T[N][C]; iargs N, HW, C, accum */
  OCTSEG_SWEEP_SE_DGATE,                /* train. ptrs g, x T[N][HW][C], s T[N][C], ds T[N][C], part f[N][shares(HW)][C], s2?, ds2?; iargs N, HW, C;
                                           shares(HW) = clamp(HW / 64, 1, 64) */
  OCTSEG_SWEEP_PARITY_PERMUTE,          /* ptrs src, dst (fine T[N][H][W][C] <-> coarse T[4N][H/2][W/2][C]); iargs N, H, W, C, to_coarse, accum */
  OCTSEG_SWEEP_MOSAIC,                  /* ptrs src, dst (fine T[N][H][W][C] <-> mosaic T[N][r (hs + 1) + 1][r (ws + 1) + 1][C], hs = ceil(H / r));
                                           iargs N, H, W, C, r, to_mosaic, accum */
  OCTSEG_SWEEP_DW_CONV,                 /* depthwise 3x3, dilation = padding = dil, on channel slices.  ptrs in T[N][H][W][inC], out T[N][H][W][outC],
                                           w f[9][wC]; iargs inC, ic0, outC, oc0, wC, wc0, N, H, W, C, dil, flip, accum (wC, wc0 multiples of 4) */
  OCTSEG_SWEEP_DW_WGRAD,                /* train. ptrs in T[N][H][W][inC], gout T[N][H][W][goC], dw f[9][wC] (accumulated); iargs inC, ic0, goC, oc0,
                                           wC, wc0, N, H, W, C, dil */
  OCTSEG_SWEEP_CAM_SEED,                /* train. ptrs seed f[B][C][HW], dlogits T[B][HW][CP] (zeros beyond C); iargs B, C, HW, CP (8 | 16) */
  /* depthwise K x K (3 | 5), stride 1 | 2, top / left padding `pad` (TF static "same"); w / dw: f[K][K][C] */
  OCTSEG_SWEEP_DWG_FWD,                 /* ptrs in T[N][H][W][C], out T[N][OH][OW][C], w; iargs N, H, W, C, OH, OW, K, stride, pad */
  OCTSEG_SWEEP_DWG_BWD_DATA,            /* train. ptrs gout T[N][OH][OW][C], gin T[N][H][W][C], w; iargs as DWG_FWD, accum */
  OCTSEG_SWEEP_DWG_BWD_W,               /* train. ptrs in, gout, dw (accumulated); iargs as DWG_FWD */
  OCTSEG_SWEEP_BNX_FWD,                 /* out = act(y scale + shift) dscale[n] + post.  ptrs y, scale?, shift?, dscale? f[npix / hw], post?, out;
                                           iargs npix, hw (pixels per image), C, act (0 identity | 1 swish) */
  OCTSEG_SWEEP_BNX_BWD,                 /* train. out = g dscale[n] act'(y scale + shift).  ptrs y?, scale?, shift?, dscale?, g, out; iargs as BNX_FWD */
  OCTSEG_SWEEP_DICE_BWD,                /* train. ptrs logits, target f[B][C][HW], sums double[1 + B][C][4] (I, S, T, BCE totals first), dlogits T[B][HW][CP]
                                           (zeros beyond C); iargs B, C, HW, CP (8 | 16), loss kind (0 dice | 1 bce | 2 both); fargs grad_scale */
  /* GroupNorm(G) + ReLU (+ bilinear x2, align_corners) of [N][HW][C]; C <= 1024 with C / vector a divisor of 256; S = clamp(HW / 1024, 1, 64) */
  OCTSEG_SWEEP_GN_FORWARD,              /* ptrs y, gamma, beta, out T[N][H up][W up][C], part f[N][S][C][2], ss f[N][C][2], stat f[N][G][2]; iargs N, H, W,
                                           C, G, up (1 | 2); fargs eps */
  OCTSEG_SWEEP_GN_BACKWARD,             /* train. ptrs y, g, dy (may alias g), gamma, dgamma, dbeta (accumulated), part, ss, stat (the forward's),
                                           coef f[N][G][2]; iargs N, HW, C, G */
  /* squeeze-excite excitation s = W2 act(W1 m + b1) + b2 on pooled vectors; W1 f[R][C], W2 f[C][R]; h, dh f[N][R] */
  OCTSEG_SWEEP_SEFC_FWD,                /* ptrs m T[N][C], s T[N][C], w1, b1, w2, b2, h; iargs N, C, R, act (0 ReLU | 1 swish) */
  OCTSEG_SWEEP_SEFC_BWD,                /* train. ptrs m, ds, dm T[N][C], w1, w2, h, dh, dw1?, db1?, dw2?, db2? (accumulated; all four or none); iargs as SEFC_FWD */
  OCTSEG_SWEEP_NUM_OPS
} octseg_sweep;
int octseg_sweep_op(int op, int dtype, const void* const* ptrs, int nptrs, const long long* iargs, int niargs, const double* fargs,
                    int nfargs, void* stream);

/* ---- single-stage door to the PAN pyramid (csrc/pan.hip) and the MAnet position attention (csrc/pab.hip); csrc/block_api.cpp, wrappers in
 * blockops.py ----
 * One call = ONE launcher of csrc/kernels.h on `stream` (IN_BWD: the launcher's two kernels; PYR_BWD: the launcher's memset of gscratch and its
 * kernel).  T = `dtype`; f = float32 whatever the dtype.  A stage reads only the fields listed for it.  Buffer sizes are the caller's contract
 * (blockops.py derives every one of them); the door checks what it can see.
 *   MAXPOOL2_FWD   x T[N][H][W][C] -> p T[N][H/2][W/2][C]                                 (16-byte vectors: C % vec == 0, H and W even)
 *   MAXPOOL2_BWD   train. x, dp T[N][H/2][W/2][C] -> dx T[N][H][W][C]: the first maximum in scan order takes dp, the others 0; accum: dx +=
 *   IN_FWD         p T[N][H][W][C], w f[K*K][C], b f[1] -> y f[N][H][W]                   (K x K conv to one channel, pad K / 2; K odd, <= 15)
 *   IN_BWD         train. p, dy f[N][H][W], w -> dp T[N][H][W][C] (stored), dw f[K*K][C] and db f[1] (accumulated)
 *   PYR_FWD        the one-channel pyramid below an H x W map (H / 8 >= 1, W / 8 >= 1): x1raw = scratch[0 .. N (H/2) (W/2)) -> every
 *                  intermediate in `scratch` (layout: pan.hip / blockops.fpa_scratch_views), uu f[N][H][W] at scratch + octseg_fpa_uu_offset().
 *                  Layers l = 0..5 = down1, down2, down3.1, down3.2, conv2, conv1: pw[l] f[k*k] and pb[l] f[1] for l >= 1 (layer 0's conv is IN_FWD),
 *                  pg[l], pbe[l], prm[l], prv[l] f[1].  train = 1: batch statistics (running statistics updated, 12 statistics kept); 0: running ones
 *   PYR_BWD        train. scratch as PYR_FWD(train = 1) left it, duu f[N][H][W] -> gscratch (zeroed here; d x1raw at gscratch + N (H/2) (W/2)),
 *                  pdw[l], pdb[l] (l >= 1), pdg[l], pdbe[l] accumulated; reads pw[l] (l >= 1), pg[l]
 *   MIX_FWD        uu f[N][HW], mid T[N][HW][C], b1 T[N][C] -> out T[N][HW][C] = uu mid + b1        (HW = H * W of the descriptor)
 *   MIX_BWD        train. uu, mid, g T[N][HW][C] -> dmid T[N][HW][C] = g uu, duu f[N][HW] = sum_c g mid
 *   PAB GEMM       octseg_pab_gemm verbatim (the launcher's PabGemm): C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n], strides in elements, *_f32: the
 *                  operand is float whatever the dtype; numelA / numelB / numelC: the elements of the three buffers
 *   PAB SOFTMAX_FWD  S f[batch][n]: softmax over ALL n entries of each image, in place
 *   PAB SOFTMAX_BWD  train. S = dP f[batch][n] -> P (dP - sum P dP) in place; P f[batch][n] is only read
 *   PAB MIX_FWD    x T[N][HW][C], M f[N][HW * C] -> y = x + M read as [C][HW] (the un-transposed reshape)
 *   PAB MIX_BWD    train. dy T[N][HW][C] -> dM f[N][HW * C] (the same index map)
 * Refused before any launch: unknown stage, null descriptor, a null required pointer, a pointer not aligned to its element (16 bytes for
 * maxpool2's tensors), scratch_floats / gscratch_floats below octseg_fpa_scratch_floats() / octseg_fpa_gscratch_floats(): OCTSEG_BAD_ARG;
 * f16 on a stage marked "train": OCTSEG_BAD_DTYPE; an empty tensor, C % vec != 0 or odd H / W for maxpool2, H / 8 < 1 or W / 8 < 1 for the
 * pyramid, K even or above 15, batch > 65535, n == 0, a tensor of 2^31 elements or more, train with N (H/8) (W/8) <= 1 ("Expected more than 1
 * value per channel when training ..."), a GEMM whose largest reachable index of A, B or C lies beyond numelA / numelB / numelC:
 * OCTSEG_BAD_SHAPE. */
typedef enum { OCTSEG_FPA_MAXPOOL2_FWD = 0, OCTSEG_FPA_MAXPOOL2_BWD, OCTSEG_FPA_IN_FWD, OCTSEG_FPA_IN_BWD, OCTSEG_FPA_PYR_FWD, OCTSEG_FPA_PYR_BWD,
               OCTSEG_FPA_MIX_FWD, OCTSEG_FPA_MIX_BWD, OCTSEG_FPA_NUM_STAGES } octseg_fpa_stage;
typedef struct {
  int N, H, W, C, K, train, accum;
  const void* x; void* p; void* dp; void* dx;                              /* MAXPOOL2_* (writes p | reads dp), IN_* (reads p | writes dp) */
  const float* w; const float* b; float* y; const float* dy; float* dw; float* db;      /* IN_* */
  float* scratch; size_t scratch_floats; float* gscratch; size_t gscratch_floats;       /* PYR_* */
  const float* pw[6]; const float* pb[6]; const float* pg[6]; const float* pbe[6]; float* prm[6]; float* prv[6];
  float* pdw[6]; float* pdb[6]; float* pdg[6]; float* pdbe[6];
  const float* uu; float* duu;                                             /* MIX_* (duu: also PYR_BWD's input) */
  const void* mid; const void* b1; void* out; const void* g; void* dmid;
} octseg_fpa_desc;
size_t octseg_fpa_scratch_floats(int N, int H, int W);    /* 0 where the pyramid refuses the map */
size_t octseg_fpa_gscratch_floats(int N, int H, int W);
size_t octseg_fpa_uu_offset(int N, int H, int W);         /* floats from scratch to uu; the 12 statistics follow uu */
int octseg_fpa_op(int stage, int dtype, const octseg_fpa_desc* desc, void* stream);

typedef enum { OCTSEG_PAB_GEMM = 0, OCTSEG_PAB_SOFTMAX_FWD, OCTSEG_PAB_SOFTMAX_BWD, OCTSEG_PAB_MIX_FWD, OCTSEG_PAB_MIX_BWD, OCTSEG_PAB_NUM_STAGES } octseg_pab_stage;
typedef struct {
  const void* A; const void* B; void* C;
  size_t sAb, sAm, sAk, sBb, sBk, sBn, sCb, sCm, sCn;
  int M, N, K, batch, a_f32, b_f32, c_f32, accum;
} octseg_pab_gemm;
typedef struct {
  octseg_pab_gemm gemm; size_t numelA, numelB, numelC;                     /* GEMM */
  float* S; const float* P; int batch; size_t n;                           /* SOFTMAX_* */
  const void* x; const float* M; void* y; float* dM; const void* dy; int N, HW, C;      /* MIX_* */
} octseg_pab_desc;
int octseg_pab_op(int stage, int dtype, const octseg_pab_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCTSEG_H */
