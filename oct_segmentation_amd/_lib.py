"""ctypes binding of ``liboctseg_hip.so`` (C ABI declared in ``include/octseg.h``).

The product path has no CPU fallback: if the library is missing or a call
fails, a ``RuntimeError`` is raised with ``octseg_last_error()``.
"""
import ctypes as C
import os

# HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) in creation order.  The engine overlaps the weight gradients (side
# stream) and a forward lane with the caller's stream; once RCCL has created its own streams (init_process_group("nccl")) the side
# stream can land on the SAME hardware queue as the main one and the overlap is silently gone: measured on one MI355X, U-Net++/resnet101
# B=16, 74.2 -> 80.8 ms per step with a one-rank RCCL group and nothing else changed, 74.6 with 8 (or 2) queues.  The setting is NOT
# free for hipGraph replay, though: with 8 queues the replayed serving ensemble runs at 15.7 ms per frame instead of 7.0 and a replayed
# training step at 98.5 ms instead of 79.2 (profiles/r3_hw_queues_ab.txt), and with 2 graph instantiation fails.  So it is applied to
# the processes that open a process group -- the ranks of a torchrun launch (WORLD_SIZE > 1); single-GPU processes keep HIP's
# default.  Must be in the environment before the HIP runtime initialises (first torch.cuda call); an explicit setting of the user wins.
def set_hw_queues_for_collectives():
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')


if int(os.environ.get('WORLD_SIZE', '1') or 1) > 1:
    set_hw_queues_for_collectives()

# torch bundles its own libamdhip64; it must be the HIP runtime this process binds (streams and device
# pointers are torch's), so torch is loaded before liboctseg_hip.so resolves its libamdhip64 dependency.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'liboctseg_hip.so')

F32, BF16, F16 = 0, 1, 2
P_CONV, P_CONVT, P_STEM, P_VEC = 0, 1, 2, 3
OPT_KINDS = {'SGD': 0, 'Adam': 1, 'RMSprop': 2, 'RAdam': 3}


class NetDesc(C.Structure):
    _fields_ = [('arch', C.c_char_p), ('encoder', C.c_char_p), ('classes', C.c_int), ('batch', C.c_int),
                ('height', C.c_int), ('width', C.c_int), ('dtype', C.c_int)]


class ParamInfo(C.Structure):
    _fields_ = [('name', C.c_char * 128), ('kind', C.c_int), ('R', C.c_int), ('S', C.c_int), ('O', C.c_int),
                ('I', C.c_int), ('KP', C.c_int), ('offset', C.c_size_t), ('numel', C.c_size_t)]


class BNInfo(C.Structure):
    _fields_ = [('name', C.c_char * 128), ('C', C.c_int), ('mean_offset', C.c_size_t), ('var_offset', C.c_size_t)]


class ConvSrc(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p), ('C', C.c_int), ('H', C.c_int), ('W', C.c_int),
                ('up', C.c_int), ('relu', C.c_int)]


class ConvDst(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('accum', C.c_int), ('pool', C.c_int)]


CONV_MAX_SRC = 5


class ConvLayerDesc(C.Structure):   # octseg_conv_layer_desc
    _fields_ = [('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('R', C.c_int), ('stride', C.c_int),
                ('pad', C.c_int), ('transposed', C.c_int), ('nsrc', C.c_int), ('src', ConvSrc * CONV_MAX_SRC), ('w', C.c_void_p),
                ('wscale', C.c_void_p), ('bias', C.c_void_p), ('relu_out', C.c_int), ('stat_slab', C.c_void_p), ('slab_row0', C.c_int),
                ('head', C.c_int), ('dst', ConvDst * CONV_MAX_SRC), ('dy', C.c_void_p), ('dW', C.c_void_p), ('scratch', C.c_void_p),
                ('scratch_bytes', C.c_size_t)]


class StemDesc(C.Structure):   # octseg_stem_desc
    _fields_ = [('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('img', C.c_void_p), ('normalize', C.c_int), ('mean', C.c_float * 3),
                ('stdv', C.c_float * 3), ('ksize', C.c_int), ('pad', C.c_int), ('KP', C.c_int), ('col', C.c_void_p), ('w', C.c_void_p),
                ('wscale', C.c_void_p), ('bias', C.c_void_p), ('relu_out', C.c_int), ('y', C.c_void_p), ('stat_slab', C.c_void_p),
                ('slab_row0', C.c_int), ('dy', C.c_void_p), ('dW', C.c_void_p)]


_PF6 = C.c_void_p * 6


class FpaDesc(C.Structure):   # octseg_fpa_desc
    _fields_ = ([(k, C.c_int) for k in ('N', 'H', 'W', 'C', 'K', 'train', 'accum')] +
                [(k, C.c_void_p) for k in ('x', 'p', 'dp', 'dx', 'w', 'b', 'y', 'dy', 'dw', 'db')] +
                [('scratch', C.c_void_p), ('scratch_floats', C.c_size_t), ('gscratch', C.c_void_p), ('gscratch_floats', C.c_size_t)] +
                [(k, _PF6) for k in ('pw', 'pb', 'pg', 'pbe', 'prm', 'prv', 'pdw', 'pdb', 'pdg', 'pdbe')] +
                [(k, C.c_void_p) for k in ('uu', 'duu', 'mid', 'b1', 'out', 'g', 'dmid')])


class PabGemm(C.Structure):   # octseg_pab_gemm (= the launcher's PabGemm)
    _fields_ = ([(k, C.c_void_p) for k in ('A', 'B', 'C')] +
                [(k, C.c_size_t) for k in ('sAb', 'sAm', 'sAk', 'sBb', 'sBk', 'sBn', 'sCb', 'sCm', 'sCn')] +
                [(k, C.c_int) for k in ('M', 'N', 'K', 'batch', 'a_f32', 'b_f32', 'c_f32', 'accum')])


class PabDesc(C.Structure):   # octseg_pab_desc
    _fields_ = [('gemm', PabGemm), ('numelA', C.c_size_t), ('numelB', C.c_size_t), ('numelC', C.c_size_t),
                ('S', C.c_void_p), ('P', C.c_void_p), ('batch', C.c_int), ('n', C.c_size_t),
                ('x', C.c_void_p), ('M', C.c_void_p), ('y', C.c_void_p), ('dM', C.c_void_p), ('dy', C.c_void_p), ('N', C.c_int), ('HW', C.c_int),
                ('C', C.c_int)]


# every exported symbol with (restype, argtypes), in the order of include/octseg.h; tests check the library exports all of them
_P = C.c_void_p
LOSS_KINDS = {'dice': 0, 'bce': 1, 'dice+bce': 2}
SLICE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t)
SYMBOLS = {
    'octseg_version': (C.c_int, []),
    'octseg_last_error': (C.c_char_p, []),
    'octseg_plan_create': (C.c_int, [C.POINTER(NetDesc), C.POINTER(_P)]),
    'octseg_plan_destroy': (C.c_int, [_P]),
    'octseg_plan_workspace_bytes': (C.c_size_t, [_P]),
    'octseg_plan_param_numel': (C.c_size_t, [_P]),
    'octseg_plan_buffer_numel': (C.c_size_t, [_P]),
    'octseg_plan_num_params': (C.c_int, [_P]),
    'octseg_plan_param_info': (C.c_int, [_P, C.c_int, C.POINTER(ParamInfo)]),
    'octseg_plan_num_bn': (C.c_int, [_P]),
    'octseg_plan_bn_info': (C.c_int, [_P, C.c_int, C.POINTER(BNInfo)]),
    'octseg_plan_fwd_macs': (C.c_double, [_P]),
    'octseg_plan_exec_macs': (C.c_int, [_P, C.POINTER(C.c_double)]),
    'octseg_plan_find_tensor': (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    'octseg_profile_start': (C.c_int, []),
    'octseg_profile_stop': (C.c_int, [C.POINTER(C.c_double)]),
    'octseg_plan_params_changed': (C.c_int, [_P]),
    'octseg_plan_set_dropout': (C.c_int, [_P, _P]),
    'octseg_plan_set_drop_connect': (C.c_int, [_P, _P]),
    'octseg_plan_num_drop_connect': (C.c_int, [_P]),
    'octseg_plan_drop_connect_rate': (C.c_float, [_P, C.c_int]),
    'octseg_plan_set_graph': (C.c_int, [_P, C.c_int]),
    'octseg_net_forward': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.c_int, _P]),
    'octseg_augment': (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    'octseg_mask_assemble': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    # M members' logits (host arrays of device pointers, classes, channels, view codes) -> voted mask, mean probability, dissent, counts (csrc/vote.hip)
    'octseg_vote_assemble': (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 4 + [_P] * 6),
    # logits + target -> int32 [N, classes, 2, 256] probability histograms per truth label (csrc/curves.hip)
    'octseg_logit_histogram': (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P, _P]),
    # uint8 frames / masks -> float32 NCHW batch (csrc/ingest.hip)
    'octseg_ingest_image': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    'octseg_ingest_mask': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    'octseg_debug_set_ingest_variant': (C.c_int, [C.c_int]),
    # float32 mask stack + uint8 frames -> uint8 overlay + colour mask (csrc/render.hip)
    'octseg_render_results': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P]),
    # float32 frames + logits + raw uint8 ground truth -> uint8 image | ground truth | prediction strips and label maps (csrc/panels.hip)
    'octseg_epoch_panels': (C.c_int, [_P, _P, _P] + [C.c_int] * 6 + [_P] * 8),
    # float32 mask stack + host ray table -> int32 set-pixel counts and per-degree radii (csrc/measure.hip)
    'octseg_stack_measure': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    # float32 mask stack + the same ray table -> int32 polar profile [N, C, 360, 5] (+ uint8 label map); uint8 frames -> polar view (csrc/polar.hip)
    'octseg_stack_polar': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    'octseg_frames_unwrap': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    # float32 mask stack -> int64 moments, box and crack perimeter [N, C, 12]; -> int32 centroid pixels [N, C, 3]; + offset table [360, R, 2] ->
    # the polar profile from those pixels and the rays' lengths (csrc/shape.hip)
    'octseg_stack_moments': (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P]),
    'octseg_moment_origins': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, _P]),
    'octseg_stack_polar_at': (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P, C.c_int, _P, _P, _P]),
    # float32 mask stack -> connected components (labels, count, the 8 largest) and the cleaned stack: smooth, keep-largest, hole fill
    # (csrc/components.hip)
    'octseg_components_scratch_bytes': (C.c_size_t, [C.c_int] * 3),
    'octseg_stack_components': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P, _P, _P]),
    'octseg_stack_cleanup': (C.c_int, [_P] + [C.c_int] * 8 + [_P, C.c_size_t, _P, _P, _P, _P]),
    # float32 mask stack -> crack-contour counts [N, C, 2]; -> per-contour table, vertex lists and labels (csrc/contours.hip)
    'octseg_stack_contour_counts': (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P]),
    'octseg_contours_scratch_bytes': (C.c_size_t, [C.c_int] * 3 + [C.c_longlong]),
    'octseg_stack_contours': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t] + [C.c_longlong] * 3 + [_P] * 5),
    # float32 mask stack -> connected components across the slices (labels, count, the 32 largest with extents, per-slice profile) and the stack
    # filtered by voxel count, rank and slice span (csrc/lesions.hip)
    'octseg_lesions_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_volume_components': (C.c_int, [_P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P, _P, _P, _P]),
    'octseg_volume_cleanup': (C.c_int, [_P] + [C.c_int] * 8 + [_P, C.c_size_t, _P, _P, _P, _P]),
    # two float32 mask stacks -> both sides' ranked lesions, the 33 x 33 table of shared voxels by lesion rank, per-slice |P & T|, |P|, |T|
    # (csrc/match.hip)
    'octseg_match_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_volume_match': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P, _P, _P, _P]),
    # float32 mask stacks -> boundary planes, exact squared distance maps, per (slice, channel pair) counts, keyed distance lists and the
    # minimum with its location (csrc/distance.hip)
    'octseg_distance_scratch_bytes': (C.c_size_t, [C.c_int] * 6),
    'octseg_stack_boundary': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P]),
    'octseg_stack_distance': (C.c_int, [_P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P]),
    'octseg_pair_distance_counts': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 3 + [_P, C.c_size_t, _P, _P, _P]),
    'octseg_pair_distance_keys': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 3 + [_P, C.c_size_t, C.c_longlong, _P, _P, C.c_longlong,
                                            _P, _P]),
    'octseg_pair_distance_min': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 3 + [_P, C.c_size_t, _P, _P]),
    # the same over the volume a channel's slices form, slice_step pixels apart: 6-neighbour boundary, 3-D distance map in bands of rows, per-pair
    # int64 counts, keyed lists and the minimum with its voxel (csrc/distance.hip)
    'octseg_volume_distance_scratch_bytes': (C.c_size_t, [C.c_int] * 7),
    'octseg_volume_boundary': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P]),
    'octseg_volume_distance': (C.c_int, [_P] + [C.c_int] * 6 + [_P, C.c_size_t, _P, _P]),
    'octseg_volume_pair_distance_counts': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 3 + [_P, C.c_size_t, _P, _P, _P]),
    'octseg_volume_pair_distance_keys': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 4 + [_P, C.c_size_t, C.c_longlong, _P, _P,
                                                   C.c_longlong, _P, _P]),
    'octseg_volume_pair_distance_min': (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P]),
    # float32 mask stack -> signed squared distance maps; two of them + a plan of integer weights -> interpolated planes (csrc/distance.hip)
    'octseg_signed_distance_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_stack_signed_distance': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P]),
    'octseg_signed_blend': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_int, _P, C.c_int, _P, _P]),
    # float32 mask stack -> the skeleton of every plane (Guo-Hall thinning, one workgroup per plane) and its census (csrc/skeleton.hip)
    'octseg_skeleton_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_stack_skeleton': (C.c_int, [_P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P, _P]),
    # float32 skeleton stack -> every plane pruned (spurs removed, ends trimmed, vanished components restored) and its census (csrc/prune.hip)
    'octseg_prune_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_stack_prune': (C.c_int, [_P] + [C.c_int] * 7 + [_P, C.c_size_t, _P, _P, _P]),
    # raw volume [S,H,W,C] uint8 | uint16 -> per-slice min / max + uint8 RGB frames; Pillow's 8-bit bicubic resize from tables (csrc/volume.hip)
    'octseg_volume_normalize': (C.c_int, [_P] + [C.c_int] * 6 + [_P, _P, _P]),
    'octseg_resize_pil_u8': (C.c_int, [_P] + [C.c_int] * 4 + [_P, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, C.c_int, _P]),
    # class activation maps: frozen-BatchNorm forward, seeded data-only backward, the map kernels (csrc/cam.hip)
    'octseg_plan_set_frozen_bn': (C.c_int, [_P, C.c_int]),
    'octseg_plan_cam_target': (C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    'octseg_net_backward_seeded': (C.c_int, [_P, _P, _P, _P, _P]),
    'octseg_cam_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
    'octseg_cam_maps': (C.c_int, [C.c_int, _P, _P] + [C.c_int] * 6 + [_P, _P, C.c_float, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_double, _P, _P]),
    'octseg_cam_overlay': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    'octseg_plan_set_loss': (C.c_int, [_P, C.c_int]),
    'octseg_dice_forward': (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    'octseg_net_backward': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_float, _P]),
    'octseg_net_train_step': (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.c_float, _P]),
    'octseg_plan_set_train_graph': (C.c_int, [_P, C.c_int]),
    'octseg_net_backward_sliced': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_int, _P, SLICE_CB, _P]),
    'octseg_optim_step': (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_float, _P]),
    'octseg_set_deterministic': (C.c_int, [C.c_int]),
    'octseg_debug_set_stamp': (C.c_int, [_P]),
    'octseg_debug_set_serial': (C.c_int, [C.c_int]),
    'octseg_conv2d_scratch_bytes': (C.c_size_t, [C.c_int] * 8),
    'octseg_conv2d_forward': (C.c_int, [C.c_int, _P, _P, _P, _P] + [C.c_int] * 10 + [_P, _P]),
    'octseg_conv2d_backward_data': (C.c_int, [C.c_int, _P, _P, _P] + [C.c_int] * 10 + [_P, _P]),
    'octseg_conv2d_backward_weight': (C.c_int, [C.c_int, _P, _P, _P] + [C.c_int] * 10 + [_P]),
    # one conv layer pass with the plan's fused descriptors per call, and its routing queries (csrc/conv_api.cpp; wrappers in convops.py)
    'octseg_conv_layer_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(ConvLayerDesc), _P]),
    'octseg_conv_layer_route': (C.c_int, [C.c_int, C.c_int, C.POINTER(ConvLayerDesc), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'octseg_conv_layer_slab_rows': (C.c_int, [C.c_int, C.POINTER(ConvLayerDesc), C.POINTER(C.c_int)]),
    # one pass of a tied decoder layer per call, with the plan's images and launches (csrc/conv_api.cpp; wrappers in convops.py)
    'octseg_tied_layer_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(ConvLayerDesc), C.c_int, _P]),
    'octseg_tied_layer_route': (C.c_int, [C.c_int, C.c_int, C.POINTER(ConvLayerDesc), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'octseg_tied_layer_scratch_bytes': (C.c_size_t, [C.c_int, C.POINTER(ConvLayerDesc)]),
    'octseg_side_wgs': (C.c_int, []),
    # one stem launch per call: im2col rows, thin.hip's 7x7 forward and weight gradient (csrc/stem_api.cpp; wrappers in convops.py)
    'octseg_stem_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(StemDesc), _P]),
    'octseg_stem_slab_rows': (C.c_int, [C.c_int] * 3),
    # one launcher of the NHWC sweep kernels per call (csrc/sweep_api.cpp; wrappers in sweeps.py)
    'octseg_sweep_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(_P), C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_double), C.c_int, _P]),
    # one launcher of the PAN pyramid / the MAnet position attention per call (csrc/block_api.cpp; wrappers in blockops.py)
    'octseg_fpa_scratch_floats': (C.c_size_t, [C.c_int] * 3),
    'octseg_fpa_gscratch_floats': (C.c_size_t, [C.c_int] * 3),
    'octseg_fpa_uu_offset': (C.c_size_t, [C.c_int] * 3),
    'octseg_fpa_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(FpaDesc), _P]),
    'octseg_pab_op': (C.c_int, [C.c_int, C.c_int, C.POINTER(PabDesc), _P]),
}

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(or `make -C oct_segmentation_amd/csrc`). There is no CPU fallback.')
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(h, name)  # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().octseg_last_error().decode()
        if 'Expected more than 1 value per channel' in msg:   # torch raises ValueError for this one
            raise ValueError(msg)
        raise RuntimeError(f'octseg error {rc}: {msg}')


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
