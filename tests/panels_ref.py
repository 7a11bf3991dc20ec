"""Host restatement of the reference's per-epoch sample strips (log_predict_model_on_epoch, src/models/smp/model.py:208-271) for the panel
tests -- written from the specification, independent of oct_segmentation_amd and of the kernel, and itself pinned against the reference's own
run (tests/golden/epoch_panel.npz, tests/test_panels.py).

Per frame: two [S, S, 3] colour masks start (128, 128, 128), two label maps start 0.  For idy, cl in enumerate(classes), in that order and
later classes overwriting earlier ones: the ground truth is painted where mask[:, :, CLASS_IDS[cl] - 1] == 255 (exactly 255), the prediction
where pred[:, :, idy] == 1; the colour is the class's, the label CLASS_IDS[cl].  The strip is hstack(frame, colour_gt, colour_pred)."""
import numpy as np

CLASS_IDS = {'Lumen': 1, 'Fibrous cap': 2, 'Lipid core': 3, 'Vasa vasorum': 4}
CLASS_COLORS_RGB = {'Lumen': (228, 30, 199), 'Fibrous cap': (123, 171, 226), 'Lipid core': (125, 227, 127), 'Vasa vasorum': (208, 2, 27)}


def nearest_index(src, dst):
    """cv2.resize(..., interpolation=INTER_NEAREST), OpenCV's resizeNN: sx = min(floor(x * (1 / (dst / src))), src - 1), in double."""
    inv = 1.0 / (float(dst) / float(src))
    return np.array([min(int(np.floor(x * inv)), src - 1) for x in range(dst)], dtype=np.int64)


def resize_nearest(mask, size):
    """[Hs, Ws, ch] -> [size, size, ch]."""
    mask = np.asarray(mask)
    return mask[nearest_index(mask.shape[0], size)][:, nearest_index(mask.shape[1], size)]


def paint(mask, pred, classes, bgr=False):
    """mask: uint8 [S, S, ch] raw ground-truth samples at panel size; pred: [S, S, len(classes)] of 0 / 1.
    Returns colour_gt, colour_pred (uint8 [S, S, 3], RGB unless bgr) and label_pred, label_gt (uint8 [S, S])."""
    mask, pred = np.asarray(mask), np.asarray(pred)
    s = mask.shape[:2]
    color_gt = np.full(s + (3,), 128, np.uint8)
    color_pred = np.full(s + (3,), 128, np.uint8)
    label_pred, label_gt = np.zeros(s, np.uint8), np.zeros(s, np.uint8)
    for idy, cl in enumerate(classes):
        col = CLASS_COLORS_RGB[cl][::-1] if bgr else CLASS_COLORS_RGB[cl]
        g = mask[:, :, CLASS_IDS[cl] - 1] == 255
        p = pred[:, :, idy] == 1
        color_gt[g] = col
        color_pred[p] = col
        label_gt[g] = CLASS_IDS[cl]
        label_pred[p] = CLASS_IDS[cl]
    return color_gt, color_pred, label_pred, label_gt


def panel(frame_bgr, mask, pred, classes):
    """The strip as an RGB array -- what the PNG cv2.imwrite makes of the reference's BGR `res` decodes to -- and labels [2, S, S]
    (0: prediction, 1: ground truth).  frame_bgr: uint8 [S, S, 3]; mask already at panel size."""
    color_gt, color_pred, label_pred, label_gt = paint(mask, pred, classes)
    rgb = np.ascontiguousarray(np.asarray(frame_bgr)[:, :, ::-1])
    return np.hstack((rgb, color_gt, color_pred)), np.stack([label_pred, label_gt])


def panels(frames_bgr, masks, preds, classes, size=None):
    """Batch form; masks at any size are nearest-resized to `size` (default: the frames')."""
    out, labs = [], []
    for f, m, p in zip(frames_bgr, masks, preds):
        s = f.shape[0] if size is None else size
        a, b = panel(f, resize_nearest(m, s), p, classes)
        out.append(a)
        labs.append(b)
    return np.stack(out), np.stack(labs)
