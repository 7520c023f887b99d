"""Training batches augmented on the GPU: the reference's SSDAugmentation (utils/augmentations.py:413-431) for a list of uint8
frames of mixed sizes.  draw() replays one sample's random draws in the reference's order on the host (numpy.random's stream,
draw for draw; the whole RandomSampleCrop search, which needs only the frame's size and its boxes) and leaves an AugParams for
the pixels; apply() is the pixel half, one launch per chunk of frames straight to a normalised float32 [B,3,H,W] batch on the
device: ctypes binding of include/yolo355_augment.h (csrc/augment.hip, the companion library libyolo355_augment.so, loaded the
first time pixels are asked for); augment_frame_list() is both.  No CPU path for the pixels: without a GPU they raise.

Kept from the reference on purpose: `random.uniform(width - w)` is uniform(low=width - w, high=1.0); the IoU constraint of a crop
mode never rejects a try (`max_iou < overlap.max()` with max_iou = inf), so a try fails only on its aspect ratio or when no box
centre lies inside -- the modes still differ in nothing but the draws; Expand fills with mean on a 0..255 scale, after the
photometric step; nothing is clipped.  `random.choice(self.sample_options)` (a ValueError under NumPy 2) is the one
randint(0, 6) it was under the NumPy of the reference's time.  Not kept: the reference scales the caller's box array in place."""
import ctypes as C
import os

import numpy as np

from . import _ffi, framelist
from ._handle import _require_gpu

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_augment.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_augment.h"))
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)          # SSDAugmentation's defaults (BGR order)
F_BRIGHTNESS, F_CONTRAST, F_CONTRAST_FIRST, F_SATURATION, F_HUE, F_MIRROR, F_HSV = 1, 2, 4, 8, 16, 32, 64
# RandomSampleCrop.sample_options: None, or (min_iou, max_iou)
SAMPLE_OPTIONS = (None, (0.1, None), (0.3, None), (0.7, None), (0.9, None), (None, None))


class AugParamsC(C.Structure):
    """y355_augment_params"""
    _fields_ = [("flags", C.c_int32), ("brightness", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float), ("hue", C.c_float),
                ("vh", C.c_int32), ("vw", C.c_int32), ("oy", C.c_int32), ("ox", C.c_int32), ("fill", C.c_float * 3)]


P = C.POINTER
_SIGS = {
    "y355_augment_last_error": (C.c_char_p, []),
    "y355_augment_abi": (C.c_int, [P(C.c_int32), P(C.c_int32)]),
    "y355_augment_check": (C.c_int, [P(_ffi.Frame), P(AugParamsC), C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float)]),
    "y355_augment_run": (C.c_int, [C.c_int32, P(_ffi.Frame), P(AugParamsC), C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float), C.c_int32,
                                   C.c_void_p, C.c_void_p]),
}
_lib = None
# libyolo355_augment.so, built with libyolo355.so by `make -C csrc`
_load, check, declared_symbols = _ffi.loader(globals(), "y355_augment_", "extensions first (make -C csrc)")


def lib():
    """the library, refused when its two structs are not this binding's"""
    l = _load()
    fb, pb = C.c_int32(0), C.c_int32(0)
    l.y355_augment_abi(C.byref(fb), C.byref(pb))
    if (fb.value, pb.value) != (C.sizeof(_ffi.Frame), C.sizeof(AugParamsC)):
        raise ImportError("yolo355: %s has structs of %d / %d bytes, this binding %d / %d: rebuild it" %
                          (LIB_PATH, fb.value, pb.value, C.sizeof(_ffi.Frame), C.sizeof(AugParamsC)))
    return l


def chunk():
    """frames of one launch"""
    return int(lib().y355_augment_abi(None, None))


class AugParams:
    """What the pixels of one sample need, as plain numbers: brightness (delta), contrast (alpha) and contrast_first, saturation
    (factor), hue (delta), each with its *_on flag; hsv: the BGR -> HSV -> BGR round trip runs (always after draw(); without it
    and without brightness the photometric step is the identity); the virtual image's size (vh, vw) -- the crop window of the
    expanded canvas, after crop and before mirror and resize; the source's origin inside it (oy, ox), which may be negative;
    mirror; fill (BGR, 0..255 scale).  The draws are kept as drawn (float64); the pixels round them to float32 first."""
    __slots__ = ("brightness", "brightness_on", "contrast", "contrast_on", "contrast_first", "saturation", "saturation_on", "hue", "hue_on",
                 "hsv", "vh", "vw", "oy", "ox", "mirror", "fill")

    def __init__(self, vh, vw, oy=0, ox=0, mirror=False, fill=MEAN, brightness=0.0, brightness_on=False, contrast=1.0, contrast_on=False,
                 contrast_first=False, saturation=1.0, saturation_on=False, hue=0.0, hue_on=False, hsv=False):
        self.vh, self.vw, self.oy, self.ox, self.mirror = int(vh), int(vw), int(oy), int(ox), bool(mirror)
        self.fill = tuple(float(v) for v in fill)
        self.brightness, self.brightness_on = float(brightness), bool(brightness_on)
        self.contrast, self.contrast_on, self.contrast_first = float(contrast), bool(contrast_on), bool(contrast_first)
        self.saturation, self.saturation_on = float(saturation), bool(saturation_on)
        self.hue, self.hue_on, self.hsv = float(hue), bool(hue_on), bool(hsv)

    @classmethod
    def identity(cls, height, width, fill=MEAN):
        """the frame as it is: apply() with these is a float-resize BaseTransform"""
        return cls(height, width, fill=fill)

    def flags(self):
        return (F_BRIGHTNESS * self.brightness_on | F_CONTRAST * self.contrast_on | F_CONTRAST_FIRST * self.contrast_first |
                F_SATURATION * self.saturation_on | F_HUE * self.hue_on | F_MIRROR * self.mirror | F_HSV * self.hsv)

    def fill_c(self, c):
        c.flags = self.flags()
        c.brightness, c.contrast, c.saturation, c.hue = self.brightness, self.contrast, self.saturation, self.hue
        c.vh, c.vw, c.oy, c.ox = self.vh, self.vw, self.oy, self.ox
        c.fill[0], c.fill[1], c.fill[2] = self.fill

    def __repr__(self):
        return "AugParams(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.__slots__)


def _who(index):
    return "sample" if index is None else "sample %s" % (index,)


def draw(height, width, boxes, labels, rng=None, mean=MEAN, index=None, trace=None):
    """One sample's draws in the reference's order -> (AugParams, boxes_out, labels_out).  boxes float64 [n,4] = (xmin, ymin,
    xmax, ymax) in [0,1] on entry and on exit; both outputs are copies, the inputs are left as they are.  rng: a
    numpy.random.RandomState, None: the global one (`np.random.seed(s)` means what it means in the reference).  All host
    arithmetic is float64 / Python ints as in the reference.  A draw that yields an empty virtual image raises ValueError
    naming the sample (`index`).  trace: a list that receives the branches taken (strings), for coverage checks."""
    rs = np.random if rng is None else rng
    note = (lambda s: None) if trace is None else trace.append
    height, width = int(height), int(width)
    boxes = np.array(boxes, dtype=np.float64).reshape(-1, 4)          # a copy
    labels = np.array(labels).reshape(-1)
    if len(labels) != len(boxes):
        raise ValueError("%s: %d boxes, %d labels" % (_who(index), len(boxes), len(labels)))
    p = AugParams(height, width, fill=mean, hsv=True)
    # ToAbsoluteCoords
    boxes[:, 0] *= width
    boxes[:, 2] *= width
    boxes[:, 1] *= height
    boxes[:, 3] *= height
    # PhotometricDistort: brightness, then contrast before or after the HSV part, chosen by one draw
    if rs.randint(2):
        p.brightness_on, p.brightness = True, float(rs.uniform(-32, 32))
    p.contrast_first = bool(rs.randint(2))
    if p.contrast_first and rs.randint(2):
        p.contrast_on, p.contrast = True, float(rs.uniform(0.5, 1.5))
    if rs.randint(2):
        p.saturation_on, p.saturation = True, float(rs.uniform(0.5, 1.5))
    if rs.randint(2):
        p.hue_on, p.hue = True, float(rs.uniform(-18.0, 18.0))
    if not p.contrast_first and rs.randint(2):
        p.contrast_on, p.contrast = True, float(rs.uniform(0.5, 1.5))
    # Expand: the canvas (ch, cw), the source at (ey, ex) in it
    ch, cw, ey, ex = height, width, 0, 0
    if not rs.randint(2):
        ratio = rs.uniform(1, 4)
        left = rs.uniform(0, width * ratio - width)
        top = rs.uniform(0, height * ratio - height)
        ch, cw, ey, ex = int(height * ratio), int(width * ratio), int(top), int(left)
        if int(top + height) - ey != height or int(left + width) - ex != width or ey + height > ch or ex + width > cw:
            raise ValueError("%s: the expanded canvas does not hold the frame (the reference's assignment fails)" % _who(index))
        boxes[:, :2] += (int(left), int(top))
        boxes[:, 2:] += (int(left), int(top))
        note("expand")
    # RandomSampleCrop on the canvas: rect = (x1, y1, x2, y2)
    rect = None
    while True:
        m = int(rs.randint(len(SAMPLE_OPTIONS)))
        note("mode%d" % m)
        if SAMPLE_OPTIONS[m] is None:
            break
        found = False
        for _ in range(50):
            w = rs.uniform(0.3 * cw, cw)
            h = rs.uniform(0.3 * ch, ch)
            if h / w < 0.5 or h / w > 2:
                note("aspect")
                continue
            left = rs.uniform(cw - w)
            top = rs.uniform(ch - h)
            r = np.array([int(left), int(top), int(left + w), int(top + h)])
            if len(boxes) == 0:
                raise ValueError("%s: no boxes (the reference's overlap.min() fails)" % _who(index))
            # (the overlap test `overlap.min() < min_iou and max_iou < overlap.max()` is never true: max_iou is inf)
            centers = (boxes[:, :2] + boxes[:, 2:]) / 2.0
            m1 = (r[0] < centers[:, 0]) * (r[1] < centers[:, 1])
            m2 = (r[2] > centers[:, 0]) * (r[3] > centers[:, 1])
            mask = m1 * m2
            if not mask.any():
                note("centre")
                continue
            note("dropped" if not mask.all() else "kept")
            cur = boxes[mask, :].copy()
            labels = labels[mask]
            cur[:, :2] = np.maximum(cur[:, :2], r[:2])
            cur[:, :2] -= r[:2]
            cur[:, 2:] = np.minimum(cur[:, 2:], r[2:])
            cur[:, 2:] -= r[:2]
            boxes, rect, found = cur, r, True
            break
        if found:
            break
        note("exhausted")
    if rect is None:
        p.vh, p.vw, p.oy, p.ox = ch, cw, ey, ex
    else:                                                             # (a slice: clipped to the canvas)
        x1, y1 = int(rect[0]), int(rect[1])
        p.vh, p.vw = max(min(int(rect[3]), ch) - y1, 0), max(min(int(rect[2]), cw) - x1, 0)
        p.oy, p.ox = ey - y1, ex - x1
    if p.vh < 1 or p.vw < 1:
        raise ValueError("%s: the draws give an empty image (%d x %d): cv2.resize fails in the reference" % (_who(index), p.vh, p.vw))
    # RandomMirror
    if rs.randint(2):
        p.mirror = True
        boxes = boxes.copy()
        boxes[:, 0::2] = p.vw - boxes[:, 2::-2]
    # ToPercentCoords
    boxes[:, 0] /= p.vw
    boxes[:, 2] /= p.vw
    boxes[:, 1] /= p.vh
    boxes[:, 3] /= p.vh
    return p, boxes, labels.copy()


def _split_targets(targets, B):
    if len(targets) != B:
        raise ValueError("%d frames, %d target arrays" % (B, len(targets)))
    out = []
    for i, t in enumerate(targets):
        t = np.asarray(t, np.float64)
        if t.ndim != 2 or t.shape[1] != 5:
            raise ValueError("targets[%d] must be [n,5] = (xmin, ymin, xmax, ymax, cls), got %s" % (i, t.shape))
        out.append((t[:, :4], t[:, 4]))
    return out


def _size(size):
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise ValueError("size must be [H, W] >= 1, got %r" % (size,))
    return H, W


def _params_array(params, B):
    if len(params) != B:
        raise ValueError("%d frames, %d AugParams" % (B, len(params)))
    arr = (AugParamsC * B)()
    for i, p in enumerate(params):
        p.fill_c(arr[i])
    return arr


def apply(frames, params, size, mean=MEAN, std=STD, to_rgb=True, out=None, device=None):
    """The pixel half for given parameters: frames (a list of uint8 [h,w,3] BGR frames; numpy, CPU torch and CUDA frames may
    be mixed, a row-pitched CUDA view passes its pitch) and one AugParams each -> float32 [B,3,H,W] on the device, written on
    the current torch stream (asynchronously); `out` is used when it is given and fits.  to_rgb: channel order R, G, B, as
    the reference's pull_item delivers; False: B, G, R.  mean / std index the image's channels (BGR)."""
    import torch
    sizes = framelist.check_frame_list(frames)
    B = len(frames)
    H, W = _size(size)
    parr = _params_array(params, B)
    l = lib()
    out_ok = out is None or (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, H, W) and
                             out.is_contiguous())
    device = _require_gpu(device if device is not None or out is None or not out_ok else out.device)
    stream = torch.cuda.current_stream(device)
    if out is not None:
        if not out_ok or out.device != device:
            raise ValueError("out must be a contiguous float32 CUDA tensor [%d,3,%d,%d] on %s" % (B, H, W, device))
        x = out
    else:
        with torch.cuda.device(device):
            x = torch.empty((B, 3, H, W), dtype=torch.float32, device=device)
    arr, _, _, held = framelist.frame_list(frames, B, device, stream)
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    check(l.y355_augment_run(device.index, arr, parr, B, H, W, m, s, 1 if to_rgb else 0, x.data_ptr(), stream.cuda_stream))
    del held, sizes                                                   # marked with record_stream / allocated on `stream`: safe to drop
    return x


def check_params(frames_c, params, size, mean=MEAN, std=STD):
    """y355_augment_check on a y355_frame array (framelist / _ffi.Frame) and a list of AugParams: pure host validation"""
    H, W = int(size[0]), int(size[1])
    n = len(params)
    m = None if mean is None else (C.c_float * 3)(*[float(v) for v in mean])
    s = None if std is None else (C.c_float * 3)(*[float(v) for v in std])
    return check(lib().y355_augment_check(frames_c, _params_array(params, n) if n else (AugParamsC * 1)(), n, H, W, m, s))


def draw_list(sizes, targets, rng=None, mean=MEAN):
    """draw() for every sample of a list, in list order from the one stream -> (params, targets_out)"""
    params, targets_out = [], []
    for i, ((hh, ww), (b, lab)) in enumerate(zip(sizes, _split_targets(targets, len(sizes)))):
        p, bo, lo = draw(hh, ww, b, lab, rng=rng, mean=mean, index=i)
        params.append(p)
        targets_out.append(np.hstack((bo, lo[:, None])))
    return params, targets_out


def augment_frame_list(frames, targets, size, rng=None, mean=MEAN, std=STD, to_rgb=True, out=None, device=None):
    """SSDAugmentation(size, mean, std) on every (frame, target) of a list -> (x, targets_out, params): x float32 CUDA
    [B,3,H,W] (see apply), targets_out[i] float64 [m_i,5] = np.hstack((boxes, labels[:, None])) -- the format loss_batch and
    calibrate_with_loss take -- and the AugParams drawn.  targets[i]: float [n_i,5] = (xmin, ymin, xmax, ymax, cls), boxes in
    [0,1].  size = [H, W] is per call (multi-scale training).  The samples draw in list order from the one stream (rng)."""
    sizes = framelist.check_frame_list(frames)
    _size(size)
    params, targets_out = draw_list(sizes, targets, rng=rng, mean=mean)
    return apply(frames, params, size, mean=mean, std=std, to_rgb=to_rgb, out=out, device=device), targets_out, params
