"""NumPy restatement of the pixel half of the reference's SSDAugmentation (utils/augmentations.py), TEST INFRASTRUCTURE ONLY:
the checker of yolo355.augment's kernel, and the `cv2` stand-ins under which tests/golden/gen_golden_augment.py runs the
reference's own module.

Parity status of the two OpenCV calls: UNPINNED, for the reason oracle/resize_oracle.py gives -- OpenCV is a third-party
dependency of the reference that is neither vendored with it nor installed in the build image, and the reference pins no
version, so no golden vector of `cv2` itself can be produced.  `resize` and `cvtColor` below restate the published algorithm of
OpenCV 4.x for CV_32FC3 (scalar code paths; a SIMD build may associate differently):

  cvtColor BGR2HSV (imgproc/src/color_hsv: RGB2HSV_f, hrange 360)
      v = max(b, g, r), vmin = min; diff = v - vmin; s = diff / (|v| + FLT_EPSILON); diff = 60 / (diff + FLT_EPSILON)
      h = (g - b) * diff if v == r else (b - r) * diff + 120 if v == g else (r - g) * diff + 240; h < 0: h += 360
      (the double division of the source rounds to the float quotient: 53 >= 2 * 24 + 2 bits)
  cvtColor HSV2BGR (HSV2RGB_native, hscale = 6.f / 360)
      s == 0: b = g = r = v.  Else h *= hscale; h = fmod(h, 6); sector = floor(h); h -= sector; a sector outside 0..5 -> (0, 0);
      tab = (v, v * (1 - s), v * (1 - s * h), v * (1 - s * (1 - h))); (b, g, r) = tab[sector_data[sector]]
  resize, INTER_LINEAR (imgproc/src/resize.cpp: resizeGeneric, HResizeLinear / VResizeLinear <float>)
      the tables of oracle/resize_oracle.py's linear_tables with the float pair (1 - f, f) as coefficients; horizontally a clamped
      offset zeroes the fraction, and from the first dx with sx >= w - 1 on (xmax) the row value is S[sx] alone; vertically the
      fraction stays and the two row indices are clipped; D = S0 * b0 + S1 * b1 on the horizontally blended rows
      dsize == ssize: the image is copied
      scale 2 on both axes: INTER_LINEAR becomes INTER_AREA's integer-scale path (ResizeAreaFast, scalar for three channels):
      D = (0 + (((S[2y][2x] + S[2y][2x+1]) + S[2y+1][2x]) + S[2y+1][2x+1])) * 0.25f

Everything around the two calls (operation order, fp32 scalar rounding, the fill, no clipping) is pinned to the reference's own
code by tests/golden/augment.npz: pixels() below, driven by yolo355.augment.draw's parameters, equals the images the reference
produced under these stand-ins bit for bit."""
import numpy as np

F = np.float32
EPS = F(1.1920928955078125e-7)
COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54          # cv2's values


def bgr2hsv(img):
    img = np.asarray(img, F)
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.where(r < g, g, r)
    v = np.where(v < b, b, v)
    vmin = np.where(r > g, g, r)
    vmin = np.where(vmin > b, b, vmin)
    with np.errstate(all="ignore"):
        diff = v - vmin
        s = diff / (np.abs(v) + EPS)
        diff = F(60.0) / (diff + EPS)
        h = np.where(v == r, (g - b) * diff, np.where(v == g, (b - r) * diff + F(120.0), (r - g) * diff + F(240.0)))
        h = np.where(h < 0, h + F(360.0), h)
    out = np.stack([h, s, v], axis=-1)
    assert out.dtype == F
    return out


def hsv2bgr(img):
    img = np.asarray(img, F)
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    with np.errstate(all="ignore"):
        h = h * (F(6.0) / F(360.0))
        h = np.fmod(h, F(6.0))
        fl = np.floor(h)
        sector = np.where(np.isfinite(fl), fl, -1).astype(np.int64)
        h = h - fl
        bad = (sector < 0) | (sector >= 6)
        sector = np.where(bad, 0, sector)
        h = np.where(bad, F(0.0), h)
        one = F(1.0)
        tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]        # [..., 3]
    out = np.take_along_axis(tab, sd, axis=-1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    assert out.dtype == F
    return out


def cvtColor(img, code):
    if code == COLOR_BGR2HSV:
        return bgr2hsv(img)
    if code == COLOR_HSV2BGR:
        return hsv2bgr(img)
    raise NotImplementedError(code)


def linear_tables(src, dst, vertical=False):
    """(i0, i1 int64 [dst], c0, c1 float32 [dst], single bool [dst]) of one axis"""
    scale = float(src) / float(dst)
    i0, i1 = np.zeros(dst, np.int64), np.zeros(dst, np.int64)
    c0, c1 = np.zeros(dst, F), np.zeros(dst, F)
    single = np.zeros(dst, bool)
    for d in range(dst):
        f = F((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = F(f - F(s))
        if vertical:
            i0[d], i1[d] = min(max(s, 0), src - 1), min(max(s + 1, 0), src - 1)
        else:
            if s < 0:
                s, f = 0, F(0.0)
            if s >= src - 1:
                s, f, single[d] = src - 1, F(0.0), True
            i0[d], i1[d] = s, s if single[d] else s + 1
        c0[d], c1[d] = F(1.0) - f, f
    return i0, i1, c0, c1, single


def resize(img, dsize):
    """cv2.resize(img, (w, h)) for a float32 [h, w, 3] image"""
    img = np.asarray(img)
    assert img.dtype == F and img.ndim == 3
    W, H = int(dsize[0]), int(dsize[1])
    h, w = img.shape[:2]
    if h < 1 or w < 1:
        raise ValueError("cv2.resize: empty image %s" % (img.shape,))
    if (h, w) == (H, W):
        return img.copy()
    with np.errstate(all="ignore"):
        if (h, w) == (2 * H, 2 * W):
            s = ((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]
            return (F(0.0) + s) * F(0.25)
        x0, x1, a0, a1, single = linear_tables(w, W)
        y0, y1, b0, b1, _ = linear_tables(h, H, vertical=True)
        hz = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
        hz = np.where(single[None, :, None], img[:, x0], hz)
        out = hz[y0] * b0[:, None, None] + hz[y1] * b1[:, None, None]
    assert out.dtype == F
    return out


def photometric(img, p):
    """PhotometricDistort on a float32 image for draw()'s parameters (p.hsv False: brightness alone)"""
    im = np.array(img, F)
    with np.errstate(all="ignore"):
        if p.brightness_on:
            im += F(p.brightness)
        if not p.hsv:
            return im
        if p.contrast_on and p.contrast_first:
            im *= F(p.contrast)
        im = bgr2hsv(im)
        if p.saturation_on:
            im[:, :, 1] *= F(p.saturation)
        if p.hue_on:
            im[:, :, 0] += F(p.hue)
            im[:, :, 0][im[:, :, 0] > 360.0] -= F(360.0)
            im[:, :, 0][im[:, :, 0] < 0.0] += F(360.0)
        im = hsv2bgr(im)
        if p.contrast_on and not p.contrast_first:
            im *= F(p.contrast)
    return im


def virtual_image(frame, p):
    """the float32 [vh, vw, 3] image on entry to cv2.resize: the distorted frame inside the fill, cropped and mirrored"""
    frame = np.asarray(frame)
    im = photometric(frame.astype(F), p)
    sh, sw = frame.shape[:2]
    v = np.empty((p.vh, p.vw, 3), F)
    v[:, :, :] = np.asarray(p.fill, F)
    y0, y1, x0, x1 = max(p.oy, 0), min(p.oy + sh, p.vh), max(p.ox, 0), min(p.ox + sw, p.vw)
    if y1 > y0 and x1 > x0:
        v[y0:y1, x0:x1] = im[y0 - p.oy:y1 - p.oy, x0 - p.ox:x1 - p.ox]
    return v[:, ::-1] if p.mirror else v


def pixels(frame, p, size, mean, std):
    """one sample's float32 [H, W, 3] BGR image as SSDAugmentation returns it"""
    im = resize(virtual_image(frame, p), (size[1], size[0]))
    with np.errstate(all="ignore"):
        im = im.astype(F)
        im /= F(255.0)
        im -= np.array(mean, F)
        im /= np.array(std, F)
    return im


def batch(frames, params, size, mean, std, to_rgb=True):
    """float32 [B, 3, H, W]: what yolo355.augment.apply returns"""
    out = np.stack([pixels(np.asarray(f), p, size, mean, std) for f, p in zip(frames, params)])
    if to_rgb:
        out = out[..., ::-1]
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))
