"""The host half of the training augmentation against the reference's own results (tests/golden/augment.npz,
tests/golden/gen_golden_augment.py): yolo355.augment.draw gives the reference's boxes, labels and image shape and consumes
exactly its draws; tests/augment_ref.py's pixel restatement, driven by draw's parameters, gives its images bit for bit.  And the
surface of the companion library: header, exports and ctypes signatures agree, the header is C99, y355_augment_check refuses
what it should before any HIP call, the other libraries' error texts stay their own, the host check builds and passes under the
sanitizers as a stand-alone program.  No GPU."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import augment_cases as AC
import augment_ref as R
from yolo355 import _ffi, augment as A

ROOT = AC.ROOT
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")
COVER = (["brightness", "no_brightness", "contrast_first", "contrast_last", "contrast", "no_contrast", "saturation", "no_saturation", "hue",
          "no_hue", "hue_above_360", "hue_below_0", "expand", "no_expand", "aspect", "centre", "dropped", "kept", "mirror", "no_mirror",
          "neg_origin", "fill_in_window"] + ["mode%d" % m for m in range(6)])


@pytest.fixture(scope="module")
def gold():
    return AC.load_golden()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_golden_covers_every_branch(gold):
    have = set()
    for tag, _, _, _ in AC.samples(gold):
        have |= set(gold[tag + "/tags"].tolist())
    assert set(COVER) <= have, set(COVER) - have
    assert {int(s) for s in gold["ids"][:, 2]} == {0, 1} and {int(s) for s in gold["ids"][:, 0]} == {0, 1, 2, 3}     # both sizes, every frame shape
    assert os.path.getsize(AC.GOLDEN) < 128 * 1024


def test_draw_equals_the_reference(gold):
    for tag, shape, seed, si in AC.samples(gold):
        frame, tgt = AC.frame(shape, seed), AC.target(shape, seed)
        before = tgt.copy()
        np.random.seed(seed)
        p, boxes, labels = A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4])
        assert int(np.random.randint(1 << 30)) == int(gold[tag + "/next"][0]), (tag, "the draws consumed")
        want = gold[tag + "/target"]
        assert boxes.dtype == np.float64 and bits(boxes) == bits(want[:, :4]) and bits(labels.astype(np.float64)) == bits(want[:, 4]), tag
        assert (p.vh, p.vw) == tuple(gold[tag + "/shape"]), tag
        assert bits(tgt) == bits(before), "the inputs are left as they are"
        assert not np.shares_memory(boxes, tgt) and not np.shares_memory(labels, tgt)
        assert p.hsv and p.fill == AC.MEAN
        # a RandomState of the same seed is the same stream, and leaves the global one alone
        np.random.seed(12345)
        p2, b2, l2 = A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4], rng=np.random.RandomState(seed))
        assert repr(p2) == repr(p) and bits(b2) == bits(boxes) and bits(l2) == bits(labels)
        np.random.seed(12345)
        a = np.random.randint(1 << 30)
        np.random.seed(12345)
        A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4], rng=np.random.RandomState(seed))
        assert np.random.randint(1 << 30) == a


def test_restated_pixels_equal_the_reference(gold):
    """pins the composition order, the fill, the absence of clipping and the fp32 scalar rounding"""
    below = above = False
    for tag, shape, seed, si in AC.samples(gold):
        frame, tgt = AC.frame(shape, seed), AC.target(shape, seed)
        np.random.seed(seed)
        p, _, _ = A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4])
        got = R.pixels(frame, p, AC.SIZES[si], AC.MEAN, AC.STD)
        want = gold[tag + "/image"]
        assert got.dtype == np.float32 and got.shape == want.shape == AC.SIZES[si] + (3,)
        assert bits(got) == bits(want), (tag, np.abs(got - want).max())
        raw = want * np.array(AC.STD, np.float32) + np.array(AC.MEAN, np.float32)
        below, above = below or (raw < -1e-3).any(), above or (raw > 1 + 1e-3).any()
    assert below and above, "nothing is clipped: values leave 0..255"


def test_samples_draw_in_list_order_from_one_stream(gold):
    ids = [(s, seed) for _, s, seed, _ in AC.samples(gold)]
    sizes = [AC.frame(s, seed).shape[:2] for s, seed in ids]
    targets = [AC.target(s, seed) for s, seed in ids]
    np.random.seed(7)
    params, out = A.draw_list(sizes, targets)
    rs = np.random.RandomState(7)
    for i, ((hh, ww), t) in enumerate(zip(sizes, targets)):
        p, b, l = A.draw(hh, ww, t[:, :4], t[:, 4], rng=rs)
        assert repr(p) == repr(params[i]) and bits(np.hstack((b, l[:, None]))) == bits(out[i]) and out[i].shape[1] == 5
    assert len({repr(p) for p in params}) > 1
    with pytest.raises(ValueError, match="target arrays"):
        A.draw_list(sizes, targets[:-1])
    with pytest.raises(ValueError, match=r"targets\[0\]"):
        A.draw_list(sizes[:1], [np.zeros((2, 4))])


def test_an_empty_window_raises_and_names_the_sample():
    t = AC.target(0, 0)
    with pytest.raises(ValueError, match="sample 3: the draws give an empty image"):
        A.draw(0, 7, t[:, :4], t[:, 4], rng=np.random.RandomState(5), index=3)          # seed 5: no expand, no crop
    with pytest.raises(ValueError, match="sample 1: 3 boxes, 2 labels"):
        A.draw(5, 7, t[:, :4], t[:2, 4], index=1)
    # no boxes: fine as long as no crop is tried, the reference's failure (overlap.min() of nothing) when one is
    seen = set()
    for seed in range(40):
        try:
            p, b, l = A.draw(5, 7, np.zeros((0, 4)), np.zeros(0), rng=np.random.RandomState(seed))
            assert b.shape == (0, 4) and l.shape == (0,)
            seen.add("passed")
        except ValueError as e:
            assert "no boxes" in str(e)
            seen.add("refused")
    assert seen == {"passed", "refused"}


def test_resize_restatement_special_cases():
    rs = np.random.RandomState(3)
    img = (rs.uniform(-40, 300, (8, 12, 3))).astype(np.float32)
    assert bits(R.resize(img, (12, 8))) == bits(img)                                     # equal sizes: a copy
    half = R.resize(img, (6, 4))                                                         # exact 2x: the area path
    want = (np.float32(0) + (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2])) * np.float32(0.25)
    assert half.shape == (4, 6, 3) and bits(half) == bits(want)
    lin = R.linear_tables(12, 6)                                                         # what the bilinear tables would have given
    assert (lin[3] == 0.5).all() and np.array_equal(lin[0], np.arange(0, 12, 2))
    up = R.resize(img, (30, 5))                                                          # (w, h) = (30, 5): the H / W order
    assert up.shape == (5, 30, 3)
    x0, x1, a0, a1, single = R.linear_tables(12, 30)
    assert single[-1] and not single[0] and (x0[single] == 11).all() and (a1[single] == 0).all() and x0[0] == 0 and a1[0] == 0   # clamped and zeroed at both borders
    y0, y1, b0, b1, _ = R.linear_tables(8, 5, vertical=True)
    assert (y0 >= 0).all() and (y1 <= 7).all()
    one = R.resize(img[:1, :1], (64, 32))                                                # 1x1: the one pixel alone horizontally, blended
    assert one.shape == (32, 64, 3) and (one == one[:, :1]).all()                        # with itself vertically (two rounded products)
    assert (np.abs(one - img[0, 0]) <= np.spacing(np.abs(img[0, 0]))).all() and (one != img[0, 0]).any()
    # identity parameters at equal size: ((frame / 255) - mean) / std
    f = AC.frame(0, 1)
    got = R.pixels(f, A.AugParams.identity(37, 53), (37, 53), AC.MEAN, AC.STD)
    want = ((f.astype(np.float32) / np.float32(255)) - np.array(AC.MEAN, np.float32)) / np.array(AC.STD, np.float32)
    assert bits(got) == bits(want)


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree():
    names = A.declared_symbols()
    assert set(names) == set(A._SIGS) and names == ["y355_augment_abi", "y355_augment_check", "y355_augment_last_error", "y355_augment_run"]
    assert _exports(A.LIB_PATH) == names
    lib = A.lib()
    fb, pb = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.y355_augment_abi(ctypes.byref(fb), ctypes.byref(pb)) == A.chunk() >= 1
    assert (fb.value, pb.value) == (ctypes.sizeof(_ffi.Frame), ctypes.sizeof(A.AugParamsC)) == (24, 48)
    assert A.chunk() * 80 + 128 <= 4096                                                   # the descriptors fit the kernel-argument limit
    text = open(A.HEADER_PATH).read()
    import re
    for name, val in (("BRIGHTNESS", A.F_BRIGHTNESS), ("CONTRAST", A.F_CONTRAST), ("CONTRAST_FIRST", A.F_CONTRAST_FIRST), ("SATURATION", A.F_SATURATION),
                      ("HUE", A.F_HUE), ("MIRROR", A.F_MIRROR), ("HSV", A.F_HSV)):
        assert int(re.search(r"#define Y355_AUG_%s (\d+)" % name, text).group(1)) == val
    for name, val in (("OK", 0), ("EINVAL", _ffi.EINVAL), ("EHIP", _ffi.EHIP), ("ENOTREADY", _ffi.ENOTREADY)):
        assert int(re.search(r"#define Y355_AUGMENT_%s \(?(-?\d+)\)?" % name, text).group(1)) == val


def test_a_library_with_other_structs_is_refused(monkeypatch):
    class Other(ctypes.Structure):
        _fields_ = A.AugParamsC._fields_ + [("more", ctypes.c_int32)]
    monkeypatch.setattr(A, "AugParamsC", Other)
    with pytest.raises(ImportError, match="rebuild"):
        A.lib()


def test_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_augment.h"\nint main(void) {\n  y355_augment_params p;\n  y355_augment_frame f;\n  p.flags = Y355_AUG_ALL_FLAGS;\n'
                   "  f.height = 1;\n  return p.flags == 127 && f.height == 1 && sizeof(p) == 48 && sizeof(f) == 24 ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_other_libraries_know_nothing_of_it():
    from yolo355 import anchors, loss
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH):
        assert not [n for n in _exports(path) if "augment" in n]
    assert not [n for n in _ffi._SIGS if "augment" in n] and "augment" not in open(_ffi.HEADER_PATH).read().lower()
    assert not [n for n in _exports(A.LIB_PATH) if not n.startswith("y355_augment_")]


def _frames(*hw, pitch=None):
    arr = (_ffi.Frame * len(hw))()
    for i, (h, w) in enumerate(hw):
        arr[i].data_dev, arr[i].height, arr[i].width, arr[i].row_bytes = 4096 + i, h, w, 0      # never dereferenced by the check
    if pitch is not None:
        arr[len(hw) - 1].row_bytes = pitch
    return arr


def _refused(text, frames, params, size=(32, 64), mean=AC.MEAN, std=AC.STD):
    with pytest.raises(_ffi.Y355Error) as e:
        A.check_params(frames, params, size, mean, std)
    assert e.value.code == _ffi.EINVAL and text in str(e.value), (text, str(e.value))
    assert A.lib().y355_augment_last_error().decode() in str(e.value)


def test_check_answers_as_specified():
    ok = lambda: [A.AugParams.identity(1, 1), A.AugParams(70, 50, oy=-5, ox=12, mirror=True, hsv=True, hue=3.0, hue_on=True)]
    fr = _frames((1, 1), (64, 48))
    assert A.check_params(fr, ok(), (32, 64)) == 0
    assert A.check_params(_frames((1, 1), (64, 48), pitch=144), ok(), (32, 64)) == 0
    assert A.check_params(_frames((1, 1), (64, 48), pitch=200), ok(), (16384, 1)) == 0
    lib = A.lib()
    assert lib.y355_augment_check(None, None, 1, 32, 64, None, None) == -1 and b"null argument" in lib.y355_augment_last_error()
    _refused("null argument", fr, ok(), mean=None)
    _refused("null argument", fr, ok(), std=None)
    _refused("n must be >= 1", fr, [])
    _refused("dst_h and dst_w must be 1..16384", fr, ok(), size=(0, 64))
    _refused("dst_h and dst_w must be 1..16384", fr, ok(), size=(32, 16385))
    _refused("std must be finite and non-zero", fr, ok(), std=(0.225, 0.0, 0.229))
    _refused("std must be finite and non-zero", fr, ok(), std=(0.225, 0.224, float("inf")))
    _refused("mean must be finite", fr, ok(), mean=(float("nan"), 0.456, 0.485))
    bad = _frames((1, 1), (64, 48))
    bad[1].data_dev = None
    _refused("frame 1: null frame pointer", bad, ok())
    _refused("frame 0: height and width must be 1..16384", _frames((0, 1), (64, 48)), ok())
    _refused("frame 1: height and width must be 1..16384", _frames((1, 1), (64, 16385)), ok())
    _refused("frame 1: row_bytes below width * 3", _frames((1, 1), (64, 48), pitch=143), ok())

    def changed(i, **kw):
        ps = ok()
        for k, v in kw.items():
            setattr(ps[i], k, v)
        return ps
    _refused("frame 0: vh and vw must be 1..16384", fr, changed(0, vh=0))
    _refused("frame 1: vh and vw must be 1..16384", fr, changed(1, vw=16385))
    _refused("frame 1: oy and ox must be within +-2^24", fr, changed(1, oy=-(1 << 24) - 1))
    _refused("frame 0: brightness, contrast, saturation and hue must be finite", fr, changed(0, contrast=float("inf")))
    _refused("frame 1: brightness, contrast, saturation and hue must be finite", fr, changed(1, hue=float("nan")))
    _refused("frame 1: fill must be finite", fr, changed(1, fill=(0.4, float("nan"), 0.4)))
    arr = A._params_array(ok(), 2)
    arr[0].flags = 128
    m, s = (ctypes.c_float * 3)(*AC.MEAN), (ctypes.c_float * 3)(*AC.STD)
    assert lib.y355_augment_check(fr, arr, 2, 32, 64, m, s) == -1 and lib.y355_augment_last_error() == b"frame 0: unknown flags"
    # run makes the same checks first, and its own two, before any HIP call
    assert lib.y355_augment_run(0, fr, arr, 2, 32, 64, m, s, 1, 4096, None) == -1 and lib.y355_augment_last_error() == b"frame 0: unknown flags"
    arr[0].flags = 0
    assert lib.y355_augment_run(-1, fr, arr, 2, 32, 64, m, s, 1, 4096, None) == -1 and lib.y355_augment_last_error() == b"device_id < 0"
    assert lib.y355_augment_run(0, fr, arr, 2, 32, 64, m, s, 1, None, None) == -1 and lib.y355_augment_last_error() == b"y355_augment_run: null destination"


_CHILD = r"""
import ctypes as C, sys
main, loss, anchors, augment = (C.CDLL(p, mode=C.RTLD_GLOBAL) for p in sys.argv[1:5])      # the main library first: its symbols lead the global scope
errs = []
for lib, name in ((main, "y355_last_error"), (loss, "y355_loss_last_error"), (anchors, "y355_anchors_last_error"), (augment, "y355_augment_last_error")):
    getattr(lib, name).restype = C.c_char_p
    errs.append(getattr(lib, name))
text = lambda: [e().decode() for e in errs]
assert text() == ["", "", "", ""], text()
assert augment.y355_augment_check(None, None, 1, 32, 64, None, None) == -1
assert text() == ["", "", "", "y355_augment: null argument"], text()
assert loss.y355_loss_create(None, None) == -1 and anchors.y355_anchors_create(0, 10, 1, 4, None) == -1 and main.y355_apeval_create(0, 3, 2, 8, None) == -1
assert text() == ["null argument", "y355_loss_create: null argument", "y355_anchors_create: null out", "y355_augment: null argument"], text()
assert augment.y355_augment_run(-1, None, None, 0, 0, 0, None, None, 0, None, None) == -1
assert text() == ["null argument", "y355_loss_create: null argument", "y355_anchors_create: null out", "y355_augment: null argument"], text()
print("apart")
"""


def test_error_state_stays_per_library():
    """a fresh process with all four libraries in its global scope: a refused call here leaves the other three texts untouched,
    and theirs leave this one's"""
    from yolo355 import anchors, loss
    r = subprocess.run([sys.executable, "-c", _CHILD, _ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, A.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "apart", r.stdout + r.stderr


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-augment: tests/augment_host_check.cpp, a stand-alone program, with the library's host code and the
    table expressions under -fsanitize=address,undefined"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-augment", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "augment_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "augment_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line


def test_python_side_without_a_gpu():
    import torch
    from yolo355.utils.augmentations import SSDAugmentation
    aug = SSDAugmentation([32, 64])
    assert (aug.size, tuple(aug.mean), tuple(aug.std)) == ([32, 64], AC.MEAN, AC.STD)
    f, t = AC.frame(2, 0), AC.target(2, 0)
    with pytest.raises(ValueError, match="uint8"):
        A.apply([f.astype(np.float32)], [A.AugParams.identity(5, 7)], (32, 64))
    with pytest.raises(ValueError, match="AugParams"):
        A.apply([f], [], (32, 64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            A.apply([f], [A.AugParams.identity(5, 7)], (32, 64))
        with pytest.raises(RuntimeError):
            A.augment_frame_list([f], [t], (32, 64), rng=np.random.RandomState(0))
        with pytest.raises(RuntimeError):
            aug(f, t[:, :4], t[:, 4])
