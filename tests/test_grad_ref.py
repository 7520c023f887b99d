"""The host restatement of the losses' gradient (tests/grad_ref.py) against the reference's own backward()
(tests/golden/grad.npz, tests/golden/gen_golden_grad.py) and against torch's float64 autograd of a restated loss; and the
surface of the companion library libyolo355_grad.so: header, exports and ctypes signatures agree, the header is C99 and
C++11, the other libraries know nothing of it, arguments are refused before any HIP call, the host check builds and passes
under the sanitizers as a stand-alone program.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import grad_ref as GR
import loss_cases as LC
import loss_ref as R
from yolo355 import _ffi, grad as G
from yolo355.tools.grad_bench import torch_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")
SMALL = [c for c in LC.LOSS_CASES if c[1] != "m3_416"]
RUNS = {"total": (0.0, 0.0, 0.0, 1.0), "mix": (1.0, 2.0, 0.0, 0.0)}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "grad.npz")) as z:
        return {k: z[k] for k in z.files}


def case_inputs(tag):
    """(geometry tag, C, labels, maps) of a LOSS_CASES entry or of "nan" """
    if tag == "nan":
        return ("t64", 2) + LC.nan_case()
    _, g, C, _ = next(c for c in LC.LOSS_CASES if c[0] == tag)
    return g, C, LC.loss_labels(tag), LC.loss_pred_maps(tag)


def restated(tag, upstream):
    g, C, labels, maps = case_inputs(tag)
    size, strides, anchors = LC.GEOM[g]
    target = R.make_targets(size, strides, labels, anchors, LC.is_multi(g))
    return GR.map_grads(maps, target, strides, anchors, C, size, LC.wh_mul(g), upstream), LC.num_anchors(g), C


def golden_maps(gold, tag, run):
    n = len([k for k in gold if k.startswith("grad/%s/%s/" % (tag, run))]) - 1
    return [gold["grad/%s/%s/%d" % (tag, run, l)] for l in range(n)], gold["grad/%s/%s/gap" % (tag, run)]


@pytest.mark.parametrize("run", sorted(RUNS))
@pytest.mark.parametrize("tag", [c[0] for c in SMALL] + ["nan"])
def test_restated_gradient_equals_the_reference(gold, tag, run):
    mine, A, C = restated(tag, RUNS[run])
    want, gap = golden_maps(gold, tag, run)
    assert len(mine) == len(want)
    GR.assert_maps(mine, want, gap, A, C, "%s %s" % (tag, run))


def test_golden_is_a_small_fixture_and_the_nan_case_is_what_it_is_meant_to_be(gold):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "grad.npz")) < 256 * 1024
    (m,), _ = golden_maps(gold, "nan", "total")
    A, C = 5, 2
    assert np.isnan(m).sum() == 1 and np.isnan(m[0, 0, 0, 0])                 # d conf of anchor 0 of cell 0: 0 * nan
    box = m[0, A * (1 + C):A * (1 + C) + 4, 0, 0]
    assert np.isfinite(box).all() and (box == 0).all()                        # d tw = 2 * 127 * 0 * 0 stays finite
    for tag, _, _, _ in SMALL:                                                # the second run leaves the box group alone
        maps, _ = golden_maps(gold, tag, "mix")
        assert all((mm[:, -4 * LC.num_anchors(tag.split("_")[0]):] == 0).all() for mm in maps)


@pytest.mark.parametrize("tag", ["t64_c2_b5", "m3_c20_b5", "nan"])
def test_restated_gradient_equals_float64_autograd(tag):
    """torch CPU float64 autograd of a restated loss on the flat tensors, every upstream at once: 1e-12 relative per element
    (both sides are float64 evaluations of the same formulas: a few 1e-16 relative each, and no cancellation beyond
    softmax - onehot on logits within [-2, 2]); exact zeros and the NaN where the restatement has them."""
    g, C, labels, maps = case_inputs(tag)
    size, strides, anchors = LC.GEOM[g]
    target = R.make_targets(size, strides, labels, anchors, LC.is_multi(g))
    conf, cls, box, label = GR.label_of(maps, target, strides, anchors, C, size, LC.wh_mul(g))
    up = (0.25, -1.5, 3.0, 0.75)
    mine = GR.flat_grads(conf, cls, box, label, C, up)
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (conf[..., None], cls, box)]
    out = torch_loss(t[0], t[1], t[2], torch.tensor(np.asarray(label, np.float64)), C)
    sum(u * o for u, o in zip(up, out)).backward()
    for name, a, b in zip(GR.GROUPS, mine, (t[0].grad.numpy()[..., 0], t[1].grad.numpy(), t[2].grad.numpy())):
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        ok = ~np.isnan(b)
        err = np.abs(a - b)[ok]
        print(tag, name, "max rel err %.3g" % (err / np.maximum(np.abs(b[ok]), 1e-300)).max())
        assert (err <= 1e-12 * np.abs(b[ok])).all(), name
    assert np.isnan(mine[0]).sum() == (1 if tag == "nan" else 0)


def test_map_layout_round_trip():
    maps = LC.loss_pred_maps("m3_c20_b5")
    conf, cls, box = R.split_pred(maps, 3, 20)
    back = GR.to_maps(conf, cls, box, [m.shape[2:] for m in maps], 3, 20)
    assert all(np.array_equal(a, b) for a, b in zip(back, maps))


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree():
    names = G.declared_symbols()
    assert set(names) == set(G._SIGS)
    assert names == ["y355_grad_backward", "y355_grad_create", "y355_grad_destroy", "y355_grad_flat", "y355_grad_forward_backward",
                     "y355_grad_last_error", "y355_grad_num_anchors_total", "y355_grad_set_labels", "y355_grad_targets_dev"]
    assert _exports(G.LIB_PATH) == names
    lib = G.lib()
    for n in names:
        assert hasattr(lib, n)
    text = open(G.HEADER_PATH).read()
    for name, val in (("OK", 0), ("EINVAL", _ffi.EINVAL), ("EHIP", _ffi.EHIP), ("ENOTREADY", _ffi.ENOTREADY)):
        assert int(re.search(r"#define Y355_GRAD_%s \(?(-?\d+)\)?" % name, text).group(1)) == val
    # number and order of the C parameters against the ctypes signatures
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in names:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % n, flat).group(1).strip()
        count = 0 if params == "void" else len(params.split(","))
        assert count == len(G._SIGS[n][1]), n


def test_header_is_c99_and_cxx11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_grad.h"\nint main(void) {\n  y355_loss_config c;\n  y355_grad *h = 0;\n  c.num_levels = Y355_LOSS_MAX_LEVELS;\n'
                   "  return c.num_levels == 3 && h == 0 && Y355_GRAD_ENOTREADY == Y355_LOSS_ENOTREADY ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_other_libraries_know_nothing_of_it():
    from yolo355 import anchors, augment, loss
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, augment.LIB_PATH):
        assert not [n for n in _exports(path) if n.startswith("y355_grad_")]
    for sigs in (_ffi._SIGS, loss._SIGS, anchors._SIGS, augment._SIGS):
        assert not [n for n in sigs if n.startswith("y355_grad_")]
    assert not [n for n in _exports(G.LIB_PATH) if not n.startswith("y355_grad_")]
    # it links nothing of them either
    needed = subprocess.run(["readelf", "-d", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libyolo355" not in needed.replace("libyolo355_grad.so", "")


def _cfg(**kw):
    cfg = G.LossConfig()
    cfg.num_levels, cfg.wh_mul, cfg.ignore_thresh, cfg.obj_weight, cfg.noobj_weight, cfg.max_batch, cfg.max_labels_per_image = 1, 1.0, 0.5, 5.0, 1.0, 1, 64
    cfg.hs[0], cfg.ws[0], cfg.stride[0], cfg.num_anchors, cfg.num_classes, cfg.in_h, cfg.in_w = 4, 4, 16, 2, 2, 64, 64
    for i in range(4):
        cfg.anchors[i] = 1.5
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("bad,text", [(dict(num_levels=4), "num_levels must be 1..3"), (dict(num_anchors=17), "num_anchors must be 1..16 per level"),
                                      (dict(num_classes=0), "num_classes must be 1..4096"), (dict(in_w=0), "in_h / in_w must be 1..65536"),
                                      (dict(wh_mul=0.0), "wh_mul must be finite and > 0"), (dict(max_batch=0), "max_batch must be 1..65535"),
                                      (dict(num_levels=2, anchors_in_grid_units=1), "anchors_in_grid_units is gt_creator's form: one level only"),
                                      (dict(ignore_thresh=float("nan")), "ignore_thresh / obj_weight / noobj_weight must be finite"),
                                      (dict(max_labels_per_image=0), "max_labels_per_image must be 1..2^20"), (dict(device_id=-1), "device_id < 0")])
def test_create_refuses_what_the_loss_library_refuses_before_any_hip_call(bad, text):
    from yolo355 import loss as L
    lib, cfg = G.lib(), _cfg(**bad)
    h = ctypes.c_void_p()
    assert lib.y355_grad_create(ctypes.byref(cfg), ctypes.byref(h)) == _ffi.EINVAL and not h.value
    assert lib.y355_grad_last_error().decode() == text
    assert L.lib().y355_loss_create(ctypes.byref(cfg), ctypes.byref(h)) == _ffi.EINVAL and L.lib().y355_loss_last_error().decode() == text


def test_arguments_are_refused_before_any_device_work():
    """the refusals that need no handle (those on a live handle run in the host check, on the host heap)"""
    lib = G.lib()
    err = lambda: lib.y355_grad_last_error().decode()
    w = 4096                                                                  # never dereferenced
    ptrs = (ctypes.c_void_p * 1)(w)
    out = (ctypes.c_double * 4)()
    assert lib.y355_grad_create(None, None) == -1 and err() == "y355_grad_create: null argument"
    assert lib.y355_grad_num_anchors_total(None) == -1 and err() == "null handle"
    assert lib.y355_grad_set_labels(None, None, None, 1) == -1 and err() == "y355_grad_set_labels: null argument"
    assert lib.y355_grad_targets_dev(None, 1, None) == -1 and err() == "y355_grad_targets_dev: null argument"
    assert lib.y355_grad_forward_backward(None, ptrs, None, 1, None, ptrs, None, out, None) == -1 and err() == "y355_grad_forward_backward: null argument"
    assert lib.y355_grad_backward(None, ptrs, None, 1, None, ptrs, None) == -1 and err() == "y355_grad_backward: null argument"
    lib.y355_grad_destroy(None)
    flat = lambda *a: lib.y355_grad_flat(*a)
    assert flat(-1, w, w, w, w, 1, 1, 1, 5.0, 1.0, None, w, w, w, None, out, None) == -1 and err() == "y355_grad_flat: null argument"
    assert flat(0, w, w, None, w, 1, 1, 1, 5.0, 1.0, None, w, w, w, None, out, None) == -1 and err() == "y355_grad_flat: null argument"
    assert flat(0, w, w, w, w, 1, 1, 1, 5.0, 1.0, None, w, None, w, None, out, None) == -1 and err() == "y355_grad_flat: give all three gradient tensors or none"
    assert flat(0, w, w, w, w, 1, 1, 1, 5.0, 1.0, None, None, None, None, None, None, None) == -1 and err() == "y355_grad_flat: neither out nor gradient tensors"
    assert flat(0, w, w, w, w, 0, 1, 1, 5.0, 1.0, None, w, w, w, None, out, None) == -1 and err().startswith("y355_grad_flat: batch must be 1..65535")
    assert flat(0, w, w, w, w, 1, 1, 4097, 5.0, 1.0, None, w, w, w, None, out, None) == -1 and err().startswith("y355_grad_flat: batch must be 1..65535")
    assert flat(0, w, w, w, w, 1, 1, 1, float("inf"), 1.0, None, w, w, w, None, out, None) == -1 and err() == "y355_grad_flat: weights must be finite"


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-grad: tests/grad_host_check.cpp, a stand-alone program, with the library's host code under
    -fsanitize=address,undefined: the create rules, the all-or-none buffers, every refusal on a live handle"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-grad", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "grad_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "grad_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line


def test_python_side_without_a_gpu():
    z = torch.zeros(1, 4, 2)
    with pytest.raises(NotImplementedError, match="only 'mse' is built"):
        G.loss(z[..., :1], z, torch.zeros(1, 4, 4), torch.zeros(1, 4, 8), 2, obj_loss_f="bce")
    with pytest.raises(ValueError, match="CUDA tensor"):
        G.loss(z[..., :1], z, torch.zeros(1, 4, 4), torch.zeros(1, 4, 8), 2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            G.YoloLossGrad([64, 64], 16, LC.GEOM["t64"][2], 2)
        with pytest.raises(RuntimeError):
            G.YoloCriterion([64, 64], 16, LC.GEOM["t64"][2], 2)
