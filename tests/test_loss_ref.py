"""The host restatement of the training targets and losses (tests/loss_ref.py) against the reference's own results
(tests/golden/loss.npz, tests/golden/gen_golden_loss.py), and the surface of the companion library: header, exports and
ctypes signatures agree, libyolo355.so and include/yolo355.h know nothing of it, arguments are refused before any HIP call.
No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_ref as R
from yolo355 import _ffi, loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "loss.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", LC.TARGET_CASES)
def test_restated_targets_equal_the_reference(gold, tag):
    LC.check_case_properties(tag)
    t = LC.restated_targets(tag)
    assert t.shape == gold["tgt/" + tag].shape
    LC.targets_match(t.astype(np.float32), gold["tgt/" + tag])


@pytest.mark.parametrize("case", LC.LOSS_CASES, ids=[c[0] for c in LC.LOSS_CASES])
def test_restated_losses_equal_the_reference(gold, case):
    tag, g, C, B = case
    size, strides, anchors = LC.GEOM[g]
    target = R.make_targets(size, strides, LC.loss_labels(tag), anchors, LC.is_multi(g))
    out, parts = R.loss(LC.loss_pred_maps(tag), target, strides, anchors, C, size, LC.wh_mul(g))
    assert parts.shape == (B, 5) and (target[..., 0] == 1).any()
    LC.assert_losses(out, gold["loss/%s/out" % tag], gold["loss/%s/gap" % tag], tag)


def test_restated_nan_case(gold):
    labels, maps = LC.nan_case()
    size, strides, anchors = LC.GEOM["t64"]
    target = R.make_targets(size, strides, labels, anchors, False)
    assert target[0, 0, 0] == 0                                   # the poisoned anchor is an unassigned (masked) one
    out, _ = R.loss(maps, target, strides, anchors, 2, size, 16.0)
    assert np.isnan(out[[0, 3]]).all() and np.isfinite(out[[1, 2]]).all()
    LC.assert_losses(out, gold["loss/nan/out"], gold["loss/nan/gap"], "nan")


def test_restated_qbf_losses(gold):
    """the reference model's own loss branch, restated on the prediction map it produced"""
    cfg = LC.QBF
    for it in range(2):
        pred = gold["qbf/%d/pred_q" % it].astype(np.float32) * np.float32(2.0 ** -int(gold["qbf/%d/sa_pred" % it][0]))
        target = R.make_targets(cfg["size"], 16, LC.qbf_labels(it), LC.GEOM["t64"][2], False)
        out, _ = R.loss([pred], target, 16, LC.GEOM["t64"][2], cfg["classes"], cfg["size"], 16.0)
        LC.assert_losses(out, gold["qbf/%d/out" % it], gold["qbf/%d/gap" % it], "qbf %d" % it)


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree(tmp_path):
    names = L.declared_symbols()
    assert set(names) == set(L._SIGS) and "y355_loss_compute" in names
    assert _exports(L.LIB_PATH) == names
    lib = L.lib()
    for n in names:
        assert hasattr(lib, n)
    # the configuration structure: size and every field's offset as a C compiler lays them out
    fields = [f[0] for f in L.LossConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yolo355_loss.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(y355_loss_config));\n' +
                   "".join('  printf(" %%zu", offsetof(y355_loss_config, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(L.LossConfig)] + [getattr(L.LossConfig, f).offset for f in fields]
    assert (L.MAX_LEVELS, L.MAX_ANCHORS, L.TARGET_FIELDS) == tuple(
        int(re.search(r"#define Y355_LOSS_%s (\d+)" % n, open(L.HEADER_PATH).read()).group(1)) for n in ("MAX_LEVELS", "MAX_ANCHORS", "TARGET_FIELDS"))


def test_the_main_library_knows_nothing_of_it():
    assert not [n for n in _exports(_ffi.LIB_PATH) if "loss" in n]
    assert not [n for n in _ffi._SIGS if "loss" in n] and not [n for n in _ffi.declared_symbols() if "loss" in n]
    assert "loss" not in open(_ffi.HEADER_PATH).read().lower()


def _cfg(**kw):
    lib = L.lib()
    cfg = L.LossConfig()
    assert lib.y355_loss_default_config(ctypes.byref(cfg)) == 0
    assert (cfg.ignore_thresh, cfg.obj_weight, cfg.noobj_weight, cfg.num_levels, cfg.wh_mul) == (0.5, 5.0, 1.0, 1, 1.0)
    cfg.hs[0], cfg.ws[0], cfg.stride[0], cfg.num_anchors, cfg.num_classes, cfg.in_h, cfg.in_w = 4, 4, 16, 2, 2, 64, 64
    for i in range(4):
        cfg.anchors[i] = 1.5
    for k, v in kw.items():
        setattr(cfg, k, v)
    return lib, cfg


@pytest.mark.parametrize("bad,text", [(dict(num_levels=4), "num_levels"), (dict(num_anchors=17), "num_anchors"), (dict(num_classes=0), "num_classes"),
                                      (dict(in_w=0), "in_h / in_w"), (dict(wh_mul=0.0), "wh_mul"), (dict(max_batch=0), "max_batch"),
                                      (dict(num_levels=2, anchors_in_grid_units=1), "one level"), (dict(ignore_thresh=float("nan")), "finite"),
                                      (dict(max_labels_per_image=0), "max_labels_per_image"), (dict(device_id=-1), "device_id")])
def test_create_refuses_bad_configurations_before_any_hip_call(bad, text):
    lib, cfg = _cfg(**bad)
    h = ctypes.c_void_p()
    assert lib.y355_loss_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    assert text in lib.y355_loss_last_error().decode()


def test_null_arguments_are_refused():
    lib = L.lib()
    assert lib.y355_loss_create(None, None) == -1
    assert lib.y355_loss_set_labels(None, None, None, 1) == -1
    assert lib.y355_loss_get_targets(None, 1, None) == -1
    assert lib.y355_loss_compute(None, None, None, 1, None, None, None) == -1
    assert lib.y355_loss_flat(0, None, None, None, None, 1, 1, 1, 5.0, 1.0, None, None, None) == -1
    assert lib.y355_loss_iou_score(0, None, None, 4, None, None) == -1
    lib.y355_loss_destroy(None)


def test_python_side_without_a_gpu():
    off, lab = L.pack_labels([[[0.1, 0.2, 0.3, 0.4, 1]], [], [[0, 0, 1, 1, 0], [0.5, 0.5, 0.6, 0.6, 1]]])
    assert off.tolist() == [0, 1, 1, 3] and lab.shape == (3, 5) and lab.dtype == np.float64
    z = torch.zeros(1, 4, 2)
    with pytest.raises(NotImplementedError):
        L.loss(z[..., :1], z, torch.zeros(1, 4, 4), torch.zeros(1, 4, 8), 2, obj_loss_f="bce")
    from yolo355 import tools
    assert tools.gt_creator is L.gt_creator and tools.multi_gt_creator is L.multi_gt_creator and tools.loss is L.loss and tools.iou_score is L.iou_score
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            L.gt_creator([64, 64], 16, [[[0.1, 0.1, 0.5, 0.5, 0]]], LC.GEOM["t64"][2])
        with pytest.raises(ValueError):
            L.iou_score(torch.zeros(2, 4), torch.zeros(2, 4))


def test_models_accept_trainable_and_keep_their_refusals():
    from yolo355 import synth
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2, SlimYOLOv2_quantize_bnfuse
    from yolo355.models.tiny_yolo_v3 import YOLOv3tiny
    from yolo355.models.yolo_v2 import myYOLOv2
    from yolo355.models.yolo_v3 import myYOLOv3, myYOLOv3Spp
    x = torch.zeros(1, 3, 64, 64)
    for cls, anchors in ((SlimYOLOv2_quantize_bnfuse, synth.ANCHOR_SIZE_MASK), (SlimYOLOv2, synth.ANCHOR_SIZE), (YOLOv3tiny, synth.TINY_MULTI_ANCHOR_SIZE),
                         (myYOLOv2, synth.ANCHOR_SIZE), (myYOLOv3, synth.MULTI_ANCHOR_SIZE), (myYOLOv3Spp, synth.MULTI_ANCHOR_SIZE)):
        m = cls("cpu", input_size=[64, 64], num_classes=2, trainable=True, anchor_size=anchors)
        assert m.trainable is True and hasattr(m, "loss_batch")
        m.eval()
        with pytest.raises(NotImplementedError):
            m(x)                                                  # trainable=True without a target: still refused
        if cls is not SlimYOLOv2_quantize_bnfuse:
            m.train()
            with pytest.raises(NotImplementedError):
                m(x, target=torch.zeros(1, 1, 11))                # BatchNorm in training mode: still refused
