"""The training targets and losses on the GPU (csrc/loss.hip through yolo355/loss.py and the models' loss branch) against
the host restatement (tests/loss_ref.py) and the reference's own results (tests/golden/loss.npz), at the smallest shapes
that can still go wrong.  Tolerances: targets exact except one fp32 ulp on tw / th (a float64 logarithm of another
library); losses 1e-5 relative against the restatement (fp32 terms that differ by a few ulps in expf / logf, non-negative,
summed in float64) and loss_cases.golden_bound against the goldens."""
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
import loss_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "loss.npz")) as z:
        return {k: z[k] for k in z.files}


def rel_close(got, want, rel=1e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok]
    print("max rel err %.3g" % (err / np.maximum(np.abs(want[ok]), 1e-300)).max() if err.size else "empty")
    assert (err <= rel * np.abs(want[ok])).all(), (got, want)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("tag", LC.TARGET_CASES)
def test_targets(gold, tag):
    from yolo355 import loss as L
    LC.check_case_properties(tag)
    size, strides, anchors = LC.GEOM[tag]
    labels = LC.target_labels(tag)
    want = LC.restated_targets(tag)
    h = L.YoloLoss(size, strides, anchors, 2, max_batch=3, max_labels_per_image=70)
    assert h.num_anchors_total == want.shape[1]
    h.set_labels(labels)
    got = h.targets()
    assert got.dtype == np.float32 and got.shape == want.shape
    LC.targets_match(got, want)
    LC.targets_match(got, gold["tgt/" + tag])
    h.set_labels(labels[2:] + labels[:1])                       # another batch on the same handle: nothing of the last one is left
    got2 = h.targets()
    assert np.array_equal(got2[1], got[0]) and np.array_equal(got2[0], got[2])
    h.close()
    creator = L.multi_gt_creator if LC.is_multi(tag) else L.gt_creator
    assert np.array_equal(creator(size, strides, labels, anchors), got.astype(np.float64))


def test_labels_are_validated_on_the_host():
    from yolo355 import _ffi, loss as L
    size, strides, anchors = LC.GEOM["t64"]
    h = L.YoloLoss(size, strides, anchors, 2, max_batch=2, max_labels_per_image=2)
    for bad in ([[[0.1, 0.1, 1.5, 0.5, 0]]], [[[0.1, 0.1, 0.5, 0.5, 2]]], [[[0.1, float("nan"), 0.5, 0.5, 0]]], [[[-0.1, 0.1, 0.5, 0.5, 0]]],
                [[[0.1, 0.1, 0.5, 0.5, 0]] * 3], [[], [], []]):
        with pytest.raises(_ffi.Y355Error):
            h.set_labels(bad)
    with pytest.raises(_ffi.Y355Error):
        h.compute([np.zeros((1, 35, 4, 4), np.float32)])          # no labels set
    with pytest.raises(ValueError):
        h.compute([np.zeros((1, 35, 4, 5), np.float32)], target=np.zeros((1, 80, 11), np.float32))
    h.close()


# ------------------------------------------------------------------------------------------------------------ loss, operator level
@pytest.mark.parametrize("case", LC.LOSS_CASES, ids=[c[0] for c in LC.LOSS_CASES])
def test_loss_operator(gold, case):
    from yolo355 import loss as L
    tag, g, C, B = case
    size, strides, anchors = LC.GEOM[g]
    labels, maps = LC.loss_labels(tag), LC.loss_pred_maps(tag)
    target = R.make_targets(size, strides, labels, anchors, LC.is_multi(g))
    want, want_parts = R.loss(maps, target, strides, anchors, C, size, LC.wh_mul(g))
    h = L.YoloLoss(size, strides, anchors, C, max_batch=B, max_labels_per_image=16)
    h.set_labels(labels)
    dev_maps = [torch.from_numpy(m).to(h.device) for m in maps]
    out, parts = h.compute(dev_maps)
    rel_close(out, want)
    rel_close(parts, want_parts)
    LC.assert_losses(out, gold["loss/%s/out" % tag], gold["loss/%s/gap" % tag], tag)
    out2, parts2 = h.compute(dev_maps)                            # two runs: the same bits
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(parts), bits(parts2))
    dense = h.targets()
    out3, parts3 = h.compute(dev_maps, target=dense)              # a caller's dense target: the same bits as the handle's own
    assert np.array_equal(bits(out), bits(out3)) and np.array_equal(bits(parts), bits(parts3))
    for i in range(B if B > 1 else 0):                            # an image alone: the parts it has inside the batch
        _, pi = h.compute([m[i:i + 1] for m in dev_maps], target=dense[i:i + 1])
        assert np.array_equal(bits(pi[0]), bits(parts[i])), (i, pi, parts[i])
    # the reference's own signatures: tools.iou_score and tools.loss on flat CUDA tensors
    A = LC.num_anchors(g)
    conf, cls, box = R.split_pred(maps, A, C)
    grids = [m.shape[2:] for m in maps]
    st = [strides] if np.isscalar(strides) else list(strides)
    dec = R.decode(box, grids, st, anchors, LC.wh_mul(g), size)
    t32 = torch.from_numpy(dense).to(h.device)
    iou = L.iou_score(torch.from_numpy(dec).to(h.device).view(-1, 4), t32[:, :, 7:].reshape(-1, 4))
    want_iou = R.iou_score(dec, dense[..., 7:])
    assert np.allclose(iou.cpu().numpy().reshape(want_iou.shape), want_iou, rtol=1e-6, atol=1e-7, equal_nan=True)
    label = torch.cat([iou.view(B, -1, 1), t32[:, :, :7]], dim=2)
    flat = L.loss(torch.from_numpy(conf).to(h.device).unsqueeze(-1), torch.from_numpy(cls).to(h.device), torch.from_numpy(box).to(h.device),
                  label, C)
    assert all(v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda for v in flat)
    rel_close([float(v) for v in flat], want.astype(np.float32), rel=1e-5 + 2.0 ** -23)     # (the drop-in returns float32)
    h.close()


def test_loss_nan_poisons_the_sum_where_the_reference_does(gold):
    from yolo355 import loss as L
    labels, maps = LC.nan_case()
    size, strides, anchors = LC.GEOM["t64"]
    h = L.YoloLoss(size, strides, anchors, 2, max_batch=1)
    h.set_labels(labels)
    assert h.targets()[0, 0, 0] == 0                              # the anchor with inf * 0 is a masked one
    out, parts = h.compute(maps)
    assert np.isnan(out[[0, 3]]).all() and np.isfinite(out[[1, 2]]).all(), out
    assert np.isnan(parts[0, 0]) and np.isfinite(parts[0, 1:]).all(), parts
    LC.assert_losses(out, gold["loss/nan/out"], gold["loss/nan/gap"], "nan")
    h.close()


# ------------------------------------------------------------------------------------------------------------ models
def _qbf_model(trainable=True):
    from yolo355 import prep, synth
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2_quantize_bnfuse
    cfg = LC.QBF
    m = SlimYOLOv2_quantize_bnfuse("cuda:0", input_size=cfg["size"], num_classes=cfg["classes"], trainable=trainable, conf_thresh=0.01,
                                   nms_thresh=0.5, anchor_size=synth.ANCHOR_SIZE_MASK)
    sd = m.state_dict()
    for name, w, b in synth.make_weights(**cfg["weights"], num_classes=cfg["classes"]):
        k = "pred" if name == "pred" else name + ".convs.0"
        for suffix, t in ((".weight", w), (".bias", b)):
            q, e = prep.to_int8_pow2(torch.from_numpy(t))
            sd[k + suffix] = torch.from_numpy(q.astype(np.float32) * np.float32(2.0 ** -e))
    m.load_state_dict(sd, strict=False)
    return m


def test_qbf_model_loss_branch_equals_the_reference(gold):
    """SlimYOLOv2_quantize_bnfuse(trainable=True)(x, target, quantization=True) over two batches: the trackers move as
    calibrate(x, freeze=False) moves them, the int8 prediction map is the reference's bit for bit, the four losses are the
    reference's within the recorded gap x 2 (only the order of the sums differs)."""
    from yolo355 import synth, tools
    cfg = LC.QBF
    m, twin = _qbf_model(), _qbf_model()
    names = [n for n, _ in m.named_buffers() if "a_tracker" in n]
    for it, seed in enumerate(cfg["image_seeds"]):
        x = torch.from_numpy(synth.make_images(seed, cfg["batch"], cfg["size"][0], cfg["size"][1], "blocks"))
        labels = LC.qbf_labels(it)
        dense = torch.tensor(tools.gt_creator(cfg["size"], 16, labels, synth.ANCHOR_SIZE_MASK)).float()
        res = m(x, target=dense, quantization=True)
        assert len(res) == 4 and all(v.dtype == torch.float32 and v.dim() == 0 for v in res)
        sa = twin.calibrate(x, freeze=False)
        bufs, tbufs = dict(m.named_buffers()), dict(twin.named_buffers())
        for n in names:
            assert torch.equal(bufs[n].cpu(), tbufs[n].cpu()), n
        assert sa[10] == int(gold["qbf/%d/sa_pred" % it][0])
        assert np.array_equal(m._engine.get_feature(9, cfg["batch"]), gold["qbf/%d/pred_q" % it])
        scales = np.array([float(bufs["%s.scale" % n]) for n in ["a_tracker_in", "a_tracker1", "a_tracker2", "a_tracker3_1", "a_tracker3_2",
                                                                  "a_tracker4_1", "a_tracker4_2", "a_tracker5", "a_tracker6", "a_tracker7",
                                                                  "a_tracker_pred"]], np.float32)
        assert np.allclose(scales, gold["qbf/%d/scales" % it], rtol=1e-6, atol=0)
        got = np.array([float(v) for v in res], np.float64)
        # the float32 the drop-in returns is the rounding of a float64 within the bound: allow that rounding on top
        want, gap = gold["qbf/%d/out" % it], gold["qbf/%d/gap" % it]
        err = np.abs(got - want.astype(np.float64))
        print("qbf", it, got, "err", err, "bound", LC.golden_bound(want, gap))
        assert (err <= LC.golden_bound(want, gap) + np.spacing(np.abs(want)) / 2).all(), (got, want, err)


def test_qbf_loss_batch_and_calibrate_with_loss(gold):
    """loss_batch (ragged labels, float64) on the same pass as forward(x, target): within the bound of the golden without
    any float32 rounding; calibrate_with_loss returns calibrate's exponents and that batch's losses."""
    from yolo355 import synth
    cfg = LC.QBF
    m, twin = _qbf_model(), _qbf_model()
    x = torch.from_numpy(synth.make_images(cfg["image_seeds"][0], cfg["batch"], cfg["size"][0], cfg["size"][1], "blocks"))
    out, parts = m.loss_batch(x, LC.qbf_labels(0), quantization=True)
    assert parts.shape == (2, 5)
    LC.assert_losses(out, gold["qbf/0/out"], gold["qbf/0/gap"], "qbf loss_batch")
    sa, out2 = twin.calibrate_with_loss(x, LC.qbf_labels(0), freeze=False)
    assert sa == twin._engine.get_act_exponents() and np.array_equal(bits(out), bits(out2))
    # a frozen (trainable=False) model: the loss of the deployed graph, trackers untouched
    m.trainable = False
    before = {n: b.clone() for n, b in m.named_buffers()}
    out3, _ = m.loss_batch(x, LC.qbf_labels(0), quantization=True)
    assert np.array_equal(bits(out), bits(out3))
    assert all(torch.equal(b, before[n]) for n, b in m.named_buffers())
    # quantization=False: the bf16 graph's loss, against the restatement on its own prediction tap
    out4, parts4 = m.loss_batch(x, LC.qbf_labels(0), quantization=False)
    pred = m.__dict__["_f32"][0].get_tensor(m.__dict__["_f32"][0].num_tensors - 1, 2)
    target = R.make_targets(cfg["size"], 16, LC.qbf_labels(0), synth.ANCHOR_SIZE_MASK, False)
    want, want_parts = R.loss([pred], target, 16, synth.ANCHOR_SIZE_MASK, 2, cfg["size"], 16.0)
    rel_close(out4, want)
    rel_close(parts4, want_parts)


# (module, class, anchors, size, weight gain: 75 layers deep, yolo_v3 needs a tamer one for finite box sizes)
NET_MODELS = [("slim_yolo_v2", "SlimYOLOv2", "ANCHOR_SIZE", [64, 64], 2.0), ("yolo_v2", "myYOLOv2", "ANCHOR_SIZE", [64, 96], 2.0),
              ("tiny_yolo_v3", "YOLOv3tiny", "TINY_MULTI_ANCHOR_SIZE", [64, 96], 2.0), ("yolo_v3", "myYOLOv3", "MULTI_ANCHOR_SIZE", [64, 96], 1.0)]


@pytest.mark.parametrize("quantization", [False, True], ids=["bf16", "int8"])
@pytest.mark.parametrize("spec", NET_MODELS, ids=[s[1] for s in NET_MODELS])
def test_net_model_losses(spec, quantization):
    """loss_batch of a y355_net family equals the restatement fed the handle's own prediction-map tap (the plumbing, without
    inheriting bf16 error); forward(x, target=dense) agrees with it; the pinned refusals still raise."""
    import importlib
    from cases import synth_state_dict
    from yolo355 import synth, tools
    from yolo355.netengine import PRED_TAIL
    modname, clsname, an, size, gain = spec
    anchors = getattr(synth, an)
    C, B = 3, 2
    m = getattr(importlib.import_module("yolo355.models." + modname), clsname)("cuda:0", input_size=size, num_classes=C, trainable=True,
                                                                               conf_thresh=0.01, nms_thresh=0.5, anchor_size=anchors)
    m.load_state_dict(synth_state_dict(m.state_dict(), 11, weight_gain=gain))
    m.eval()
    x = torch.from_numpy(synth.make_images(61, B, size[0], size[1], "blocks"))
    labels = [LC.random_labels(7000 + b, 3 + b, C, 0.2, 0.9) for b in range(B)]
    out, parts = m.loss_batch(x, labels, quantization=quantization)
    net = m._ready_net(B, quantization)
    maps = sorted([net.get_tensor(net.num_tensors - k, B) for k in PRED_TAIL[modname]], key=lambda t: -t.shape[2] * t.shape[3])   # finest level first
    multi = not np.isscalar(m.stride)
    target = R.make_targets(size, m.stride, labels, anchors, multi)
    assert (target[..., 0] == 1).sum() >= B
    want, want_parts = R.loss(maps, target, m.stride, anchors, C, size, 1.0 if multi else float(m.stride))
    assert np.isfinite(out).all(), out
    rel_close(out, want)
    rel_close(parts, want_parts)
    creator = tools.multi_gt_creator if multi else tools.gt_creator
    dense = torch.tensor(creator(size, m.stride, labels, anchors)).float()
    if quantization and modname != "tiny_yolo_v3":                # (their forward has no quantization argument, as in the reference)
        res = m._forward_loss(x, dense, True)
    else:
        res = m(x, target=dense, quantization=True) if quantization else m(x, target=dense)
    assert all(v.dtype == torch.float32 and v.dim() == 0 for v in res)
    assert np.array_equal(np.array([float(v) for v in res], np.float32), out.astype(np.float32))
    with pytest.raises(NotImplementedError):
        m(x)                                                      # trainable=True, no target
    m.train()
    with pytest.raises(NotImplementedError):
        m(x, target=dense)                                        # BatchNorm in training mode
    m.eval()
    m.trainable = False
    assert len(m(x)) == 3                                         # trainable=False: detections, as before
    if quantization:
        m.trainable = True
        sa, out5 = m.calibrate_with_loss(x, labels, freeze=True)
        assert sa == m.act_exponents and np.isfinite(out5).all()
