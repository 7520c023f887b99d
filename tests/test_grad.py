"""The losses with their gradient on the GPU (csrc/grad.hip through yolo355/grad.py) at the shapes of tests/loss_cases.py:
the value against libyolo355_loss.so bit for bit, the gradient maps against the reference's own backward()
(tests/golden/grad.npz) under grad_ref.assert_maps' bound and, for the 416-pixel case, against the float64 restatement
(tests/grad_ref.py) within 1e-5 of each channel group's largest gradient; what makes the maps usable -- every element
written once, exact zeros at masked slots, the same bits from run to run, an image's gradient independent of its batch, the
upstream factors, backward alone, the flat form -- and the autograd module inside a torch graph."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import grad_ref as GR
import loss_cases as LC
import loss_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c[0] for c in LC.LOSS_CASES if c[1] != "m3_416"]
RUNS = {"total": None, "mix": (1.0, 2.0, 0.0, 0.0)}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "grad.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """(geometry tag, C, B, labels, maps) of a LOSS_CASES entry or of "nan": computed once, left unchanged"""
    if tag == "nan":
        labels, maps = LC.nan_case()
        return "t64", 2, 1, labels, maps
    _, g, C, B = next(c for c in LC.LOSS_CASES if c[0] == tag)
    return g, C, B, LC.loss_labels(tag), LC.loss_pred_maps(tag)


def handle(tag, cls=None, **kw):
    from yolo355 import grad as G
    g, C, B, labels, maps = inputs(tag)
    size, strides, anchors = LC.GEOM[g]
    h = (cls or G.YoloLossGrad)(size, strides, anchors, C, max_batch=B, max_labels_per_image=16, **kw)
    return h, labels, maps


def golden_maps(gold, tag, run):
    n = len([k for k in gold if k.startswith("grad/%s/%s/" % (tag, run))]) - 1
    return [gold["grad/%s/%s/%d" % (tag, run, l)] for l in range(n)], gold["grad/%s/%s/gap" % (tag, run)]


def host(maps):
    return [m.cpu().numpy() for m in maps]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------------------------------------------------ value and targets
@pytest.mark.parametrize("tag", [c[0] for c in LC.LOSS_CASES])
def test_value_is_the_loss_library_s_bit_for_bit(tag):
    from yolo355 import loss as L
    h, labels, maps = handle(tag)
    ref, _, _ = handle(tag, cls=L.YoloLoss)
    h.set_labels(labels)
    ref.set_labels(labels)
    dev = [torch.from_numpy(m).to(h.device) for m in maps]
    want, want_parts = ref.compute(dev)
    out, parts, grads = h.forward_backward(dev)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(parts), bits(want_parts)), (out, want)
    out2, parts2, none = h.forward_backward(dev, with_grad=False)                  # the value only: the same bits
    assert none == [] and np.array_equal(bits(out2), bits(want)) and np.array_equal(bits(parts2), bits(want_parts))
    out3, parts3, _ = h.forward_backward(dev, target=ref.targets())                # a caller's dense target
    assert np.array_equal(bits(out3), bits(want)) and np.array_equal(bits(parts3), bits(want_parts))
    assert [tuple(g.shape) for g in grads] == [m.shape for m in maps] and all(g.dtype == torch.float32 and g.is_cuda for g in grads)
    h.close()
    ref.close()


@pytest.mark.parametrize("tag", LC.TARGET_CASES)
def test_targets_are_the_loss_library_s_and_a_view(tag):
    from yolo355 import _ffi, grad as G, loss as L
    size, strides, anchors = LC.GEOM[tag]
    labels = LC.target_labels(tag)
    h = G.YoloLossGrad(size, strides, anchors, 2, max_batch=3, max_labels_per_image=70)
    ref = L.YoloLoss(size, strides, anchors, 2, max_batch=3, max_labels_per_image=70)
    with pytest.raises(_ffi.Y355Error, match="no labels set"):
        h.targets()
    with pytest.raises(_ffi.Y355Error, match="no labels set and no target given"):
        h.forward_backward([np.zeros((1, h.num_anchors * 7, hs, ws), np.float32) for hs, ws in h.grids])
    h.set_labels(labels)
    ref.set_labels(labels)
    t = h.targets()
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (3, h.num_anchors_total, 11)
    assert np.array_equal(bits(t.cpu().numpy()), bits(ref.targets()))
    p = ctypes.c_void_p()
    assert h._lib.y355_grad_targets_dev(h._h, 3, ctypes.byref(p)) == 0 and t.data_ptr() == p.value        # no copy
    h.set_labels(labels[2:] + labels[:1])                       # a batch of two: the view shows the handle's tensor as it is now
    ref.set_labels(labels[2:] + labels[:1])
    assert np.array_equal(bits(t[:2].cpu().numpy()), bits(ref.targets())) and tuple(h.targets().shape) == (2, h.num_anchors_total, 11)
    for bad in ([[[0.1, 0.1, 1.5, 0.5, 0]]], [[[0.1, 0.1, 0.5, 0.5, 2]]], [[], [], [], []]):
        with pytest.raises(_ffi.Y355Error):
            h.set_labels(bad)
    h.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------ gradient
NAN_FILL = 0x7FC0BEEF            # a quiet NaN no arithmetic produces


def prefilled(maps, device):
    return [torch.full(m.shape, NAN_FILL, dtype=torch.int32, device=device).view(torch.float32) for m in maps]


@pytest.mark.parametrize("tag", SMALL + ["nan"])
def test_gradient_equals_the_reference(gold, tag):
    """both upstreams against the golden; every element of pre-filled maps overwritten; two runs, backward alone and a caller's
    target give the same bits"""
    h, labels, maps = handle(tag)
    g, C = inputs(tag)[:2]
    A = LC.num_anchors(g)
    h.set_labels(labels)
    dev = [torch.from_numpy(m).to(h.device) for m in maps]
    for run, up in RUNS.items():
        want, gap = golden_maps(gold, tag, run)
        mine = prefilled(maps, h.device)
        _, _, grads = h.forward_backward(dev, upstream=up, grad_maps=mine)
        got = host(grads)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(grads, mine))
        assert not any((bits(m) == NAN_FILL).any() for m in got), "an element was not written"
        GR.assert_maps(got, want, gap, A, C, "%s %s" % (tag, run))
        assert same_bits(host(h.forward_backward(dev, upstream=up)[2]), got), "run to run"
        assert same_bits(host(h.backward(dev, upstream=up, grad_maps=prefilled(maps, h.device))), got), "y355_grad_backward"
        assert same_bits(host(h.backward(dev, target=h.targets().clone(), upstream=np.asarray(up or GR.UNIT, np.float32))), got)
    h.close()


def test_large_case_against_the_restatement():
    """N = 10 647: more than one grid-stride pass of the 32 workgroups of an image; 1e-5 of each group's largest gradient"""
    tag = "m3_416_c20_b2"
    h, labels, maps = handle(tag)
    g, C = inputs(tag)[:2]
    size, strides, anchors = LC.GEOM[g]
    A = LC.num_anchors(g)
    assert h.num_anchors_total == 10647 > 32 * 256
    h.set_labels(labels)
    target = h.targets().cpu().numpy()
    want = GR.map_grads(maps, target, strides, anchors, C, size, LC.wh_mul(g))
    mine = prefilled(maps, h.device)
    _, _, grads = h.forward_backward(maps, grad_maps=mine)
    got = host(grads)
    assert not any((bits(m) == NAN_FILL).any() for m in got)
    assert all(np.isfinite(m).all() for m in got)
    err, top = GR.group_gap(got, want, A, C), GR.group_max(want, A, C)
    for k in GR.GROUPS:
        print(tag, k, "err %.3g bound %.3g" % (err[k], 1e-5 * top[k]))
        assert top[k] > 0 and err[k] <= 1e-5 * top[k], (k, err[k], top[k])
    assert same_bits(host(h.backward(maps)), got)
    h.close()


@pytest.mark.parametrize("tag", ["t64_c2_b5", "m3_c20_b5"])
def test_masked_slots_hold_exact_zeros(tag):
    h, labels, maps = handle(tag)
    g, C = inputs(tag)[:2]
    A = LC.num_anchors(g)
    h.set_labels(labels)
    t = h.targets().cpu().numpy()
    _, _, grads = h.forward_backward(maps)
    _, g_cls, g_box = R.split_pred(host(grads), A, C)
    ignored, unassigned, positive = t[..., 0] == -1, (t[..., 0] == 0) & (t[..., 6] == 0), t[..., 0] == 1
    assert ignored.any() and unassigned.any() and positive.any() and (ignored | unassigned | positive).all()
    for slots in (ignored, unassigned):
        assert (g_cls[slots] == 0).all() and (g_box[slots] == 0).all()
    assert (g_cls[positive] != 0).all() and (g_box[positive] != 0).any()
    g_conf = R.split_pred(host(grads), A, C)[0]
    assert (g_conf[ignored] == 0).all() and (g_conf[unassigned] != 0).all()
    h.close()


@pytest.mark.parametrize("tag", ["t96x64_c20_b5", "m3_c2_b5"])
def test_an_image_s_gradient_does_not_depend_on_its_batch(tag):
    """image b of the batch of five, upstream None, against the image alone with upstream (0, 0, 0, 1/5 as fp32): k is the
    last factor of every element, and fl(1 / 5) is what (0 + 1) / 5 gives"""
    h, labels, maps = handle(tag)
    h.set_labels(labels)
    dev = [torch.from_numpy(m).to(h.device) for m in maps]
    dense = h.targets().clone()
    _, _, grads = h.forward_backward(dev)
    whole = host(grads)
    fifth = torch.tensor([0.0, 0.0, 0.0, float(np.float32(1.0) / np.float32(5.0))], dtype=torch.float32)
    for b in range(5):
        _, _, one = h.forward_backward([m[b:b + 1] for m in dev], target=dense[b:b + 1], upstream=fifth)
        assert same_bits(host(one), [w[b:b + 1] for w in whole]), b
    h.close()


def test_zero_upstream_gives_zeros_and_nan_where_zero_times_nan_arises():
    h, labels, maps = handle("nan")
    h.set_labels(labels)
    _, _, grads = h.forward_backward(maps, upstream=(0.0, 0.0, 0.0, 0.0))
    (m,) = host(grads)
    assert np.isnan(m).sum() == 1 and np.isnan(m[0, 0, 0, 0])
    assert (m[~np.isnan(m)] == 0).all()
    h.close()
    h, labels, maps = handle("m2_c20_b5")
    h.set_labels(labels)
    assert all((g == 0).all() for g in host(h.forward_backward(maps, upstream=(0.0, 0.0, 0.0, 0.0))[2]))
    h.close()


# ------------------------------------------------------------------------------------------------------------ flat form
def flat_inputs(h, maps, A, C):
    """The tensors the models hand tools.loss, cut from the maps on the device.  The label's IoU has to carry the bits the map
    kernel computes for itself: the decode in the kernel's operation order, one torch operation per rounding (no two of them
    can fuse into an fma), and the library's own iou_score on the result."""
    from yolo355 import loss as L
    dev = [torch.from_numpy(m).to(h.device) for m in maps]
    conf, cls, box = (torch.from_numpy(v).to(h.device) for v in R.split_pred(maps, A, C))
    t = h.targets()
    gx, gy, st, aw, ah = [], [], [], [], []
    anchors = np.asarray(h.anchors, np.float32).reshape(len(h.strides), A, 2)
    for (hs, ws), s, an in zip(h.grids, h.strides, anchors):
        yy, xx = np.meshgrid(np.arange(hs), np.arange(ws), indexing="ij")
        gx.append(np.repeat(xx.reshape(-1), A)); gy.append(np.repeat(yy.reshape(-1), A))
        st.append(np.full(hs * ws * A, s)); aw.append(np.tile(an[:, 0], hs * ws)); ah.append(np.tile(an[:, 1], hs * ws))
    gx, gy, st, aw, ah = (torch.from_numpy(np.concatenate(v).astype(np.float32)).to(h.device) for v in (gx, gy, st, aw, ah))
    full = lambda v: torch.full_like(conf, float(v))             # tensor operands: a scalar divisor would become a reciprocal
    sig = lambda x: torch.div(full(1), torch.add(torch.exp(torch.neg(x)), full(1)))
    wh_mul = full(1.0 if h.multi else h.strides[0])
    cx, cy = torch.mul(torch.add(sig(box[..., 0]), gx), st), torch.mul(torch.add(sig(box[..., 1]), gy), st)
    bw, bh = torch.mul(torch.mul(torch.exp(box[..., 2]), aw), wh_mul), torch.mul(torch.mul(torch.exp(box[..., 3]), ah), wh_mul)
    hw, hh = torch.div(bw, full(2)), torch.div(bh, full(2))
    in_h, in_w = full(h.input_size[0]), full(h.input_size[1])
    dec = torch.stack([torch.div(torch.sub(cx, hw), in_w), torch.div(torch.sub(cy, hh), in_h), torch.div(torch.add(cx, hw), in_w),
                       torch.div(torch.add(cy, hh), in_h)], -1)
    iou = L.iou_score(dec.reshape(-1, 4), t[..., 7:].reshape(-1, 4)).view(conf.shape)
    label = torch.cat([iou.unsqueeze(-1), t[..., :7]], -1).contiguous()
    return dev, conf.unsqueeze(-1), cls, box, label


@pytest.mark.parametrize("tag", ["t64_c2_b5", "t96x64_c20_b1", "m3_c20_b5", "nan"])
def test_flat_form_agrees_with_the_map_form_bit_for_bit(tag):
    from yolo355 import grad as G
    h, labels, maps = handle(tag)
    g, C, B = inputs(tag)[:3]
    A = LC.num_anchors(g)
    h.set_labels(labels)
    dev, conf, cls, box, label = flat_inputs(h, maps, A, C)
    for up in (None, (1.0, 2.0, 0.0, 0.0)):
        out, parts, grads = h.forward_backward(dev, upstream=up)
        f_out, f_parts, (g_conf, g_cls, g_box) = G.flat_forward_backward(conf, cls, box, label, C, upstream=up)
        assert g_conf.shape == conf.shape and g_cls.shape == cls.shape and g_box.shape == box.shape
        want = R.split_pred(host(grads), A, C)
        got = [g_conf[..., 0].cpu().numpy(), g_cls.cpu().numpy(), g_box.cpu().numpy()]
        for name, a, b in zip(GR.GROUPS, got, want):
            print(tag, name, "elements that differ:", int((bits(a) != bits(b)).sum()))
        assert same_bits(got, list(want))
        assert np.array_equal(bits(f_out), bits(out)) and np.array_equal(bits(f_parts), bits(parts))
    h.close()


@pytest.mark.parametrize("C", [24, 25])
def test_both_sides_of_the_register_threshold(C):
    """C = 24 is the last class count whose logits stay in registers (Y355_GRAD_CREG), C = 25 the first that reads them
    again: value against the loss library (bits), gradient against the restatement (1e-5 of each group's largest gradient)
    and against the flat form, which always reads again (bits)"""
    from yolo355 import grad as G, loss as L, synth
    size, strides, anchors = LC.GEOM["t96x64"]
    A, B = LC.num_anchors("t96x64"), 2
    labels = [LC.random_labels(8100 + C + b, 3 + b, C) for b in range(B)]
    maps = [synth.uniform_pm1(8200 + C, (B, A * (5 + C), 6, 4)) * np.float32(2.0)]
    h = G.YoloLossGrad(size, strides, anchors, C, max_batch=B, max_labels_per_image=16)
    ref = L.YoloLoss(size, strides, anchors, C, max_batch=B, max_labels_per_image=16)
    h.set_labels(labels)
    ref.set_labels(labels)
    assert (ref.targets()[..., 0] == 1).sum() >= B
    out, parts, grads = h.forward_backward(maps, grad_maps=prefilled(maps, h.device))
    want_out, want_parts = ref.compute(maps)
    assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(parts), bits(want_parts))
    got = host(grads)
    assert not any((bits(m) == NAN_FILL).any() for m in got)
    want = GR.map_grads(maps, ref.targets(), strides, anchors, C, size, LC.wh_mul("t96x64"))
    err, top = GR.group_gap(got, want, A, C), GR.group_max(want, A, C)
    for k in GR.GROUPS:
        print("C", C, k, "err %.3g bound %.3g" % (err[k], 1e-5 * top[k]))
        assert top[k] > 0 and err[k] <= 1e-5 * top[k], (k, err[k], top[k])
    assert same_bits(host(h.backward(maps)), got)
    _, conf, cls, box, label = flat_inputs(h, maps, A, C)
    f_out, _, (g_conf, g_cls, g_box) = G.flat_forward_backward(conf, cls, box, label, C)
    assert same_bits([g_conf[..., 0].cpu().numpy(), g_cls.cpu().numpy(), g_box.cpu().numpy()], list(R.split_pred(got, A, C)))
    assert np.array_equal(bits(f_out), bits(out))
    h.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------ inside a torch graph
def conv_head(tag, seed=5):
    g, C, B, labels, maps = inputs(tag)
    A = LC.num_anchors(g)
    torch.manual_seed(seed)
    hs, ws = maps[0].shape[2:]
    head = torch.nn.Conv2d(8, A * (5 + C), 1).to("cuda:0")
    x = torch.randn(B, 8, hs, ws, device="cuda:0")
    return head, x


def weight_bound(x, gmap):
    """what two fp32 summation orders of weight.grad[o, i] = sum g[b, o, y, x] * x[b, i, y, x] may differ by: n summands, each
    product rounded once, n - 1 additions: n * 2^-23 * sum |g| |x| covers both orders"""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    return n * 2.0 ** -23 * torch.einsum("boyx,biyx->oi", gmap.abs().double(), x.abs().double())


@pytest.mark.parametrize("tag", ["t64_c2_b5", "t96x64_c20_b5"])
def test_criterion_inside_a_torch_graph(gold, tag):
    """a 1 x 1 convolution head in front of YoloCriterion: backward() from total_loss and from conf_loss + 2 * cls_loss gives
    the head the weight gradient that torch gives when handed our (golden-checked) gradient map by hand"""
    from yolo355 import grad as G
    g, C, B, labels, maps = inputs(tag)
    size, strides, anchors = LC.GEOM[g]
    crit = G.YoloCriterion(size, strides, anchors, C, max_batch=B, max_labels_per_image=16)
    head, x = conv_head(tag)
    for pick, up in ((lambda o: o[3], None), (lambda o: o[0] + 2 * o[1], (1.0, 2.0, 0.0, 0.0))):
        head.zero_grad()
        pred = head(x)
        out = crit(pred, label_lists=labels)
        assert len(out) == 4 and all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.grad_fn is not None for v in out)
        want_out, _, gmaps = crit.handle.forward_backward(pred.detach(), upstream=up)
        assert np.array_equal(np.array([float(v) for v in out], np.float32), want_out.astype(np.float32))
        pick(out).backward()
        want_w, want_b = torch.autograd.grad(head(x), [head.weight, head.bias], grad_outputs=gmaps[0])
        err = (head.weight.grad - want_w).abs().double().reshape(want_w.shape[0], -1)
        print(tag, "weight.grad err %.3g of %.3g" % (float(err.max()), float(want_w.abs().max())))
        assert (err <= weight_bound(x, gmaps[0])).all()
        assert torch.allclose(head.bias.grad, want_b, rtol=0, atol=float(x.shape[0] * x.shape[2] * x.shape[3] * 2.0 ** -23 * gmaps[0].abs().sum((0, 2, 3)).max()))
        assert float(want_w.abs().max()) > 0
    # a dense target instead of label lists, and neither: the labels of the last call
    dense = crit.handle.targets().clone()
    a = crit(head(x).detach(), target=dense)
    b = crit(head(x).detach())
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        crit(head(x), label_lists=labels, target=dense)
    crit.close()


def test_criterion_respects_a_non_default_stream(gold):
    """forward and backward on a side stream, results read on it without any synchronise by the test"""
    from yolo355 import grad as G
    tag = "t96x64_c20_b5"
    g, C, B, labels, maps = inputs(tag)
    size, strides, anchors = LC.GEOM[g]
    crit = G.YoloCriterion(size, strides, anchors, C, max_batch=B, max_labels_per_image=16)
    head, x = conv_head(tag)
    crit.handle.set_labels(labels)
    want_out, _, gmaps = crit.handle.forward_backward(head(x).detach())
    want_w = torch.autograd.grad(head(x), [head.weight], grad_outputs=gmaps[0])[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        head.zero_grad()
        pred = head(x)
        pred.retain_grad()
        out = crit(pred, label_lists=labels)
        out[3].backward()
        got_map, got_w = pred.grad.cpu().numpy(), head.weight.grad.clone()
        got_out = np.array([float(v) for v in out], np.float32)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(got_out, want_out.astype(np.float32))
    assert np.array_equal(bits(got_map), bits(gmaps[0].cpu().numpy()))
    assert ((got_w - want_w).abs().double() <= weight_bound(x, gmaps[0])).all()
    crit.close()


@pytest.mark.parametrize("tag", ["t64_c2_b5", "m3_c20_b5"])
def test_flat_drop_in_carries_a_graph(tag):
    """yolo355.grad.loss on leaf tensors: backward() from total_loss and from conf_loss + 2 * cls_loss fills the leaves with
    y355_grad_flat's gradients"""
    from yolo355 import grad as G, loss as L
    h, labels, maps = handle(tag)
    g, C = inputs(tag)[:2]
    A = LC.num_anchors(g)
    h.set_labels(labels)
    _, conf, cls, box, label = flat_inputs(h, maps, A, C)
    for pick, up in ((lambda o: o[3], None), (lambda o: o[0] + 2 * o[1], (1.0, 2.0, 0.0, 0.0))):
        leaves = [v.clone().requires_grad_(True) for v in (conf, cls, box)]
        out = G.loss(leaves[0], leaves[1], leaves[2], label, C)
        assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.grad_fn is not None for v in out)
        want_out, _, want = G.flat_forward_backward(conf, cls, box, label, C, upstream=up)
        assert np.array_equal(np.array([float(v) for v in out], np.float32), want_out.astype(np.float32))
        assert all(torch.equal(a, b) for a, b in zip(out, L.loss(conf, cls, box, label, C)))          # the value-only drop-in's numbers
        pick(out).backward()
        assert same_bits([v.grad.cpu().numpy() for v in leaves], [w.cpu().numpy() for w in want])
    h.close()


# ------------------------------------------------------------------------------------------------------------ handles
def test_two_handles_of_different_geometry_do_not_disturb_each_other():
    tags = ("t96x64_c2_b5", "m3_c20_b1")
    alone = []
    for tag in tags:
        h, labels, maps = handle(tag)
        h.set_labels(labels)
        out, parts, grads = h.forward_backward(maps)
        alone.append((out, parts, host(grads)))
        h.close()
    hs = [handle(tag) for tag in tags]
    for h, labels, _ in hs:
        h.set_labels(labels)
    for rnd in range(2):                                            # interleaved, twice
        for (h, _, maps), (out, parts, grads) in zip(hs, alone):
            o, p, g = h.forward_backward(maps)
            assert np.array_equal(bits(o), bits(out)) and np.array_equal(bits(p), bits(parts)) and same_bits(host(g), grads)
    for (h, _, maps), (_, _, grads) in zip(reversed(hs), reversed(alone)):
        assert same_bits(host(h.backward(maps)), grads)
    for h, _, _ in hs:
        h.close()
