"""int8 forms of myYOLOv2, myYOLOv3 and myYOLOv3Spp (y355_net with Y355_DT_INT8): the integer rules of the DarkNet-only ops
(residual, network input, reorg into a concat buffer, SPP) restated in tests/int8_wide_ref.py, checked here against their
definitions and the reference's fp32 maps on the CPU, and against the engine bit for bit on the GPU."""
import os
from fractions import Fraction

import numpy as np
import pytest

import int8_wide_ref as R
from cases import WIDE_MODEL_CASES, WIDE3_MODEL_CASES, synth_state_dict
from helpers import dets_match

WGOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "models_wide.npz"))
# (tag, arch, drop-in class, input size, classes, seed, weight gain) -- the reference's golden cases
CASES = [(t, "yolo_v2", c, s, k, seed, 2.0) for t, c, s, k, seed in WIDE_MODEL_CASES] + \
        [(t, m.split(".")[-1], c, s, k, seed, g) for t, m, c, s, k, seed, g in WIDE3_MODEL_CASES]


def _model(arch, cls, size, classes, seed, gain, device="cpu", conf=0.05):
    from yolo355 import synth
    from yolo355.models import yolo_v2, yolo_v3
    mod = yolo_v2 if arch == "yolo_v2" else yolo_v3
    anchors = synth.ANCHOR_SIZE if arch == "yolo_v2" else synth.MULTI_ANCHOR_SIZE
    m = getattr(mod, cls)(device, input_size=size, num_classes=classes, trainable=False, conf_thresh=conf, nms_thresh=0.5,
                          anchor_size=anchors)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed, weight_gain=gain))
    m.eval()
    return m, anchors


def _rne(v):
    """round half to even of a Fraction"""
    f = v.numerator // v.denominator
    r = v - f
    return f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2) else 0)


def _clamp(q):
    return max(-127, min(127, q))


# ---------------------------------------------------------------------------------------------------- CPU
def test_residual_rule_matches_its_definition():
    """u = t' 2^(G-E) + q_r 2^(G-s_r), q = clamp(RNE(u 2^(s_out-G))): both signs, exact ties, E >= s_r and E < s_r,
    saturating cases -- against exact rational arithmetic"""
    rng = np.random.default_rng(7)
    for E, s_r, s_out in [(20, 5, 4), (20, 20, 12), (6, 9, 7), (3, 11, 11), (12, 4, 9), (0, 3, -2), (15, 15, 15)]:
        tp = rng.integers(-2 ** 26, 2 ** 26, size=400, dtype=np.int64)
        qr = rng.integers(-127, 128, size=400, dtype=np.int64)
        sh = max(E, s_r) - s_out
        if sh > 0 and E >= s_r:         # exact ties: u = (2k + 1) 2^(sh-1)
            tp[:40] = (2 * rng.integers(-300, 300, 40) + 1) << (sh - 1)
            qr[:40] = 0
        q, sat = R.residual_rule(tp, E, qr, s_r, s_out)
        want = [_rne((Fraction(int(a), 2 ** E) + Fraction(int(b), 2 ** s_r)) * Fraction(2) ** s_out) for a, b in zip(tp, qr)]
        assert [int(v) for v in q] == [_clamp(w) for w in want], (E, s_r, s_out)
        assert sat == sum(abs(w) > 127 for w in want)
        assert sat > 0 or max(abs(w) for w in want) <= 127
    # the whole epilogue: requant() on a conv equals t' then the rule
    L = dict(q_b=np.array([3, -5], np.int64), e_w=7, e_b=9)
    acc = rng.integers(-5000, 5000, size=(1, 2, 3, 3)).astype(np.int64)
    qr = rng.integers(-127, 128, size=(1, 2, 3, 3))
    for act in (R.L100, R.L125, R.NONE):
        lk, m = R.ACT[act]
        for sa_in, s_r, s_out in [(4, 2, 3), (4, 30, 5), (2, 6, 6)]:
            Fb = max(sa_in + 7, 9)
            got = R.requant(acc, L, sa_in, s_out, act, qr, s_r)
            for idx in np.ndindex(acc.shape):
                t = Fraction(int(acc[idx]), 2 ** (sa_in + 7)) + Fraction(int(L["q_b"][idx[1]]), 2 ** 9)
                tp = t if t >= 0 else t * Fraction(m, 2 ** lk)
                assert (tp * 2 ** Fb * 2 ** lk).denominator == 1
                assert got[idx] == _rne((tp + Fraction(int(qr[idx]), 2 ** s_r)) * Fraction(2) ** s_out), (act, sa_in, s_r, s_out)


def test_reorg_rescale_and_input_rules_match_their_definition():
    rng = np.random.default_rng(11)
    q = rng.integers(-127, 128, size=(2, 8, 4, 6))
    for d in (-3, -1, 0, 1, 2, 8):
        got, sat = R.rescale(q, d)
        want = np.array([_rne(Fraction(int(v)) * Fraction(2) ** d) for v in q.ravel()]).reshape(q.shape)
        assert np.array_equal(got, np.clip(want, -127, 127)) and sat == int((np.abs(want) > 127).sum())
    r = R.reorg(q, 2)                                   # out channel (sy*2 + sx)*C + c
    for sy in range(2):
        for sx in range(2):
            assert np.array_equal(r[:, (sy * 2 + sx) * 8:(sy * 2 + sx + 1) * 8], q[:, :, sy::2, sx::2])
    x = np.concatenate([rng.normal(0, 3, 300), np.arange(-20, 20) + 0.5, [300.0, -300.0, 126.5, -127.5]]).astype(np.float32)
    for sa_in in (0, 2, 5):
        got, sat = R.quantize_input(x, sa_in)
        want = [_rne(Fraction(float(v)) * Fraction(2) ** sa_in) for v in x]
        assert [int(v) for v in got] == [_clamp(w) for w in want] and sat == sum(abs(w) > 127 for w in want)
    # SPP: clipped windows -- a corner of all-negative values keeps its own maximum (a zero halo would give 0)
    t = -np.arange(1, 1 + 2 * 3 * 7 * 7).reshape(2, 3, 7, 7).astype(np.int64)
    p5, p9, p13 = R.spp_pools(t)
    assert p5[0, 0, 0, 0] == t[0, 0, :3, :3].max() and p13[1, 2, 6, 6] == t[1, 2].max() and (p9 < 0).all()


def test_stride2_conv_equals_torch_conv2d():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    for H, W in [(8, 8), (7, 10), (13, 6)]:
        q = rng.integers(-127, 128, size=(2, 5, H, W))
        w = rng.integers(-127, 128, size=(4, 5, 3, 3))
        got = R.conv_int(q, w, 2)
        want = F.conv2d(torch.as_tensor(q, dtype=torch.float64), torch.as_tensor(w, dtype=torch.float64), None, 2, 1).numpy()
        assert got.shape == (2, 4, (H + 1) // 2, (W + 1) // 2) and np.array_equal(got, want.astype(np.int64))


def test_quantized_weights_of_the_product_equal_the_restatement():
    from oracle import net_int8_oracle as N
    from yolo355 import prep
    from yolo355.utils.modules import folded_f32
    tag, arch, cls, size, classes, seed, gain = CASES[1]
    m, _ = _model(arch, cls, size, classes, seed, gain)
    folded = N.fold_bn(R.layers_of(m))
    prod = prep.quantize_folded([folded_f32(c) for c in m._conv_modules()])
    assert len(prod) == R.GRAPHS[arch]().nlayers
    for a, b in zip(prod, N.quantize_folded(folded)):
        assert a["e_w"] == b["e_w"] and a["e_b"] == b["e_b"]
        assert np.array_equal(a["q_w"], b["q_w"]) and np.array_equal(a["q_b"], b["q_b"])


# relative L2 of the int8 maps against the reference's fp32 maps (exponents from the float64 activations), measured on
# the CPU: yolo_v2_224 0.0909; yolo_v3_224 0.0300 / 0.0357 / 0.0365 and yolo_v3_spp_224 0.0314 / 0.0354 / 0.0402 (strides
# 8, 16, 32).  Asserted with about 30 % margin.
REL_L2 = {"yolo_v2": 0.12, "yolo_v3": 0.055, "yolo_v3_spp": 0.055}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_tracks_the_reference_fp32_maps(case):
    from oracle import net_int8_oracle as N
    from yolo355 import synth
    tag, arch, cls, size, classes, seed, gain = case
    m, anchors = _model(arch, cls, size, classes, seed, gain)
    layers = R.layers_of(m)
    folded = N.fold_bn(layers)
    predc = m.anchor_number * (5 + classes)
    x = synth.make_images(seed + 1, 1, size[0], size[1])
    sa_in, sa, T = R.calibrate_f64(arch, x, folded, predc)
    g = R.GRAPHS[arch]()
    gold = [WGOLD[tag + "_pred"]] if arch == "yolo_v2" else [WGOLD[tag + "_pred_%d" % k].astype(np.float64) for k in (1, 2, 3)]
    for p, ref in zip(g.pred, gold):         # the float64 graph is the reference's model
        assert np.abs(T[p] - ref).max() < 2e-3 * np.abs(ref).max() + 2e-3
    r = R.forward_int(arch, x, N.quantize_folded(folded), sa_in, sa, predc)
    rel = []
    for p, ref in zip(R.preds_float(r), gold):
        rel.append(float(np.sqrt(((p.astype(np.float64) - ref) ** 2).sum() / (ref.astype(np.float64) ** 2).sum())))
    print(tag, "relative L2", ["%.4f" % v for v in rel])
    assert max(rel) <= REL_L2[arch], rel


# ---------------------------------------------------------------------------------------------------- GPU
GPU_CASES = CASES + [("yolo_v2_224x320", "yolo_v2", "myYOLOv2", [224, 320], 20, 4100, 2.0),
                     ("yolo_v3_224x320", "yolo_v3", "myYOLOv3", [224, 320], 20, 4200, 1.3)]


def _images(seed, B, size):
    from yolo355 import synth
    return np.concatenate([synth.make_images(seed + 1 + i, 1, size[0], size[1]) for i in range(B)])


def _check_against_restatement(net, x, ref, arch, size, anchors, classes, conf):
    B = x.shape[0]
    sa_in, sa_eff = net.get_act_exponents()
    assert sa_eff == ref["sa"]
    out = net.forward(x, tap=True)
    for t in range(net.num_tensors):
        got = np.rint(net.get_tensor(t, B).astype(np.float64) * 2.0 ** sa_eff[t]).astype(np.int64)
        assert np.array_equal(got, ref["t"][t]), "tensor %d differs in %d places" % (t, int((got != ref["t"][t]).sum()))
    assert net.counters() == ref["sat"]
    box, sc, dets = R.detect(arch, ref, size, anchors, classes, conf, 0.5)
    cb, cs, cc = net.candidates(B)
    assert np.allclose(cb, box, atol=2e-5, rtol=0)
    assert np.allclose(cs, sc.max(axis=2), atol=2e-6, rtol=1e-5)
    for i in range(B):
        ok, msg = dets_match(dets[i][:3], out[i], all_scores=sc[i].max(axis=1))
        assert ok, (i, msg)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_int8_wide_bit_exact(case):
    import torch
    from oracle import net_int8_oracle as N
    tag, arch, cls, size, classes, seed, gain = case
    B = 2
    m, anchors = _model(arch, cls, size, classes, seed, gain, device="cuda")
    predc = m.anchor_number * (5 + classes)
    x = _images(seed, B, size)
    xd = torch.from_numpy(x).cuda()
    # the drop-in: exponents freeze at the first quantized call (bf16 run of that input) and are reused after
    assert m.act_exponents is None
    first = m.forward_batch(xd, quantization=True)
    exps = m.act_exponents
    assert exps is not None
    folded = N.fold_bn(R.layers_of(m))
    sa_in, sa, T = R.calibrate_f64(arch, x, folded, predc)
    assert abs(exps[0] - sa_in) <= 1
    assert all(abs(a - b) <= 1 for a, b in zip(exps[1], sa)), [(i, a, b) for i, (a, b) in enumerate(zip(exps[1], sa)) if abs(a - b) > 1]
    x2 = _images(seed + 50, B, size)
    m.forward_batch(torch.from_numpy(x2).cuda(), quantization=True)
    assert m.act_exponents is exps
    net = m._get_net(B, int8=True)
    assert net.get_act_exponents()[0] == exps[0]
    # bit-exact against the restatement on the product's own exponents and weights
    qor = N.quantize_folded(folded)
    ref = R.forward_int(arch, x, qor, exps[0], exps[1], predc)
    out = _check_against_restatement(net, x, ref, arch, size, anchors, classes, 0.05)
    for i in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(first[i], out[i]))
    # without the tap: the same detections; element i of the batch equals the single-image run
    out2 = net.forward(x)
    for i in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(out[i], out2[i]))
    for i in range(B):
        one = net.forward(x[i:i + 1])[0]
        assert all(np.array_equal(a, b) for a, b in zip(one, out[i])), i


@pytest.mark.gpu
def test_int8_residual_with_E_below_s_r_is_exact_or_erange():
    """exponents that put a residual tensor's exponent above E = F + lk of the layer adding it: bit-exact to the
    restatement where the 64-bit bound holds, Y355_ERANGE (and the exponents unchanged) where it does not"""
    import torch
    from oracle import net_int8_oracle as N
    from yolo355 import _ffi
    tag, arch, cls, size, classes, seed, gain = CASES[1]
    B = 2
    m, anchors = _model(arch, cls, size, classes, seed, gain, device="cuda")
    predc = m.anchor_number * (5 + classes)
    x = _images(seed, B, size)
    m.forward_batch(torch.from_numpy(x).cuda(), quantization=True)
    net = m._get_net(B, int8=True)
    sa_in, sa = m.act_exponents
    folded = N.fold_bn(R.layers_of(m))
    qor = N.quantize_folded(folded)
    g = R.GRAPHS[arch]()
    sa_eff = R.effective_exponents(g, sa_in, sa)
    res_ops = [o for o in g.ops if o["op"] == "conv" and o["res"] >= 0]
    o = res_ops[len(res_ops) // 2]
    L = qor[o["layer"]]
    E = max(sa_eff[o["i"]] + L["e_w"], L["e_b"]) + R.ACT[o["act"]][0]
    sa2 = list(sa)
    sa2[o["res"]] = E + 3
    assert sa2[o["res"]] > E
    net.set_act_exponents(sa_in, sa2)
    ref = R.forward_int(arch, x, qor, sa_in, sa2, predc)
    _check_against_restatement(net, x, ref, arch, size, anchors, classes, 0.05)
    # far beyond: u cannot be bounded in int64 -> ERANGE, nothing changed
    sa3 = list(sa2)
    sa3[o["res"]] = 64
    with pytest.raises(_ffi.Y355Error) as ei:
        net.set_act_exponents(sa_in, sa3)
    assert ei.value.code == _ffi.ERANGE
    assert net.get_act_exponents()[1] == ref["sa"]


@pytest.mark.gpu
def test_int8_yolo_v3_at_416_compaction_head_is_exact():
    """10 647 anchors per image: the threshold-then-compact head on the engine's own int8 maps, B = 2"""
    import torch
    from oracle import fp32_oracle as F
    size, classes, seed = [416, 416], 20, 4200
    m, anchors = _model("yolo_v3", "myYOLOv3", size, classes, seed, 1.3, device="cuda")
    x = torch.from_numpy(_images(seed, 2, size)).cuda()
    outs = m.forward_batch(x, quantization=True)
    net = m._get_net(2, int8=True)
    assert net.num_anchors_total == 10647
    nt = net.num_tensors
    preds = [net.get_tensor(nt - 1, 2), net.get_tensor(nt - 3, 2), net.get_tensor(nt - 5, 2)]
    want = F.detect_v3(preds, anchors, classes, size, 0.05, 0.5)
    for (b, s, c), w in zip(outs, want):
        assert len(s) > 20 and len(w[1]) == len(s) and np.array_equal(w[2], c)
        assert np.abs(w[0] - b).max() < 2e-5 and np.abs(w[1] - s).max() < 2e-6
