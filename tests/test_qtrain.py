"""The quantisation-aware training step on the GPU (csrc/qtrain.hip through yolo355/qtrain.py) at the shapes of
tests/qtrain_cases.py, each under the calibrated activation exponents ("cal") and under exponents one higher ("cal+1": every
tracker clips in t64_b2_c20 or t16_b5_c2).

Exact, bit for bit: A_k 2^e_a[k] and P 2^e_a[10] against the integer oracle (oracle/yolo_oracle.py, saturate=True) and, on
t64_b2_c20 (64 x 64, a size the int8 engine takes), against Engine.get_feature after load_quantized(quantized_layers()) +
set_act_exponents; the state bytes against the float64 restatement (tests/qtrain_ref.py); act_stats against the oracle's sat and
maxima; the packed weights, bq and the exponents against prep.quantize_folded of the masters, before and after SGD steps; G_10;
the zeros of clipped and unselected elements; the SGD update against the NumPy restatement; the same bits from run to run.
Per op, from the handle's own tensors, every element: G_{k-1} in tests/test_train.py's interval with the factor of the state
byte; dW / db within 2 K u S 1.001.  The whole step: the losses are libyolo355_grad.so's on the handle's P; every layer's
gradient within a relative L2 distance of 2 * emu_relerr + 1e-6 of the float64 straight-through backward, emu_relerr the
distance of the CPU emulation that rounds every G to bf16.

Measured on one MI355X: the module (55 tests) in 4.9 s, its slowest test 0.53 s (the first, which computes the oracle on the
CPU); the whole-step distances are in test_gradients_against_the_float64_straight_through_backward's docstring; under "cal+1"
the clipped share per tracker is 0.04 % .. 11 % on t64_b2_c20 and 0 .. 12 % on t16_b5_c2, each of the eleven non-zero in one."""
import functools

import numpy as np
import pytest
import torch

import bf16_layer_ref as BL
import qtrain_cases as QC
import qtrain_ref as QR
import train_cases as TC
import train_ref as TR

pytestmark = pytest.mark.gpu
U = TR.U


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def trainer(tag, eset="cal", lr=1e-3, size=None, max_batch=None, ws=None, exps=None):
    from yolo355 import qtrain as Q
    csize, B, C = QC.CASES[tag]
    t = Q.SlimQatTrainer(size or csize, C, QC.ANCHORS, max_batch or B, lr)
    t.load_weights(ws if ws is not None else QC.weights(tag))
    t.set_act_exponents(exps if exps is not None else QC.exponents(tag, eset))
    return t


def all_grads(t):
    return [t.get_grad(k) for k in range(1, 11)]


def same_grads(a, b):
    return all(same(x[0], y[0]) and same(x[1], y[1]) for x, y in zip(a, b))


def everything(t):
    """the gradients, losses, P, statistics and every tensor the handle hands out after a forward_backward"""
    from yolo355 import qtrain as Q
    out = [g for pair in all_grads(t) for g in pair] + [np.array(t.losses), t.pred().cpu().numpy().copy()] + list(t.act_stats())
    out += [t.get_tensor(Q.ACT, k) for k in range(10)] + [t.get_tensor(Q.STATE, k) for k in range(1, 11)] + [t.get_tensor(Q.GRAD, k) for k in range(1, 11)]
    return out


@functools.lru_cache(maxsize=None)
def run(tag, eset):
    """one forward_backward of a case on a fresh trainer and everything the tests read from it: computed once, left unchanged"""
    from yolo355 import qtrain as Q
    t = trainer(tag, eset)
    losses = t.forward_backward(dev(QC.images(tag)), QC.labels(tag))
    r = dict(losses=np.array(t.losses), loss_tensors=[float(v) for v in losses], P=t.pred().cpu().numpy().copy(), dP=t._dpred.cpu().numpy().copy())
    r["A"] = [TR.bf16_bits_to_f64(t.get_tensor(Q.ACT, k)) for k in range(10)]
    r["S"] = {k: torch.from_numpy(t.get_tensor(Q.STATE, k)) for k in range(1, 11)}
    r["I"] = {k: t.get_tensor(Q.IDX, k) for k in Q.POOLED}
    r["G"] = {k: TR.bf16_bits_to_f64(t.get_tensor(Q.GRAD, k)) for k in range(1, 11)}
    r["Wq"] = [TR.bf16_bits_to_f64(t.get_packed(k)) for k in range(1, 11)]
    r["bq"] = [t.get_qbias(k) for k in range(1, 11)]
    r["wexp"], r["ql"], r["stats"] = t.weight_exponents(), t.quantized_layers(), t.act_stats()
    r["layers"] = [t.get_layer(k) for k in range(1, 11)]
    r["grads"], r["everything"] = all_grads(t), everything(t)
    t.close()
    return r


@functools.lru_cache(maxsize=None)
def restated(tag, eset):
    """the float64 restatement's forward of the case"""
    return QR.forward(QR.quantize_masters(QC.weights(tag)), QC.images(tag), QC.exponents(tag, eset))


def assert_quantised_as_prep(t, what):
    """get_packed, bq, the exponents and quantized_layers() against prep.quantize_folded of the masters the handle holds"""
    from yolo355 import prep
    masters = [t.get_layer(k) for k in range(1, 11)]
    want = prep.quantize_folded(masters)
    got, wexp = t.quantized_layers(), t.weight_exponents()
    for k, (L, M) in enumerate(zip(want, got), 1):
        assert (L["e_w"], L["e_b"]) == (M["e_w"], M["e_b"]) == wexp[k - 1], (what, k)
        assert QC.exact_exponent(np.abs(masters[k - 1][0]).max()) == L["e_w"] and QC.exact_exponent(np.abs(masters[k - 1][1]).max()) == L["e_b"]
        assert np.array_equal(L["q_w"], M["q_w"]) and np.array_equal(L["q_b"], M["q_b"]), (what, k)
        assert M["q_w"].dtype == np.int32 and np.abs(M["q_w"]).max() <= 127 and np.abs(M["q_b"]).max() <= 127
        assert np.array_equal(TR.bf16_bits_to_f64(t.get_packed(k)).numpy(), np.ldexp(L["q_w"].astype(np.float64), -L["e_w"])), (what, k)
        assert same(t.get_qbias(k), np.ldexp(L["q_b"].astype(np.float32), -L["e_b"]).astype(np.float32)), (what, k)
    return masters


# ------------------------------------------------------------------------------------------------------------ the forward
@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_forward_is_the_integer_oracle_bit_for_bit(tag, eset):
    """A_0 = fq(x); A_k 2^e_a[k], k = 1..9, and P 2^e_a[10] are the oracle's saturated maps; the state bytes are the
    restatement's (S_10 padded with zeros; I_k is S_k); act_stats is the oracle's sat and the maxima its trackers saw"""
    QC.check(tag, eset)
    r, o, f, sa = run(tag, eset), QC.oracle(tag, eset), restated(tag, eset), QC.exponents(tag, eset)
    assert torch.equal(r["A"][0][:, :3], f["A"][0]) and not r["A"][0][:, 3:].any()
    for k in range(1, 10):
        assert np.array_equal(np.ldexp(r["A"][k].numpy(), sa[k]), o["maps"][k - 1].astype(np.float64)), (tag, eset, k)
    assert r["P"].dtype == np.float32 and np.array_equal(np.ldexp(r["P"].astype(np.float64), sa[10]), o["pred_q"].astype(np.float64))
    cout = r["P"].shape[1]
    for k in range(1, 11):
        got = r["S"][k]
        if k == 10:
            assert got.shape[1] >= 32 and got.shape[1] & (got.shape[1] - 1) == 0 and not got[:, cout:].any()
            got = got[:, :cout]
        bad = got != f["S"][k]
        assert not bad.any(), (tag, eset, k, int(bad.sum()), torch.nonzero(bad)[:5].tolist())
    for k, i in r["I"].items():
        assert np.array_equal(i, r["S"][k].numpy())
    mx, clipped = r["stats"]
    assert clipped.tolist() == list(o["sat"]), (clipped.tolist(), o["sat"])
    assert same(mx, o["max_abs"]), (mx, o["max_abs"])
    if eset == "cal+1" and tag in QC.CLIP_TAGS:
        print(tag, "clipped share per tracker", [round(c / max(n, 1), 5) for c, n in zip(clipped.tolist(), [r["A"][0][:, :3].numel()] + [
            r["A"][k].numel() * (4 if TC.POOL[k - 1] else 1) for k in range(1, 10)] + [r["P"].size])])


def test_every_tracker_clips_on_the_gpu_in_one_of_the_clip_cases():
    got = np.array([run(tag, "cal+1")["stats"][1] for tag in QC.CLIP_TAGS])
    assert (got.max(0) > 0).all(), got.tolist()


@pytest.mark.parametrize("eset", QC.SETS)
def test_the_int8_engine_computes_the_same_maps(eset):
    """t64_b2_c20: Engine.load_quantized(quantized_layers()) + set_act_exponents(act_exponents()).  The engine's default
    forward (fused front end and conv3 pair, whose inner maps stay on chip): the maps it writes, P among them; then one launch
    per layer so that every map is written: get_feature(0..9) are A_1..A_9 and P as integers"""
    from yolo355 import _ffi
    from yolo355.engine import Engine
    tag = QC.ENGINE_TAG
    size, B, C = QC.CASES[tag]
    r, sa = run(tag, eset), QC.exponents(tag, eset)
    t = trainer(tag, eset)
    assert t.act_exponents() == sa
    eng = Engine(size, C, QC.ANCHORS, max_batch=B)
    eng.load_quantized(t.quantized_layers())
    eng.set_act_exponents(t.act_exponents())
    t.close()
    want = [np.ldexp(r["A"][k].numpy(), sa[k]).astype(np.int8) for k in range(1, 10)] + [np.ldexp(r["P"].astype(np.float64), sa[10]).astype(np.int8)]
    x = QC.images(tag)
    eng.forward(x)
    for k in (1, 3, 4, 5, 6, 7, 8, 9):                        # 0 and 2 are the fused launches' inner maps
        assert np.array_equal(eng.get_feature(k, B), want[k]), (eset, "default forward", k)
    eng.set_option(_ffi.OPT_FUSE_FRONT, 0)
    eng.set_option(_ffi.OPT_FUSE_PAIRS, 0)
    eng.forward(x)
    for k in range(10):
        assert np.array_equal(eng.get_feature(k, B), want[k]), (eset, k)
    eng.close()


# ------------------------------------------------------------------------------------------------------------ the weights
def test_weights_are_quantised_as_prep_quantize_folded_before_and_after_steps():
    """after the load, after every one of two SGD steps, and after a second load of one layer"""
    tag = "t48x80_b3_c2"
    t = trainer(tag, lr=3e-4)
    first = assert_quantised_as_prep(t, "loaded")
    assert all(same(m[0], w) and same(m[1], b) for m, (w, b) in zip(first, QC.weights(tag)))
    x, labels = dev(QC.images(tag)), QC.labels(tag)
    before = t.get_packed(5).copy()
    for it in range(2):
        t.step(x, labels)
        assert_quantised_as_prep(t, "step %d" % it)
    assert not same(t.get_packed(5), before) or not same(t.get_layer(5)[0], first[4][0])
    w, b = QC.weights(tag)[2]
    t.load_layer(3, w * np.float32(3.0), np.zeros_like(b))       # another scale, and an all-zero tensor: e = 0, q = 0
    assert t.weight_exponents()[2][1] == 0 and not t.get_qbias(3).any()
    assert t.weight_exponents()[2][0] == QC.exact_exponent(np.abs(w * np.float32(3.0)).max())
    q3 = t.quantized_layers()[2]
    assert q3["e_b"] == 0 and not q3["q_b"].any() and np.array_equal(q3["q_w"], QR.quantize_tensor(w * np.float32(3.0))[0])
    t.close()


# ------------------------------------------------------------------------------------------------------------ per op: backward
@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_data_gradients_per_element(tag, eset):
    """G_10 == rb(dP [not clipped]) exactly (padding channels zero).  Every G_{k-1} from the handle's G_k, Wq_k and S_{k-1}:
    exactly 0 at clipped elements and at positions the pool did not select; elsewhere within [rb(z - e), rb(z + e)],
    e = 2 K u S 1.001 + u |z|, K = 9 Cout (tests/test_train.py's interval), z with slope 0.125 exactly where bit 2 is set --
    among them elements whose A is 0 on either side"""
    r = run(tag, eset)
    cout10 = r["dP"].shape[1]
    keep10 = ((r["S"][10][:, :cout10].long() & QR.S_CLIP) == 0).double()
    assert torch.equal(r["G"][10][:, :cout10], BL.rb(torch.from_numpy(r["dP"]).double() * keep10)) and not r["G"][10][:, cout10:].any()
    zero_pos = zero_neg = 0
    for k in range(10, 1, -1):
        cout = cout10 if k == 10 else r["Wq"][k - 1].shape[0]
        G, Wq, Sp = r["G"][k][:, :cout], r["Wq"][k - 1], r["S"][k - 1]
        fac = QR.state_factor(Sp)
        z = TR.dgrad(G, Wq) * fac
        S = TR.dgrad(G.abs(), Wq.abs()) * fac * 1.001
        e = 2 * (9 * cout) * U * S * 1.001 + U * z.abs()
        got = r["G"][k - 1]
        if TC.POOL[k - 2]:
            gw = TR.windows(got)
            pos = (Sp.long() & QR.S_POS).unsqueeze(-1)
            others = gw.masked_fill(torch.arange(4).view(1, 1, 1, 1, 4) == pos, 0.0)
            assert not others.any(), (tag, k, "a position the pool did not select is not zero")
            got = torch.gather(gw, -1, pos).squeeze(-1)
        assert got.shape == z.shape
        clipped = (Sp.long() & QR.S_CLIP) != 0
        assert not got[clipped].any(), (tag, k, "a clipped element carries a gradient")
        lo, hi = BL.rb(z - e), BL.rb(z + e)
        bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
        print(tag, eset, "dgrad of layer", k, "n %d bad %d exact %.3f clipped %d" % (got.numel(), int(bad.sum()), float((got == BL.rb(z)).double().mean()), int(clipped.sum())))
        assert not bad.any(), (tag, k, int(bad.sum()), torch.nonzero(bad)[:5].tolist())
        zero = (r["A"][k - 1] == 0) & (got != 0)
        zero_neg += int((zero & ((Sp.long() & QR.S_NEG) != 0)).sum())
        zero_pos += int((zero & ((Sp.long() & QR.S_NEG) == 0)).sum())
    if tag in ("t48x80_b3_c2", "t64_b2_c20"):
        assert zero_pos > 0 and zero_neg > 0, (zero_pos, zero_neg)


@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_weight_and_bias_gradients_per_element(tag, eset):
    """from the handle's G_k and the quantised A_{k-1} in float64: |got - z| <= 2 K u S 1.001, K = B H W, S = sum |G| |A|"""
    r = run(tag, eset)
    for k in range(1, 11):
        dw, db = r["grads"][k - 1]
        cout, cin = dw.shape[:2]
        G, Ap = r["G"][k][:, :cout], r["A"][k - 1][:, :cin]
        K = G.shape[0] * G.shape[2] * G.shape[3]
        zw, zb = TR.wgrad(G, Ap)
        Sw, Sb = TR.wgrad(G.abs(), Ap.abs())
        for what, got, z, S in (("dw", dw, zw, Sw), ("db", db, zb, Sb)):
            err = (torch.from_numpy(got).double() - z).abs()
            bound = 2 * K * U * S * 1.001
            print(tag, eset, "layer", k, what, "K %d max err / bound %.3g" % (K, float((err / bound.clamp(min=1e-300)).max())))
            assert bool((err <= bound).all()), (tag, k, what, float(err.max()), torch.nonzero(err > bound)[:3].tolist())
        assert float(zw.abs().max()) > 0 and np.isfinite(dw).all()


# ------------------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_losses_are_the_gradient_library_s_on_the_handle_s_map(tag, eset):
    from yolo355 import grad as G
    r = run(tag, eset)
    size, B, C = QC.CASES[tag]
    h = G.YoloLossGrad(size, 16, QC.ANCHORS, C, max_batch=B, max_labels_per_image=1024)
    h.set_labels(QC.labels(tag))
    out, _, grads = h.forward_backward([dev(r["P"])])
    assert same(out, r["losses"]) and same(grads[0].cpu().numpy(), r["dP"])
    assert [np.float32(v) for v in out] == [np.float32(v) for v in r["loss_tensors"]]
    h.close()


@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_gradients_against_the_float64_straight_through_backward(tag, eset):
    """every layer's dW and db within a relative L2 distance of 2 * emu_relerr + 1e-6 of the restatement's float64
    straight-through backward from the handle's own dP, emu_relerr being the distance of the CPU emulation that rounds every
    G_k to bf16 (float64 sums) from the same float64 backward -- as tests/test_train.py takes its tolerance.

    Measured on one MI355X, relative L2 distance from the float64 backward over the ten layers (the emulation's in brackets is
    the same to the digits shown unless stated; the bound is twice the emulation's):
      t48x80_b3_c2   cal    dw 9.0e-4 .. 4.9e-3   db 6.1e-4 .. 4.3e-3   (at most 1.03 x the emulation's)
      t48x80_b3_c2   cal+1  dw 9.3e-4 .. 5.5e-3   db 6.9e-4 .. 5.3e-3   (at most 1.16 x)
      t64_b2_c20     cal    dw 9.7e-4 .. 5.1e-3   db 8.3e-4 .. 4.6e-3
      t64_b2_c20     cal+1  dw 8.6e-4 .. 5.3e-3   db 5.1e-4 .. 4.7e-3
      t16_b5_c2      cal    dw 1.1e-3 .. 4.7e-3   db 1.1e-3 .. 3.5e-3
      t16_b5_c2      cal+1  dw 5.3e-4 .. 6.0e-3   db 5.3e-4 .. 5.7e-3
      t16x32_b3_c20  cal    dw 1.2e-3 .. 4.3e-3   db 1.1e-3 .. 3.7e-3
      t16x32_b3_c20  cal+1  dw 9.9e-4 .. 4.3e-3   db 8.7e-4 .. 2.8e-3
    The largest distance is conv1's in every case, the smallest pred's: the roundings of G add up down the stack."""
    r, f = run(tag, eset), restated(tag, eset)
    ql = QR.quantize_masters(QC.weights(tag))
    exact, _ = QR.backward(ql, f["A"], f["S"], r["dP"])
    emu, _ = QR.backward(ql, f["A"], f["S"], r["dP"], round_g=True)
    worst = []
    for k, name in enumerate(TC.LAYERS, 1):
        dw, db = r["grads"][k - 1]
        rel = (TC.rel_l2(emu[k - 1][0].numpy(), exact[k - 1][0].numpy()), TC.rel_l2(emu[k - 1][1].numpy(), exact[k - 1][1].numpy()))
        got = (TC.rel_l2(dw, exact[k - 1][0].numpy()), TC.rel_l2(db, exact[k - 1][1].numpy()))
        print("DIST", tag, eset, name, "dw %.4g (emulation %.4g)  db %.4g (emulation %.4g)" % (got[0], rel[0], got[1], rel[1]))
        if got[0] > 2 * rel[0] + 1e-6 or got[1] > 2 * rel[1] + 1e-6:
            worst.append((name, got, rel))
    assert not worst, worst


def test_sgd_is_the_numpy_restatement_bit_for_bit():
    """three steps: masters and momentum equal train_ref.sgd fed with the handle's own gradients; the packed weights, bq and
    the exponents equal the restatement's quantiser on those masters"""
    tag = "t48x80_b3_c2"
    lr, mom, wd = 3e-4, 0.9, 5e-4
    t = trainer(tag, "cal+1", lr=lr)
    x, labels = dev(QC.images(tag)), QC.labels(tag)
    p = [t.get_layer(k) for k in range(1, 11)]
    m = [(None, None)] * 10
    for it in range(3):
        t.forward_backward(x, labels)
        g = all_grads(t)
        t.update()
        wexp = t.weight_exponents()
        for k in range(10):
            w, mw = TR.sgd(p[k][0], g[k][0], m[k][0], lr, mom, wd, it == 0)
            b, mb = TR.sgd(p[k][1], g[k][1], m[k][1], lr, mom, wd, it == 0)
            gw, gb = t.get_layer(k + 1)
            gmw, gmb = t.get_momentum(k + 1)
            assert same(gw, w) and same(gb, b), (it, k, "parameters")
            assert same(gmw, mw) and same(gmb, mb), (it, k, "momentum")
            (qw, ew), (qb, eb) = QR.quantize_tensor(w), QR.quantize_tensor(b)
            assert wexp[k] == (ew, eb), (it, k, "exponents")
            assert np.array_equal(TR.bf16_bits_to_f64(t.get_packed(k + 1)).numpy(), np.ldexp(qw.astype(np.float64), -ew)), (it, k, "packed weights")
            assert same(t.get_qbias(k + 1), np.ldexp(qb.astype(np.float32), -eb).astype(np.float32)), (it, k, "bq")
            assert not same(w, p[k][0])
            p[k], m[k] = (w, b), (mw, mb)
        assert same_grads(all_grads(t), g)                                     # the update leaves the gradients as they were
    t.close()


@pytest.mark.parametrize("tag,eset", [("t48x80_b3_c2", "cal"), ("t64_b2_c20", "cal+1")], ids=["t48x80_b3_c2-cal", "t64_b2_c20-cal+1"])
def test_two_runs_give_the_same_bits(tag, eset):
    r = run(tag, eset)
    t = trainer(tag, eset)
    x = dev(QC.images(tag))
    for _ in range(2):
        t.forward_backward(x, QC.labels(tag))
        got = everything(t)
        assert all(same(a, b) for a, b in zip(got, r["everything"])), [i for i, (a, b) in enumerate(zip(got, r["everything"])) if not same(a, b)]
    t.close()


def test_two_runs_of_a_deep_case_give_the_same_bits():
    """t240x272_b9_c20 (every weight-gradient run longer than one step, the statistics' atomics from thousands of waves), at
    the exponents of t64_b2_c20's calibration plus one so that maps clip: gradients, losses, statistics and P twice"""
    tag = QC.DEEP_TAG
    t = trainer(tag, exps=QC.exponents("t64_b2_c20", "cal+1"))
    x, labels = dev(QC.images(tag)), QC.labels(tag)
    out = []
    for _ in range(2):
        t.forward_backward(x, labels)
        out.append(all_grads(t) + [(np.array(t.losses), t.pred().cpu().numpy().copy())] + [t.act_stats()])
    t.close()
    assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(out[0], out[1]))
    assert out[0][-1][1].sum() > 0 and np.isfinite(out[0][-2][0]).all()


def test_set_grid_equals_fresh_handles():
    """one handle built for 96 x 160, switched 64 x 64 -> 96 x 160 -> 64 x 64; the exponents stay"""
    from yolo355 import synth
    tag = "t96x160_b1"
    exps = QC.exponents("t48x80_b3_c2", "cal+1")
    x = {(64, 64): dev(synth.make_images(77, 1, 64, 64, "noise")), (96, 160): dev(TC.images(tag))}
    labels = TC.labels(tag)
    want = {}
    for size in x:
        f = trainer(tag, size=list(size), exps=exps)
        f.forward_backward(x[size], labels)
        want[size] = everything(f)
        f.close()
    t = trainer(tag, exps=exps)
    for size in ((64, 64), (96, 160), (64, 64)):
        t.set_grid(list(size))
        assert t.act_exponents() == exps
        t.forward_backward(x[size], labels)
        got = everything(t)
        assert all(same(a, b) for a, b in zip(got, want[size])), size
    t.close()


def test_state_round_trip_gives_the_same_next_step():
    """state_dict() holds the fp32 masters and the trackers' buffers under the reference's keys; a trainer loaded from it takes
    its exponents from them and makes the same next step"""
    from yolo355 import prep, qtrain as Q
    tag = "t64_b2_c20"
    x, labels = dev(QC.images(tag)), QC.labels(tag)
    a = trainer(tag)
    tr = [prep.RangeTracker(scale=torch.tensor([2.0 ** e * 1.25]), first_a=1) for e in QC.exponents(tag, "cal")]
    a.set_act_exponents(tr)
    a.step(x, labels)
    sd = a.state_dict()
    keys = [k for i in range(1, 11) for k in TC.keys(i)] + [n + s for n in Q.TRACKER_NAMES for s in (".scale", ".first_a")]
    assert sorted(sd) == sorted(keys) and all(v.dtype == torch.float32 and not v.is_cuda for v in sd.values())
    size, B, C = QC.CASES[tag]
    b = Q.SlimQatTrainer(size, C, QC.ANCHORS, B, 1e-3)
    with pytest.raises(Exception, match="y355_qtrain_forward: the activation exponents are not set"):
        b.forward(x)
    b.load_state_dict(sd)
    assert b.act_exponents() == QC.exponents(tag, "cal")
    c = trainer(tag, ws=[(sd[TC.keys(k)[0]].numpy(), sd[TC.keys(k)[1]].numpy()) for k in range(1, 11)])
    lb, lc = b.step(x, labels), c.step(x, labels)
    assert [float(v) for v in lb] == [float(v) for v in lc] and same_grads(all_grads(b), all_grads(c))
    for k in range(1, 11):
        assert all(same(u, v) for u, v in zip(b.get_layer(k), c.get_layer(k))) and same(b.get_packed(k), c.get_packed(k))
    la = a.forward_backward(x, labels)                        # the trainer that went on without the round trip: the same forward
    assert [float(v) for v in la] == [float(v) for v in lb]
    for t in (a, b, c):
        t.close()


def test_update_trackers_sets_the_next_forward_s_exponents():
    """the maxima of a forward go through prep.RangeTracker on the host: the first call takes 127 / max, the next ones the
    moving average; the exponents hold for the NEXT forward (one step later than the reference's order)"""
    from yolo355 import prep
    tag = "t16x32_b3_c20"
    t = trainer(tag, "cal")
    x = dev(QC.images(tag))
    t.forward(x)
    mx, clipped = t.act_stats()
    assert same(mx, QC.oracle(tag, "cal")["max_abs"]) and not clipped.any()
    e = t.update_trackers()                                   # the first call: the maxima of the calibration batch themselves
    ref = [prep.RangeTracker() for _ in range(11)]
    assert e == [tr.update(float(m), False) for tr, m in zip(ref, mx)] == t.act_exponents() == QC.exponents(tag, "cal")
    t.set_act_exponents(QC.exponents(tag, "cal+1"))           # (the caller's own exponents leave the trackers as they are)
    t.forward(x)
    assert same(t.pred().cpu().numpy(), run(tag, "cal+1")["P"]) and t.act_stats()[1].sum() > 0
    e2 = t.update_trackers()
    assert e2 == [tr.update(float(m), False) for tr, m in zip(ref, t.act_stats()[0])] and len(t.state_dict()) == 20 + 22
    assert t.update_trackers(freeze=True) == e2
    t.close()


def test_refusals_leave_the_handle_usable():
    from yolo355 import _ffi, qtrain as Q
    tag = "t48x80_b3_c2"
    size, B, C = QC.CASES[tag]
    t = Q.SlimQatTrainer(size, C, QC.ANCHORS, B, 1e-3)
    t.load_weights(QC.weights(tag))
    x = dev(QC.images(tag))
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_forward: the activation exponents are not set"):
        t.forward(x)
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_get_act_exponents: the activation exponents are not set"):
        t.act_exponents()
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_set_act_exponents: an exponent beyond"):
        t.set_act_exponents([0] * 10 + [97])
    with pytest.raises(ValueError):
        t.set_act_exponents([0] * 10)
    t.set_act_exponents(QC.exponents(tag, "cal"))
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_backward: no forward pass has run at this size"):
        t.backward(torch.zeros(3, 35, 3, 5, device="cuda"))
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_get_act_stats: no forward pass has run at this size"):
        t.act_stats()
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_sgd_step: no backward pass has run"):
        t.update()
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_set_size: height and width must be multiples of 16"):
        t.set_grid([40, 80])
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_set_size: size beyond the handle's maximum"):
        t.set_grid([64, 80])
    assert t.input_size == [48, 80]
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_forward: batch must be 1..max_batch"):
        t.forward(torch.cat([x, x[:1]]))
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_layer_shape: layer index must be 1..10"):
        t.load_layer(11, np.zeros((1, 1, 3, 3), np.float32), np.zeros(1, np.float32))
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_get_qbias: layer index must be 1..10"):
        t._call("get_qbias", 0, None)
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_tensor_shape: no such tensor"):
        t.get_tensor(Q.STATE, 11)
    with pytest.raises(_ffi.Y355Error, match="y355_qtrain_tensor_shape: no such tensor"):
        t.get_tensor(Q.STATE, 0)
    w = np.zeros((16, 3, 3, 3), np.float32)
    assert t._lib.y355_qtrain_load_layer(t._h, 0, w.ctypes.data, w.ctypes.data) == -1
    assert t._lib.y355_qtrain_last_error().decode() == "y355_qtrain_load_layer: layer index must be 1..10"
    with pytest.raises(ValueError):
        t.forward(x[:, :, :32])
    t.forward_backward(x, QC.labels(tag))
    assert same_grads(all_grads(t), run(tag, "cal")["grads"])
    t.close()


def test_from_model_and_step_frame_list():
    from yolo355 import synth, qtrain as Q
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2_quantize_bnfuse
    tag = "t64_b2_c20"
    size, B, C = QC.CASES[tag]
    model = SlimYOLOv2_quantize_bnfuse("cuda:0", input_size=size, num_classes=C, trainable=True, anchor_size=QC.ANCHORS)
    model.load_state_dict(TC.state_dict(QC.weights(tag)), strict=False)
    frames = [f for f in synth.make_frames_u8(5, B, 50, 70, "blocks")]
    labels = [np.array(l, np.float64).reshape(-1, 5) for l in QC.labels(tag)]
    out = []
    for _ in range(2):
        t = Q.SlimQatTrainer.from_model(model, B, 1e-4)
        assert all(same(t.get_layer(k)[0], QC.weights(tag)[k - 1][0]) for k in range(1, 11)) and t.input_size == size
        with pytest.raises(Exception, match="the activation exponents are not set"):      # an uncalibrated model: nothing to take
            t.act_exponents()
        t.set_act_exponents(QC.exponents(tag, "cal"))
        losses = t.step_frame_list(frames, labels, seed=3)
        out.append(([float(v) for v in losses], [t.get_layer(k)[0] for k in (1, 10)]))
        assert all(v.dtype == torch.float32 and v.dim() == 0 for v in losses) and np.isfinite(out[-1][0]).all()
        assert not same(t.get_layer(10)[0], QC.weights(tag)[9][0])
        t.close()
    assert out[0][0] == out[1][0] and all(same(u, v) for u, v in zip(out[0][1], out[1][1]))


def test_two_handles_in_one_process():
    """each gives what it gives alone, interleaved"""
    pairs = (("t48x80_b3_c2", "cal+1"), ("t64_b2_c20", "cal"))
    ts = [trainer(tag, eset) for tag, eset in pairs]
    xs = [dev(QC.images(tag)) for tag, _ in pairs]
    for _ in range(2):
        for t, (tag, eset), x in zip(ts, pairs, xs):
            t.forward_backward(x, QC.labels(tag))
        for t, (tag, eset) in zip(ts, pairs):
            assert all(same(a, b) for a, b in zip(everything(t), run(tag, eset)["everything"]))
    for t in ts:
        t.close()


def test_overfit_run_and_the_engine_deploys_what_was_trained():
    """30 steps on one fixed batch of t64_b2_c20 at lr 1e-4, the rate at which the loss of the CPU restatement
    (qtrain_ref.emulate_steps: exact forward, G rounded to bf16; 49 s, so not run here) falls from 38.98 to 11.50: the loss of the
    quantised forward falls by at least 30 %; then the int8 Engine loaded from quantized_layers() reproduces the trainer's P of
    the trained network exactly, and every feature map"""
    from yolo355 import _ffi
    from yolo355.engine import Engine
    tag = QC.ENGINE_TAG
    size, B, C = QC.CASES[tag]
    sa = QC.exponents(tag, "cal")
    t = trainer(tag, lr=1e-4)
    x, labels = dev(QC.images(tag)), QC.labels(tag)
    got = [float(t.step(x, labels)[3]) for _ in range(30)]
    print("gpu lr 1e-4", got)
    assert np.isfinite(got).all() and got[-1] <= 0.7 * got[0]
    P = t.forward(x).cpu().numpy()
    assert not same(P, run(tag, "cal")["P"])
    from yolo355 import qtrain as Q
    A = [np.ldexp(TR.bf16_bits_to_f64(t.get_tensor(Q.ACT, k)).numpy(), sa[k]).astype(np.int8) for k in range(1, 10)]
    eng = Engine(size, C, QC.ANCHORS, max_batch=B)
    eng.load_quantized(t.quantized_layers())
    eng.set_act_exponents(t.act_exponents())
    eng.set_option(_ffi.OPT_FUSE_FRONT, 0)
    eng.set_option(_ffi.OPT_FUSE_PAIRS, 0)
    eng.forward(QC.images(tag))
    for k in range(9):
        assert np.array_equal(eng.get_feature(k, B), A[k]), k
    pq = eng.get_feature(9, B)
    assert same(np.ldexp(pq.astype(np.float32), -sa[10]).astype(np.float32), P)
    eng.close()
    t.close()
