"""The training step on the GPU (csrc/train.hip through yolo355/train.py) at the shapes of tests/train_cases.py.

Per op, from the engine's own tensors (nothing accumulates across layers; every element is checked): the forward
convolutions in the interval of tests/bf16_layer_ref.py, the stored pool positions, the data gradients, the weight and bias
gradients, G_10 == rb(dP), and the SGD update bit for bit against the NumPy restatement.  The whole step: the losses are
libyolo355_grad.so's on the engine's P, the gradients lie within 2 * emu_relerr + 1e-6 of the reference's own backward()
(tests/golden/train.npz), the same bits from run to run, set_size against fresh handles, the state round trip, an overfit
run, the refusals, and several handles in one process.

The weight gradient's long runs.  y355_train_backward cuts a layer's B H W pixels into at most max_runs runs of `chunk` pixels
(a multiple of 32); a wave walks its run in steps of 32 and train_reduce_kernel adds the runs.  At the first three cases every
chunk is 32 -- one step a wave, the cap never reached -- while every fine-tuning step (64 x 416 x 416, 32 x 240 x 320) has chunks
of 160 to 5408 pixels.  The two TC.DEEP cases sit just above the threshold of that regime (524 288 input pixels), and the tests
ask the live handle for the plan (SlimTrainer.wgrad_plan, the function the backward launches from) instead of restating it.
As y355_train_wgrad_plan printed them on an MI355X (layer: runs x chunk, last run):

  t416x448_b3_c2    1: 1942 x 288, 96    2: 1456 x 96, 96    3: 546 x 64, 64     4: 364 x 96, 96     5: 137 x 64, 32
                    6: 91 x 96, 96       7: 35 x 64, 8       8: 23 x 96, 72      9: 23 x 96, 72      10: 35 x 64, 8
  t240x272_b9_c20   1: 2040 x 288, 288   2: 1530 x 96, 96    3: 574 x 64, 48     4: 383 x 96, 48     5: 144 x 64, 28
                    6: 96 x 96, 60       7: 36 x 64, 55      8: 24 x 96, 87      9: 24 x 96, 87      10: 36 x 64, 55

On them: every per-op test; a sparse dP (K of the bound = the pixels where G_k is not zero, so a pixel dropped or taken twice
fails) with its probes on both sides of run and image boundaries; a one-hot dP whose dW_10 is A_9 bit for bit; the same bits
from run to run.  t16_b5_c2 and t16x32_b3_c20 have 1 x 1 and 1 x 2 maps at stride 16; a batch below max_batch runs on a handle
whose buffers hold an older, larger one.

Measured on one MI355X: the module (52 tests) in 9.9 s; its slowest new test is
test_forward_convolutions_per_element[t416x448_b3_c2], 2.0 s (float64 on the CPU), every other new one below 0.6 s."""
import functools
import os

import numpy as np
import pytest
import torch

import bf16_layer_ref as BL
import train_cases as TC
import train_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = TR.U
CIN = [3, 16, 32, 64, 64, 128, 128, 256, 256, 256]
DIV = [1, 2, 4, 4, 8, 8, 16, 16, 16, 16]                     # layer k's grid is the input's divided by DIV[k - 1]


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "train.npz")) as z:
        return {k: z[k] for k in z.files}


def trainer(tag, lr=1e-3, size=None, max_batch=None, ws=None):
    from yolo355 import train as T
    csize, B, C = TC.CASES[tag]
    t = T.SlimTrainer(size or csize, C, TC.ANCHORS, max_batch or B, lr)
    t.load_weights(ws if ws is not None else TC.weights(tag))
    return t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_grads(t):
    return [t.get_grad(k) for k in range(1, 11)]


def same_grads(a, b):
    return all(same(x[0], y[0]) and same(x[1], y[1]) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def run(tag):
    """one forward_backward of a case on a fresh trainer and everything the tests read from it: computed once, left unchanged"""
    from yolo355 import train as T
    t = trainer(tag)
    losses = t.forward_backward(dev(TC.images(tag)), TC.labels(tag))
    r = dict(losses=np.array(t.losses), loss_tensors=[float(v) for v in losses], P=t.pred().cpu().numpy().copy())
    r["dP"] = t._dpred.cpu().numpy().copy()
    r["A"] = [TR.bf16_bits_to_f64(t.get_tensor(T.ACT, k)) for k in range(10)]
    r["I"] = {k: torch.from_numpy(t.get_tensor(T.IDX, k)) for k in T.POOLED}
    r["G"] = {k: TR.bf16_bits_to_f64(t.get_tensor(T.GRAD, k)) for k in range(1, 11)}
    r["Wb"] = [TR.bf16_bits_to_f64(t.get_packed(k)) for k in range(1, 11)]
    r["layers"] = [t.get_layer(k) for k in range(1, 11)]
    r["grads"] = all_grads(t)
    r["plan"] = [t.wgrad_plan(k) for k in range(1, 11)]     # of the backward that has just run
    t.close()
    return r


# ------------------------------------------------------------------------------------------------------------ per op: forward
@pytest.mark.parametrize("tag", TC.TAGS)
def test_forward_convolutions_per_element(tag):
    """A_0 = rb(x) exactly; every A_k and P in the interval of its own op on the engine's A_{k-1}; every I_k a position whose
    z + e reaches the window's largest z - e, the first one where float64 ties exactly"""
    r = run(tag)
    x = torch.from_numpy(TC.images(tag)).double()
    assert torch.equal(r["A"][0][:, :3], BL.rb(x)) and not r["A"][0][:, 3:].any()
    for k in range(1, 11):
        w, b = TC.weights(tag)[k - 1]
        assert torch.equal(r["Wb"][k - 1], BL.rb(torch.from_numpy(w).double())), (k, "the packed weights are rb(W)")
        assert same(r["layers"][k - 1][0], w) and same(r["layers"][k - 1][1], b)
        o = dict(s2=0, k=3, act=None if k == 10 else 0.125, cin=CIN[k - 1])
        z, zc, S, e = BL.conv_terms(o, r["A"][k - 1][:, :CIN[k - 1]], r["Wb"][k - 1], b)
        pool = 1 if k < 10 and TC.POOL[k - 1] else 0
        got = torch.from_numpy(r["P"]).double() if k == 10 else r["A"][k]
        st = BL.interval_stats(got, z, e, S, pool, fp32_out=(k == 10))
        print(tag, "layer", k, "n %d bad %d exact %.3f rho_max %.3g" % (st["n"], st["bad"], st["exact"], st["rho_max"]))
        assert st["bad"] == 0, (tag, k, st)
        if pool:
            zw, ew = TR.windows(z), TR.windows(e)
            pos = r["I"][k].long()
            assert int(pos.max()) <= 3
            reach = torch.gather(zw + ew, -1, pos.unsqueeze(-1)).squeeze(-1) >= (zw - ew).amax(-1)
            assert bool(reach.all()), (tag, k, "a stored position that cannot hold the maximum", int((~reach).sum()))
            top = zw == zw.amax(-1, keepdim=True)
            tie = top.sum(-1) > 1
            first = torch.where(top, torch.arange(4).view(1, 1, 1, 1, 4), torch.tensor(4)).amin(-1)
            assert bool((pos[tie] == first[tie]).all()), (tag, k, "not the first of an exact tie")


# ------------------------------------------------------------------------------------------------------------ per op: backward
@pytest.mark.parametrize("tag", TC.TAGS)
def test_data_gradients_per_element(tag):
    """G_10 == rb(dP) exactly (padding channels zero); every G_{k-1} from the engine's G_k, rb(W_k), A_{k-1} and I_{k-1}: the
    selected position within [rb(z - e), rb(z + e)], e = 2 K u S 1.001 + u |z|, K = 9 Cout; every other position exactly 0"""
    r = run(tag)
    cout10 = r["dP"].shape[1]
    assert torch.equal(r["G"][10][:, :cout10], BL.rb(torch.from_numpy(r["dP"]).double())) and not r["G"][10][:, cout10:].any()
    for k in range(10, 1, -1):
        cout = cout10 if k == 10 else r["Wb"][k - 1].shape[0]
        G, Wb, Ap = r["G"][k][:, :cout], r["Wb"][k - 1], r["A"][k - 1]
        mask = TR.slope_mask(Ap)
        z = TR.dgrad(G, Wb) * mask
        S = TR.dgrad(G.abs(), Wb.abs()) * mask * 1.001
        e = 2 * (9 * cout) * U * S * 1.001 + U * z.abs()
        got = r["G"][k - 1]
        if TC.POOL[k - 2]:
            gw = TR.windows(got)
            pos = r["I"][k - 1].long().unsqueeze(-1)
            sel = torch.gather(gw, -1, pos).squeeze(-1)
            others = gw.masked_fill(torch.arange(4).view(1, 1, 1, 1, 4) == pos, 0.0)
            assert not others.any(), (tag, k, "a position the pool did not select is not zero")
            got = sel
        assert got.shape == z.shape
        lo, hi = BL.rb(z - e), BL.rb(z + e)
        bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
        print(tag, "dgrad of layer", k, "n %d bad %d exact %.3f" % (got.numel(), int(bad.sum()), float((got == BL.rb(z)).double().mean())))
        assert not bad.any(), (tag, k, int(bad.sum()), torch.nonzero(bad)[:5].tolist())


def assert_weight_gradients(tag, grads, G_of, A, support_only=False):
    """every dW_k and db_k against float64 from G_k (G_of(k)) and A_{k-1}: |got - z| <= 2 K u S 1.001, S = sum |G| |A|, K the
    number of pixels summed over -- B H W, or with support_only the pixels at which G_k has a nonzero channel (zeros add
    exactly).  Returns {k: the [B, H, W] support of G_k}."""
    support = {}
    for k in range(1, 11):
        dw, db = grads[k - 1]
        cout, cin = dw.shape[:2]
        G, Ap = G_of(k)[:, :cout], A[k - 1][:, :cin]
        support[k] = (G != 0).any(1)
        K = int(support[k].sum()) if support_only else G.shape[0] * G.shape[2] * G.shape[3]
        zw, zb = TR.wgrad(G, Ap)
        Sw, Sb = TR.wgrad(G.abs(), Ap.abs())
        for what, got, z, S in (("dw", dw, zw, Sw), ("db", db, zb, Sb)):
            err = (torch.from_numpy(got).double() - z).abs()
            bound = 2 * K * U * S * 1.001
            print(tag, "layer", k, what, "K %d max err / bound %.3g" % (K, float((err / bound.clamp(min=1e-300)).max())), "max |z| %.3g" % float(z.abs().max()))
            assert bool((err <= bound).all()), (tag, k, what, float(err.max()), torch.nonzero(err > bound)[:3].tolist())
        assert float(zw.abs().max()) > 0 and np.isfinite(dw).all()
    return support


@pytest.mark.parametrize("tag", TC.TAGS)
def test_weight_and_bias_gradients_per_element(tag):
    """from the engine's G_k and A_{k-1} in float64: |got - z| <= 2 K u S 1.001, K = B H W, S = sum |G| |A|"""
    r = run(tag)
    assert_weight_gradients(tag, r["grads"], lambda k: r["G"][k], r["A"])


# ------------------------------------------------------------------------------------------- the weight gradient's long runs
def last_run(p):
    return p["npix"] - (p["runs"] - 1) * p["chunk"]


def test_deep_cases_reach_the_long_run_regime():
    """asked of the live handles (y355_train_wgrad_plan): every layer of a deep case sums over runs of two or more 32-pixel
    steps in more than one run; over the two cases some layer's last run is shorter than the others and some layer's last
    run ends inside an 8-pixel group.  A condition on the inputs of the tests below."""
    lasts = []
    for tag in TC.DEEP:
        (h, w), B, _ = TC.CASES[tag]
        for k, p in enumerate(run(tag)["plan"], 1):
            print("PLAN", tag, "layer", k, "npix %d max_runs %d runs %d chunk %d last run %d" % (p["npix"], p["max_runs"], p["runs"], p["chunk"], last_run(p)))
            assert p["npix"] == B * (h // DIV[k - 1]) * (w // DIV[k - 1])
            assert p["chunk"] >= 64 and p["chunk"] % 32 == 0 and 1 < p["runs"] <= p["max_runs"] and 0 < last_run(p) <= p["chunk"]
            lasts.append((last_run(p), p["chunk"]))
    assert any(l < c for l, c in lasts) and any(l % 8 for l, c in lasts)
    for tag in TC.TAGS[:3]:                                  # what the first three cases never left
        assert all(p["chunk"] == 32 for p in run(tag)["plan"])


def probes(t, B, h, w):
    """stride-16 pixels (flat b, y, x) chosen from the plans of layers 10 and 8: the first pixel of image 0, the last of the
    last image, both sides of an image boundary, both sides of a run boundary of either plan, the first and the last pixel of
    either plan's last run"""
    hw, npix = h * w, B * h * w
    ps = {0, npix - 1, hw - 1, hw}
    for k in (10, 8):
        p = t.wgrad_plan(k)
        assert p["npix"] == npix and p["runs"] > 2
        mid = (p["runs"] // 2) * p["chunk"]
        ps |= {mid - 1, mid, (p["runs"] - 1) * p["chunk"], npix - 1}
    return sorted(ps)


def forwarded(tag):
    """a fresh trainer after one forward of the case: the tensors of run(tag)"""
    t = trainer(tag)
    P = t.forward(dev(TC.images(tag)))
    assert same(P.cpu().numpy(), run(tag)["P"])
    return t


@pytest.mark.parametrize("tag", TC.DEEP)
def test_sparse_upstream_gradient(tag):
    """dP zero but at a handful of stride-16 pixels (probes) that carry random values in every channel: dW_k and db_k of all
    ten layers against float64 from the engine's own G_k and A_{k-1}, with K the number of pixels at which G_k is not zero --
    a pixel of the support dropped or taken twice is outside the bound.  Every layer has a run boundary inside the support."""
    from yolo355 import synth, train as T
    (h, w), B, C = TC.CASES[tag]
    h, w = h // 16, w // 16
    r, t = run(tag), forwarded(tag)
    ps = probes(t, B, h, w)
    dP = np.zeros((B, 5 * (5 + C), h, w), np.float32)
    vals = synth.uniform_pm1(TC._seed(tag) + 7, (len(ps), dP.shape[1]))
    for i, p in enumerate(ps):
        dP[p // (h * w), :, p % (h * w) // w, p % w] = vals[i]
    t.backward(dev(dP))
    grads, plan = all_grads(t), [t.wgrad_plan(k) for k in range(1, 11)]
    assert plan == r["plan"]
    support = assert_weight_gradients(tag, grads, lambda k: TR.bf16_bits_to_f64(t.get_tensor(T.GRAD, k)), r["A"], support_only=True)
    t.close()
    assert int(support[10].sum()) == len(ps)
    for k in range(1, 11):
        s, c = support[k].reshape(-1), plan[k - 1]["chunk"]
        inside = sum(1 for i in range(1, plan[k - 1]["runs"]) if s[i * c - 1] and s[i * c])
        print("SUPPORT", tag, "layer", k, "pixels %d of %d, run boundaries inside it %d of %d" % (int(s.sum()), s.numel(), inside, plan[k - 1]["runs"] - 1))
        assert inside >= 1, (tag, k)


@pytest.mark.parametrize("tag", TC.DEEP)
def test_one_hot_upstream_gradient_bit_for_bit(tag):
    """dP is 1.0 at one probe pixel per prediction channel (the probes taken in turn): dW_10[c, ci, tap] is the element of A_9
    under that tap, or 0 in the padding, and db_10[c] is 1.0 -- sums of one nonzero term, so as bits (a -0.0 of A_9 comes out
    of the fp32 sum from +0.0 as +0.0)"""
    (h, w), B, C = TC.CASES[tag]
    h, w = h // 16, w // 16
    r, t = run(tag), forwarded(tag)
    ps = probes(t, B, h, w)
    cout = 5 * (5 + C)
    dP = np.zeros((B, cout, h, w), np.float32)
    A9 = np.pad(r["A"][9].numpy().astype(np.float32), ((0, 0), (0, 0), (1, 1), (1, 1)))
    want = np.zeros((cout, 256, 3, 3), np.float32)
    for c in range(cout):
        p = ps[c % len(ps)]
        b, y, x = p // (h * w), p % (h * w) // w, p % w
        dP[b, c, y, x] = 1.0
        want[c] = A9[b, :, y:y + 3, x:x + 3] + np.float32(0.0)
    t.backward(dev(dP))
    dw, db = t.get_grad(10)
    t.close()
    assert np.count_nonzero(want) > 0.5 * want.size                             # (the probes in corners have five taps in the padding)
    bad = np.argwhere(bits(dw) != bits(want))
    assert not len(bad), (tag, len(bad), bad[:5].tolist())
    assert same(db, np.ones(cout, np.float32))


@pytest.mark.parametrize("tag", TC.DEEP)
def test_two_runs_of_a_deep_case_give_the_same_bits(tag):
    """the order of the sum is fixed with the number of runs at or near its cap too"""
    r = run(tag)
    t = trainer(tag)
    x = dev(TC.images(tag))
    for _ in range(2):
        t.forward_backward(x, TC.labels(tag))
        assert same_grads(all_grads(t), r["grads"]) and same(t.losses, r["losses"])
    t.close()


def everything(t):
    """the gradients, losses and P of the last forward_backward and every tensor the handle hands out"""
    from yolo355 import train as T
    out = [g for pair in all_grads(t) for g in pair] + [np.array(t.losses), t.pred().cpu().numpy().copy()]
    out += [t.get_tensor(T.ACT, k) for k in range(10)] + [t.get_tensor(T.IDX, k) for k in T.POOLED] + [t.get_tensor(T.GRAD, k) for k in range(1, 11)]
    return out


@pytest.mark.parametrize("tag,sub", [("t48x80_b3_c2", (1, 2)), ("t16_b5_c2", (3, 5))], ids=["t48x80_b3_c2-1of3", "t16_b5_c2-2of5"])
def test_a_batch_below_max_batch_after_a_full_one(tag, sub):
    """a handle whose buffers hold the full batch runs images sub[0]:sub[1] of it: everything equals a fresh handle of that
    max_batch on the same images, bit for bit and in shape; then the full batch again equals its first run.  Two images of
    t16_b5_c2 are 2 stride-16 pixels, inside one 8-pixel group, with three older images behind them in every buffer."""
    r = run(tag)
    x, labels = dev(TC.images(tag)), TC.labels(tag)
    xs, ls = x[sub[0]:sub[1]].contiguous(), labels[sub[0]:sub[1]]
    f = trainer(tag, max_batch=sub[1] - sub[0])
    f.forward_backward(xs, ls)
    want = everything(f)
    f.close()
    assert want[-1].shape[0] == sub[1] - sub[0] and want[21].shape[0] == sub[1] - sub[0]
    t = trainer(tag)
    t.forward_backward(x, labels)
    first = everything(t)
    assert same_grads(all_grads(t), r["grads"]) and same(first[20], r["losses"]) and same(first[21], r["P"])
    t.forward_backward(xs, ls)
    got = everything(t)
    assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want)), [i for i, (a, b) in enumerate(zip(got, want)) if not same(a, b)]
    assert [p for p in (t.wgrad_plan(k) for k in range(1, 11))] == [t.wgrad_plan(k, sub[1] - sub[0]) for k in range(1, 11)]
    t.forward_backward(x, labels)
    again = everything(t)
    assert all(same(a, b) for a, b in zip(again, first)), [i for i, (a, b) in enumerate(zip(again, first)) if not same(a, b)]
    t.close()


def test_sgd_is_the_numpy_restatement_bit_for_bit():
    """three steps: parameters, momentum and the packed bf16 weights read back equal train_ref.sgd fed with the engine's own
    gradients"""
    tag = "t48x80_b3_c2"
    lr, mom, wd = 3e-4, 0.9, 5e-4
    t = trainer(tag, lr=lr)
    x, labels = dev(TC.images(tag)), TC.labels(tag)
    p = [t.get_layer(k) for k in range(1, 11)]
    m = [(None, None)] * 10
    for it in range(3):
        t.forward_backward(x, labels)
        g = all_grads(t)
        t.update()
        for k in range(10):
            w, mw = TR.sgd(p[k][0], g[k][0], m[k][0], lr, mom, wd, it == 0)
            b, mb = TR.sgd(p[k][1], g[k][1], m[k][1], lr, mom, wd, it == 0)
            gw, gb = t.get_layer(k + 1)
            gmw, gmb = t.get_momentum(k + 1)
            assert same(gw, w) and same(gb, b), (it, k, "parameters")
            assert same(gmw, mw) and same(gmb, mb), (it, k, "momentum")
            assert torch.equal(TR.bf16_bits_to_f64(t.get_packed(k + 1)), BL.rb(torch.from_numpy(w).double())), (it, k, "packed weights")
            assert not same(w, p[k][0])
            p[k], m[k] = (w, b), (mw, mb)
        assert same_grads(all_grads(t), g)                                     # the update leaves the gradients as they were
    t.close()


# ------------------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("tag", TC.TAGS)
def test_losses_are_the_gradient_library_s_on_the_engine_s_map(tag):
    from yolo355 import grad as G
    r = run(tag)
    size, B, C = TC.CASES[tag]
    h = G.YoloLossGrad(size, 16, TC.ANCHORS, C, max_batch=B, max_labels_per_image=1024)
    h.set_labels(TC.labels(tag))
    out, _, grads = h.forward_backward([dev(r["P"])])
    assert same(out, r["losses"]) and same(grads[0].cpu().numpy(), r["dP"])
    assert [np.float32(v) for v in out] == [np.float32(v) for v in r["loss_tensors"]]
    h.close()


@pytest.mark.parametrize("tag", TC.GOLDEN_TAGS)
def test_gradients_against_the_reference(gold, tag):
    """every layer within a relative L2 distance of 2 * emu_relerr + 1e-6 of the reference's own backward()"""
    r = run(tag)
    want = gold["train/%s/losses" % tag].astype(np.float64)
    print(tag, "losses", r["losses"], "reference", want)
    assert (np.abs(r["losses"] - want) <= 0.01 * np.abs(want)).all()
    worst = []
    for k, name in enumerate(TC.LAYERS, 1):
        dw, db = r["grads"][k - 1]
        rel = gold["train/%s/emu_relerr/%s" % (tag, name)]
        got = (TC.rel_l2(dw.reshape(-1)[TC.sample_index(dw.size, tag)], gold["train/%s/dw/%s" % (tag, name)]), TC.rel_l2(db, gold["train/%s/db/%s" % (tag, name)]))
        print("DIST", tag, name, "dw %.4g (emulation %.4g)  db %.4g (emulation %.4g)" % (got[0], rel[0], got[1], rel[1]))
        if got[0] > 2 * rel[0] + 1e-6 or got[1] > 2 * rel[1] + 1e-6:
            worst.append((name, got, tuple(rel)))
    assert not worst, worst


def test_two_runs_give_the_same_bits():
    tag = "t48x80_b3_c2"
    r = run(tag)
    t = trainer(tag)
    x = dev(TC.images(tag))
    for _ in range(2):
        t.forward_backward(x, TC.labels(tag))
        assert same_grads(all_grads(t), r["grads"]) and same(t.losses, r["losses"])
    t.close()


def test_set_size_equals_fresh_handles():
    """one handle built for 96 x 160, switched 64 x 64 -> 96 x 160 -> 64 x 64"""
    from yolo355 import synth
    tag = "t96x160_b1"
    ws, C = TC.weights(tag), TC.CASES[tag][2]
    x = {(64, 64): dev(synth.make_images(77, 1, 64, 64, "noise")), (96, 160): dev(TC.images(tag))}
    labels = TC.labels(tag)
    want = {}
    for size in x:
        f = trainer(tag, size=list(size))
        f.forward_backward(x[size], labels)
        want[size] = (all_grads(f), np.array(f.losses))
        f.close()
    assert same_grads(want[(96, 160)][0], run(tag)["grads"])
    t = trainer(tag)
    for size in ((64, 64), (96, 160), (64, 64)):
        t.set_grid(list(size))
        t.forward_backward(x[size], labels)
        assert same_grads(all_grads(t), want[size][0]) and same(np.array(t.losses), want[size][1]), size
    t.close()


def test_state_round_trip_gives_the_same_next_step():
    tag = "t64_b2_c20"
    x, labels = dev(TC.images(tag)), TC.labels(tag)
    a = trainer(tag)
    a.step(x, labels)
    sd = a.state_dict()
    assert sorted(sd) == sorted(k for i in range(1, 11) for k in TC.keys(i)) and all(v.dtype == torch.float32 and not v.is_cuda for v in sd.values())
    b = trainer(tag, ws=[(np.zeros_like(w), np.zeros_like(bb)) for w, bb in TC.weights(tag)])
    b.load_state_dict(sd)
    c = trainer(tag, ws=[(sd[TC.keys(k)[0]].numpy(), sd[TC.keys(k)[1]].numpy()) for k in range(1, 11)])
    lb, lc = b.step(x, labels), c.step(x, labels)
    assert [float(v) for v in lb] == [float(v) for v in lc] and same_grads(all_grads(b), all_grads(c))
    for k in range(1, 11):
        assert all(same(u, v) for u, v in zip(b.get_layer(k), c.get_layer(k)))
    # and the trainer that went on without the round trip: the same forward (its momentum differs from a fresh one's)
    la = a.forward_backward(x, labels)
    assert [float(v) for v in la] == [float(v) for v in lb]
    for t in (a, b, c):
        t.close()


def test_overfit_run_reduces_the_loss():
    """ten steps on one fixed batch; lr chosen on the CPU with the emulation so that ITS total loss falls by at least 30 %"""
    tag = "t64_b2_c20"
    size, B, C = TC.CASES[tag]
    target = TR.targets(size, TC.labels(tag))
    lr = None
    for cand in (1e-4, 2e-4, 5e-5, 4e-4):
        e = TR.emulate_steps(TC.weights(tag), TC.images(tag), target, size, C, cand, 10)
        print("emulation lr", cand, e)
        if np.isfinite(e).all() and e[-1] <= 0.7 * e[0]:
            lr = cand
            break
    assert lr is not None, "no candidate lr makes the emulation's loss fall by 30 %"
    t = trainer(tag, lr=lr)
    x, labels = dev(TC.images(tag)), TC.labels(tag)
    got = [float(t.step(x, labels)[3]) for _ in range(10)]
    print("gpu lr", lr, got)
    assert np.isfinite(got).all() and got[-1] < got[0]
    t.close()


def test_refusals_leave_the_handle_usable():
    from yolo355 import _ffi
    tag = "t48x80_b3_c2"
    t = trainer(tag)
    x = dev(TC.images(tag))
    with pytest.raises(_ffi.Y355Error, match="y355_train_backward: no forward pass has run at this size"):
        t.backward(torch.zeros(3, 35, 3, 5, device="cuda"))
    with pytest.raises(_ffi.Y355Error, match="y355_train_sgd_step: no backward pass has run"):
        t.update()
    with pytest.raises(_ffi.Y355Error, match="y355_train_set_size: height and width must be multiples of 16"):
        t.set_grid([40, 80])
    with pytest.raises(_ffi.Y355Error, match="y355_train_set_size: size beyond the handle's maximum"):
        t.set_grid([64, 80])
    assert t.input_size == [48, 80]
    with pytest.raises(_ffi.Y355Error, match="y355_train_forward: batch must be 1..max_batch"):
        t.forward(torch.cat([x, x[:1]]))
    with pytest.raises(_ffi.Y355Error, match="y355_train_layer_shape: layer index must be 1..10"):
        t.load_layer(11, np.zeros((1, 1, 3, 3), np.float32), np.zeros(1, np.float32))
    w = np.zeros((16, 3, 3, 3), np.float32)
    assert t._lib.y355_train_load_layer(t._h, 0, w.ctypes.data, w.ctypes.data) == -1
    assert t._lib.y355_train_last_error().decode() == "y355_train_load_layer: layer index must be 1..10"
    with pytest.raises(ValueError):
        t.forward(x[:, :, :32])
    t.forward_backward(x, TC.labels(tag))
    assert same_grads(all_grads(t), run(tag)["grads"])
    t.close()


def test_from_model_and_step_frame_list():
    from yolo355 import synth, train as T
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2_quantize_bnfuse
    tag = "t64_b2_c20"
    size, B, C = TC.CASES[tag]
    model = SlimYOLOv2_quantize_bnfuse("cuda:0", input_size=size, num_classes=C, trainable=True, anchor_size=TC.ANCHORS)
    model.load_state_dict(TC.state_dict(TC.weights(tag)), strict=False)
    frames = [f for f in synth.make_frames_u8(5, B, 50, 70, "blocks")]
    labels = [np.array(l, np.float64).reshape(-1, 5) for l in TC.labels(tag)]
    out = []
    for _ in range(2):
        t = T.SlimTrainer.from_model(model, B, 1e-4)
        assert all(same(t.get_layer(k)[0], TC.weights(tag)[k - 1][0]) for k in range(1, 11)) and t.input_size == size
        losses = t.step_frame_list(frames, labels, seed=3)
        out.append(([float(v) for v in losses], [t.get_layer(k)[0] for k in (1, 10)]))
        assert all(v.dtype == torch.float32 and v.dim() == 0 for v in losses) and np.isfinite(out[-1][0]).all()
        assert not same(t.get_layer(10)[0], TC.weights(tag)[9][0])
        t.close()
    assert out[0][0] == out[1][0] and all(same(u, v) for u, v in zip(out[0][1], out[1][1]))


def test_two_trainers_and_an_engine_in_one_process():
    """each gives what it gives alone"""
    from oracle import yolo_oracle as O
    from yolo355 import synth
    from yolo355.engine import Engine
    from yolo355.prep import RangeTracker
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0))
    xc, xe = synth.make_images(1, 1, 96, 96, "blocks"), synth.make_images(3, 2, 96, 96, "blocks")

    def engine():
        eng = Engine([96, 96], 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=2)
        eng.load_quantized(ql)
        eng.calibrate(xc, [RangeTracker() for _ in range(11)])
        return eng

    eng = engine()
    alone = eng.forward(xe)
    eng.close()
    tags = ("t48x80_b3_c2", "t64_b2_c20")
    ts = [trainer(tag) for tag in tags]
    eng = engine()
    xs = [dev(TC.images(tag)) for tag in tags]
    for t, tag, x in zip(ts, tags, xs):
        t.forward_backward(x, TC.labels(tag))
    dets = eng.forward(xe)
    for t, tag in zip(ts, tags):
        assert same_grads(all_grads(t), run(tag)["grads"]) and same(np.array(t.losses), run(tag)["losses"])
    for (b0, s0, c0), (b1, s1, c1) in zip(alone, dets):
        assert np.array_equal(b0, b1) and np.array_equal(s0, s1) and np.array_equal(c0, c1)
    ts[0].forward_backward(xs[0], TC.labels(tags[0]))                 # again, after the engine ran
    assert same_grads(all_grads(ts[0]), run(tags[0])["grads"])
    eng.close()
    for t in ts:
        t.close()
