"""The BatchNorm training step on the GPU (csrc/bntrain.hip through yolo355/bntrain.py) at the shapes of tests/bntrain_cases.py.

Per op, from the engine's own tensors (nothing accumulates across layers; every element is checked): Z_k and P in the
interval of tests/bf16_layer_ref.py; the batch and running statistics against float64 NumPy on the engine's Z_k within one
fp32 rounding widened by the float64 summation bound; A_k and I_k bit for bit against the NumPy fp32 restatement
(tests/bntrain_ref.py); dY_k by section 6m's data-gradient rule; dgamma and dbeta against float64 sums; G_k bit for bit; dW_k
and db_k by section 6m's rule; the SGD update of all four parameter kinds bit for bit.  The whole step: gradients within
2 * emu_relerr + 1e-6 of the reference's own backward() (tests/golden/bntrain.npz), the same bits from run to run, set_size
and smaller batches against fresh handles, the state round trip, the N < 2 refusal, an overfit run, the hand-over to the
folded trainer, several handles in one process, from_model and step_frame_list.

Measured distances from the reference and the reductions' plans are in DESIGN.md section 6n."""
import functools
import os

import numpy as np
import pytest
import torch

import bf16_layer_ref as BL
import bntrain_cases as BC
import bntrain_ref as BR
import train_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = TR.U
CIN = [3, 16, 32, 64, 64, 128, 128, 256, 256, 256]
DIV = BC.DIV


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "bntrain.npz")) as z:
        return {k: z[k] for k in z.files}


def load(t, layers):
    for k, L in enumerate(layers, 1):
        t.load_layer(k, L["w"], L["b"])
        if L["bn"]:
            t.load_bn(k, *L["bn"])


def trainer(tag, lr=1e-3, size=None, max_batch=None, layers=None):
    from yolo355 import bntrain as T
    csize, B, C = BC.CASES[tag]
    t = T.SlimBNTrainer(size or csize, C, BC.ANCHORS, max_batch or B, lr)
    load(t, layers if layers is not None else BC.params(tag))
    return t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_grads(t):
    """[dW, db] of layers 1..10, then [dgamma, dbeta] of layers 1..9, flat"""
    return [g for k in range(1, 11) for g in t.get_grad(k)] + [g for k in range(1, 10) for g in t.get_bn_grad(k)]


def same_lists(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


def everything(t):
    """gradients, losses, P, statistics, buffers and every tensor the handle hands out"""
    from yolo355 import bntrain as T
    out = all_grads(t) + [np.array(t.losses), t.pred().cpu().numpy().copy()]
    out += [s for k in range(1, 10) for s in t.batch_stats(k)] + [s for k in range(1, 10) for s in t.get_bn(k)[2:4]]
    out += [t.get_tensor(T.ACT, k) for k in range(10)] + [t.get_tensor(T.IDX, k) for k in T.POOLED]
    out += [t.get_tensor(kind, k) for kind in (T.Z, T.DY) for k in range(1, 10)] + [t.get_tensor(T.GRAD, k) for k in range(1, 11)]
    return out


@functools.lru_cache(maxsize=None)
def run(tag):
    """one forward_backward of a case on a fresh trainer and everything the tests read from it: computed once, left unchanged"""
    from yolo355 import bntrain as T
    t = trainer(tag)
    losses = t.forward_backward(dev(BC.images(tag)), BC.labels(tag))
    r = dict(losses=np.array(t.losses), loss_tensors=[float(v) for v in losses], P=t.pred().cpu().numpy().copy())
    r["dP"] = t._dpred.cpu().numpy().copy()
    r["A"] = [t.get_tensor(T.ACT, k) for k in range(10)]                          # bf16 bits
    r["I"] = {k: t.get_tensor(T.IDX, k) for k in T.POOLED}
    r["Z"] = {k: BR.bits_to_f32(t.get_tensor(T.Z, k)) for k in range(1, 10)}       # float32 (exact)
    r["DY"] = {k: BR.bits_to_f32(t.get_tensor(T.DY, k)) for k in range(1, 10)}
    r["G"] = {k: t.get_tensor(T.GRAD, k) for k in range(1, 11)}                    # bf16 bits
    r["Wb"] = [TR.bf16_bits_to_f64(t.get_packed(k)) for k in range(1, 11)]
    r["stats"] = {k: t.batch_stats(k) for k in range(1, 10)}
    r["bn"] = {k: t.get_bn(k) for k in range(1, 10)}
    r["grads"] = [t.get_grad(k) for k in range(1, 11)]
    r["bn_grads"] = {k: t.get_bn_grad(k) for k in range(1, 10)}
    r["flat"] = all_grads(t)
    r["plan"] = {k: t.stats_plan(k) for k in range(1, 10)}
    t.close()
    return r


def f64(bits16):
    return TR.bf16_bits_to_f64(bits16)


# ------------------------------------------------------------------------------------------------------------ per op: forward
@pytest.mark.parametrize("tag", BC.TAGS)
def test_convolutions_per_element(tag):
    """A_0 = rb(x) exactly; every Z_k and P in the interval of its own op (no activation) on the engine's A_{k-1}"""
    r = run(tag)
    layers = BC.params(tag)
    x = torch.from_numpy(BC.images(tag)).double()
    A0 = f64(r["A"][0])
    assert torch.equal(A0[:, :3], BL.rb(x)) and not A0[:, 3:].any()
    for k in range(1, 11):
        w, b = layers[k - 1]["w"], layers[k - 1]["b"]
        assert torch.equal(r["Wb"][k - 1], BL.rb(torch.from_numpy(w).double())), (k, "the packed weights are rb(W)")
        o = dict(s2=0, k=3, act=None, cin=CIN[k - 1])
        z, zc, S, e = BL.conv_terms(o, f64(r["A"][k - 1])[:, :CIN[k - 1]], r["Wb"][k - 1], b)
        got = torch.from_numpy(r["P"]).double() if k == 10 else torch.from_numpy(r["Z"][k]).double()
        st = BL.interval_stats(got, z, e, S, 0, fp32_out=(k == 10))
        print(tag, "layer", k, "n %d bad %d exact %.3f rho_max %.3g" % (st["n"], st["bad"], st["exact"], st["rho_max"]))
        assert st["bad"] == 0, (tag, k, st)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_batch_and_running_statistics(tag):
    """mean, var, invstd and the moved running statistics against float64 NumPy on the engine's Z_k: one fp32 rounding of a
    value within the float64 summation bound (N 2^-53 sum |terms|, propagated through each expression) of it"""
    r = run(tag)
    layers = BC.params(tag)
    for k in range(1, 10):
        s = BR.batch_stats_f64(r["Z"][k])
        mean, var, invstd = r["stats"][k]
        _, _, rm, rv, nbt = r["bn"][k]
        N = s["N"]
        assert N == r["plan"][k]["N"] and nbt == 1
        checks = (("mean", mean, s["mean"], s["e_mean"]), ("var", var, s["var"], s["e_var"]), ("invstd", invstd, s["invstd"], s["e_invstd"]),
                  ("running_mean", rm, BR.running_f64(layers[k - 1]["bn"][2], s["mean"]), 0.1 * s["e_mean"] + 2.0 ** -51 * (np.abs(s["mean"]) + 1)),
                  ("running_var", rv, BR.running_f64(layers[k - 1]["bn"][3], s["unbiased"]), 0.1 * s["e_var"] * N / (N - 1) + 2.0 ** -50 * (s["unbiased"] + 2)))
        for what, got, want, e in checks:
            ok = BR.within_one_rounding(got, want, e)
            print(tag, "layer", k, what, "N %d exact %.3f" % (N, float((got == want.astype(np.float32)).mean())))
            assert got.dtype == np.float32 and ok.all(), (tag, k, what, np.nonzero(~ok)[0][:5].tolist())
        assert (var >= 0).all() and np.isfinite(invstd).all()
    if tag == BC.PLANTED:
        for k in range(1, 10):
            zero, _ = BC.planted_channels(k)
            mean, var, invstd = r["stats"][k]
            assert var[zero] == 0.0 and invstd[zero] == np.float32(1.0 / np.sqrt(1e-5)) and bits(mean[zero]) == bits(r["Z"][k][0, zero, 0, 0])


@pytest.mark.parametrize("tag", BC.TAGS)
def test_normalise_leaky_pool_bit_for_bit(tag):
    """A_k and I_k equal the NumPy fp32 restatement from the engine's Z_k, its reported mean and invstd, gamma and beta: the
    first position on ties (the planted all-zero filter: four equal values) and the windows a negative gamma reverses"""
    r = run(tag)
    layers = BC.params(tag)
    for k in range(1, 10):
        mean, _, invstd = r["stats"][k]
        gamma, beta = layers[k - 1]["bn"][:2]
        A, I = BR.normalise_pool(r["Z"][k], mean, invstd, gamma, beta, BC.POOL[k - 1])
        bad = np.argwhere(A != r["A"][k])
        assert not len(bad), (tag, k, "A", len(bad), bad[:5].tolist())
        if BC.POOL[k - 1]:
            bad = np.argwhere(I != r["I"][k])
            assert not len(bad), (tag, k, "I", len(bad), bad[:5].tolist())
            if tag == BC.PLANTED:
                zero, neg = BC.planted_channels(k)
                assert not r["I"][k][:, zero].any() and len(np.unique(r["I"][k][:, neg])) > 1
    assert np.isfinite(BR.bits_to_f32(r["A"][9])).all()


# ------------------------------------------------------------------------------------------------------------ per op: backward
@pytest.mark.parametrize("tag", BC.TAGS)
def test_data_gradients_per_element(tag):
    """G_10 == rb(dP) exactly (padding channels zero); every dY_{k-1} from the engine's G_k, rb(W_k), A_{k-1} and I_{k-1} by
    section 6m's rule: the selected position within [rb(z - e), rb(z + e)], e = 2 K u S 1.001 + u |z|, K = 9 Cout; every
    other position exactly 0"""
    r = run(tag)
    cout10 = r["dP"].shape[1]
    G10 = f64(r["G"][10])
    assert torch.equal(G10[:, :cout10], BL.rb(torch.from_numpy(r["dP"]).double())) and not G10[:, cout10:].any()
    for k in range(10, 1, -1):
        cout = cout10 if k == 10 else r["Wb"][k - 1].shape[0]
        G, Wb, Ap = f64(r["G"][k])[:, :cout], r["Wb"][k - 1], f64(r["A"][k - 1])
        mask = TR.slope_mask(Ap)
        z = TR.dgrad(G, Wb) * mask
        S = TR.dgrad(G.abs(), Wb.abs()) * mask * 1.001
        e = 2 * (9 * cout) * U * S * 1.001 + U * z.abs()
        got = torch.from_numpy(r["DY"][k - 1]).double()
        if BC.POOL[k - 2]:
            gw = TR.windows(got)
            pos = torch.from_numpy(r["I"][k - 1]).long().unsqueeze(-1)
            sel = torch.gather(gw, -1, pos).squeeze(-1)
            others = gw.masked_fill(torch.arange(4).view(1, 1, 1, 1, 4) == pos, 0.0)
            assert not others.any(), (tag, k, "a position the pool did not select is not zero")
            got = sel
        assert got.shape == z.shape
        lo, hi = BL.rb(z - e), BL.rb(z + e)
        bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
        print(tag, "dgrad of layer", k, "n %d bad %d exact %.3f" % (got.numel(), int(bad.sum()), float((got == BL.rb(z)).double().mean())))
        assert not bad.any(), (tag, k, int(bad.sum()), torch.nonzero(bad)[:5].tolist())


@pytest.mark.parametrize("tag", BC.TAGS)
def test_batchnorm_backward_per_element(tag):
    """dgamma and dbeta against float64 sums over the engine's dY_k and the fp32-restated xhat (one fp32 rounding plus the
    summation bound); G_k bit for bit against the NumPy fp32 restatement from the engine's dY_k, Z_k, reported statistics and
    reported dgamma / dbeta, and not zero at the positions the pool did not select"""
    r = run(tag)
    layers = BC.params(tag)
    for k in range(1, 10):
        mean, _, invstd = r["stats"][k]
        dgamma, dbeta = r["bn_grads"][k]
        db64, dg64, e_db, e_dg = BR.bn_sums_f64(r["DY"][k], r["Z"][k], mean, invstd)
        for what, got, want, e in (("dbeta", dbeta, db64, e_db), ("dgamma", dgamma, dg64, e_dg)):
            ok = BR.within_one_rounding(got, want, e)
            assert got.dtype == np.float32 and ok.all(), (tag, k, what, np.nonzero(~ok)[0][:5].tolist())
        N = r["plan"][k]["N"]
        G = BR.bn_apply(r["DY"][k], r["Z"][k], mean, invstd, dgamma, dbeta, layers[k - 1]["bn"][0], N)
        bad = np.argwhere(G != r["G"][k])
        assert not len(bad), (tag, k, "G", len(bad), bad[:5].tolist())
        assert np.isfinite(BR.bits_to_f32(r["G"][k])).all()
        if BC.POOL[k - 1] and N > 64:
            assert np.count_nonzero(BR.bits_to_f32(r["G"][k])) > 0.5 * G.size, (tag, k, "G_k is dense")
    if tag == BC.PLANTED:
        for k in range(1, 10):
            zero, _ = BC.planted_channels(k)
            assert r["bn_grads"][k][0][zero] == 0.0                         # dgamma = sum dY * 0


@pytest.mark.parametrize("tag", BC.TAGS)
def test_weight_and_bias_gradients_per_element(tag):
    """from the engine's G_k and A_{k-1} in float64: |got - z| <= 2 K u S 1.001, K = N = B h w, S = sum |G| |A| (the conv biases
    of layers 1..9, rounding residue on both sides, are held to this bound and to nothing else)"""
    r = run(tag)
    for k in range(1, 11):
        dw, db = r["grads"][k - 1]
        cout, cin = dw.shape[:2]
        G, Ap = f64(r["G"][k])[:, :cout], f64(r["A"][k - 1])[:, :cin]
        K = G.shape[0] * G.shape[2] * G.shape[3]
        zw, zb = TR.wgrad(G, Ap)
        Sw, Sb = TR.wgrad(G.abs(), Ap.abs())
        for what, got, z, S in (("dw", dw, zw, Sw), ("db", db, zb, Sb)):
            err = (torch.from_numpy(got).double() - z).abs()
            bound = 2 * K * U * S * 1.001
            print(tag, "layer", k, what, "K %d max err / bound %.3g" % (K, float((err / bound.clamp(min=1e-300)).max())), "max |z| %.3g" % float(z.abs().max()))
            assert bool((err <= bound).all()), (tag, k, what, float(err.max()), torch.nonzero(err > bound)[:3].tolist())
        assert np.isfinite(dw).all() and np.isfinite(db).all()


def test_deep_case_reductions_span_many_runs():
    """asked of the live handle (y355_bntrain_stats_plan): every layer of the deep case sums over many runs that cover the
    pixels; from layer 2 on the last run is shorter than the others (layer 1: 587 520 = 918 x 640 exactly), and at stride 16
    N = 9 x 15 x 17 = 2295 is odd (the grids before it, 60 x 68 and 30 x 34, have even pixel counts)"""
    (h, w), B, _ = BC.CASES[BC.DEEP]
    for k, p in run(BC.DEEP)["plan"].items():
        last = p["N"] - (p["runs"] - 1) * p["chunk"]
        print("PLAN", BC.DEEP, "layer", k, "N %d runs %d chunk %d last run %d" % (p["N"], p["runs"], p["chunk"], last))
        assert p["N"] == B * (h // DIV[k - 1]) * (w // DIV[k - 1])
        assert p["runs"] >= 16 and p["chunk"] % 128 == 0 and 0 < last <= p["chunk"]
        assert last < p["chunk"] or k == 1
        assert p["N"] % 2 == (1 if k >= 7 else 0)
    for tag in BC.SMALLEST:
        assert [run(tag)["plan"][k]["N"] for k in (7, 8, 9)] == [2, 2, 2]


# ------------------------------------------------------------------------------------------------------------ the update
def test_sgd_is_the_numpy_restatement_bit_for_bit():
    """three steps: W, b, gamma, beta, their momentum buffers and the packed bf16 weights read back equal train_ref.sgd fed
    with the engine's own gradients; the update leaves the running statistics and the gradients as they were"""
    tag = "b48x80_b3_c2"
    lr, mom, wd = 3e-4, 0.9, 5e-4
    t = trainer(tag, lr=lr)
    x, labels = dev(BC.images(tag)), BC.labels(tag)
    p = [list(t.get_layer(k)) + (list(t.get_bn(k)[:2]) if k <= 9 else []) for k in range(1, 11)]
    m = [[None] * len(q) for q in p]
    for it in range(3):
        t.forward_backward(x, labels)
        g = [list(t.get_grad(k)) + (list(t.get_bn_grad(k)) if k <= 9 else []) for k in range(1, 11)]
        flat = all_grads(t)
        running = [t.get_bn(k)[2:] for k in range(1, 10)]
        t.update()
        for k in range(10):
            got_p = list(t.get_layer(k + 1)) + (list(t.get_bn(k + 1)[:2]) if k < 9 else [])
            got_m = list(t.get_momentum(k + 1)) + (list(t.get_bn_momentum(k + 1)) if k < 9 else [])
            for i in range(len(p[k])):
                w, mw = TR.sgd(p[k][i], g[k][i], m[k][i], lr, mom, wd, it == 0)
                assert same(got_p[i], w), (it, k, i, "parameter")
                assert same(got_m[i], mw), (it, k, i, "momentum")
                assert not same(w, p[k][i])
                p[k][i], m[k][i] = w, mw
            assert torch.equal(TR.bf16_bits_to_f64(t.get_packed(k + 1)), BL.rb(torch.from_numpy(p[k][0]).double())), (it, k, "packed weights")
        assert same_lists(all_grads(t), flat)
        after = [t.get_bn(k)[2:] for k in range(1, 10)]
        assert all(same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] == it + 1 for a, b in zip(after, running))
    t.close()


def test_repeated_forwards_move_the_running_statistics():
    """two forwards move the running statistics twice (float64 NumPy on the engine's Z_k, started from the first forward's
    fp32 values) and num_batches_tracked to 2; a backward leaves them alone"""
    from yolo355 import bntrain as T
    tag = "b64_b2_c20"
    t = trainer(tag)
    x = dev(BC.images(tag))
    t.forward(x)
    first = {k: t.get_bn(k) for k in range(1, 10)}
    assert all(same(first[k][2], run(tag)["bn"][k][2]) and same(first[k][3], run(tag)["bn"][k][3]) for k in first)
    t.forward(x)
    for k in range(1, 10):
        s = BR.batch_stats_f64(BR.bits_to_f32(t.get_tensor(T.Z, k)))
        _, _, rm, rv, nbt = t.get_bn(k)
        N = s["N"]
        assert nbt == 2 and not same(rm, first[k][2]) and not same(rv, first[k][3])
        assert BR.within_one_rounding(rm, BR.running_f64(first[k][2], s["mean"]), 0.1 * s["e_mean"] + 2.0 ** -51 * (np.abs(s["mean"]) + 1)).all()
        assert BR.within_one_rounding(rv, BR.running_f64(first[k][3], s["unbiased"]), 0.1 * s["e_var"] * N / (N - 1) + 2.0 ** -50 * (s["unbiased"] + 2)).all()
    before = [t.get_bn(k)[2:] for k in range(1, 10)]
    t.backward(dev(run(tag)["dP"]))
    assert all(same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2] for a, b in zip([t.get_bn(k)[2:] for k in range(1, 10)], before))
    t.close()


# ------------------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("tag", BC.GOLDEN_TAGS)
def test_gradients_against_the_reference(gold, tag):
    """losses within 1 %; dw, dgamma, dbeta of every layer (and db of pred) within a relative L2 distance of
    2 * emu_relerr + 1e-6 of the reference's own backward(); running statistics within the bf16 storage of Z"""
    r = run(tag)
    want = gold["bntrain/%s/losses" % tag].astype(np.float64)
    print(tag, "losses", r["losses"], "reference", want)
    assert (np.abs(r["losses"] - want) <= 0.01 * np.abs(want)).all()
    worst = []
    for k, name in enumerate(BC.LAYERS, 1):
        dw, db = r["grads"][k - 1]
        rel = gold["bntrain/%s/emu_relerr/%s" % (tag, name)]
        pairs = [("dw", dw.reshape(-1)[BC.sample_index(dw.size, tag)], 0)]
        if k == 10:
            pairs.append(("db", db, 1))
        else:
            pairs += [("dgamma", r["bn_grads"][k][0], 2), ("dbeta", r["bn_grads"][k][1], 3)]
        for what, got, i in pairs:
            d = BC.rel_l2(got, gold["bntrain/%s/%s/%s" % (tag, what, name)])
            print("DIST", tag, name, what, "%.4g (emulation %.4g)" % (d, rel[i]))
            if d > 2 * rel[i] + 1e-6:
                worst.append((name, what, d, float(rel[i])))
    assert not worst, worst


def test_two_runs_of_the_deep_case_give_the_same_bits():
    r = run(BC.DEEP)
    t = trainer(BC.DEEP)
    x = dev(BC.images(BC.DEEP))
    for _ in range(2):
        t.forward_backward(x, BC.labels(BC.DEEP))
        assert same_lists(all_grads(t), r["flat"]) and same(t.losses, r["losses"])
        assert all(same(a, b) for k in range(1, 10) for a, b in zip(t.batch_stats(k), r["stats"][k]))
    t.close()


def test_set_size_equals_fresh_handles():
    """one handle built for 96 x 160, switched 64 x 64 -> 96 x 160 -> 64 x 64 (parameters and buffers reloaded before each
    step: the running statistics move with every forward)"""
    from yolo355 import synth
    tag = "b96x160_b1"
    layers = BC.params(tag)
    x = {(64, 64): dev(synth.make_images(77, 1, 64, 64, "noise")), (96, 160): dev(BC.images(tag))}
    labels = BC.labels(tag)
    want = {}
    for size in x:
        f = trainer(tag, size=list(size))
        f.forward_backward(x[size], labels)
        want[size] = everything(f)
        f.close()
    assert same_lists(want[(96, 160)][:38], run(tag)["flat"])
    t = trainer(tag)
    for size in ((64, 64), (96, 160), (64, 64)):
        load(t, layers)
        t.set_grid(list(size))
        assert t.stats_plan(9, 1) == dict(N=size[0] * size[1] // 256, runs=1, chunk=128)
        t.forward_backward(x[size], labels)
        got = everything(t)
        assert same_lists(got, want[size]), (size, [i for i, (a, b) in enumerate(zip(got, want[size])) if not same(a, b)])
    t.close()


@pytest.mark.parametrize("tag,sub", [("b48x80_b3_c2", (1, 2)), ("b16_b2_c2", (0, 2))], ids=["b48x80_b3_c2-1of3", "b16_b2_c2-2of4"])
def test_a_batch_below_max_batch_after_a_full_one(tag, sub):
    """a handle whose Z, dY and every other buffer hold a full batch runs fewer images: everything equals a fresh handle of that
    max_batch, bit for bit and in shape -- no stale row reaches a statistic.  b16_b2_c2: two images on a handle of four."""
    layers = BC.params(tag)
    x, labels = BC.images(tag), BC.labels(tag)
    full_x, full_l = (np.concatenate([x, x]), labels + labels) if tag == "b16_b2_c2" else (x, labels)
    xs, ls = dev(x[sub[0]:sub[1]]), labels[sub[0]:sub[1]]
    f = trainer(tag, max_batch=sub[1] - sub[0])
    f.forward_backward(xs, ls)
    want = everything(f)
    f.close()
    t = trainer(tag, max_batch=len(full_l))
    t.forward_backward(dev(full_x), full_l)
    load(t, layers)
    t.forward_backward(xs, ls)
    got = everything(t)
    assert got[-1].shape[0] == sub[1] - sub[0]
    assert same_lists(got, want), [i for i, (a, b) in enumerate(zip(got, want)) if not same(a, b)]
    t.close()


def test_state_round_trip_gives_the_same_next_step():
    tag = "b64_b2_c20"
    x, labels = dev(BC.images(tag)), BC.labels(tag)
    a = trainer(tag)
    a.step(x, labels)
    sd = a.state_dict()
    names = [n for k in range(1, 11) for n in BC.keys(k)] + [n for k in range(1, 10) for n in BC.bn_keys(k)]
    names += ["%s.convs.1.num_batches_tracked" % n for n in BC.LAYERS[:9]]
    assert sorted(sd) == sorted(names) and all(not v.is_cuda for v in sd.values())
    assert all(int(sd["%s.convs.1.num_batches_tracked" % n]) == 1 for n in BC.LAYERS[:9])
    b = trainer(tag, layers=[dict(L, w=np.zeros_like(L["w"]), b=np.zeros_like(L["b"])) for L in BC.params(tag)])
    b.load_state_dict(sd)
    lb, la = b.forward_backward(x, labels), a.forward_backward(x, labels)
    assert [float(v) for v in la] == [float(v) for v in lb] and same_lists(all_grads(a), all_grads(b))
    assert all(same(u, v) for k in range(1, 10) for u, v in zip(a.get_bn(k)[:4], b.get_bn(k)[:4])) and b.get_bn(9)[4] == 2
    with pytest.raises(KeyError, match="conv3_1.convs.1.running_var"):
        b.load_state_dict({k: v for k, v in sd.items() if k != "conv3_1.convs.1.running_var"})
    a.close()
    b.close()


def test_too_few_values_per_channel_are_refused():
    """16 x 16 with B = 1: one value per channel at layers 7..9; refused before any launch, the handle stays usable"""
    from yolo355 import _ffi
    tag = "b16_b2_c2"
    t = trainer(tag)
    x = dev(BC.images(tag))
    before = [t.get_bn(k) for k in range(1, 10)]
    with pytest.raises(_ffi.Y355Error, match="y355_bntrain_forward: BatchNorm in training mode needs more than one value per channel"):
        t.forward(x[:1])
    with pytest.raises(_ffi.Y355Error, match="y355_bntrain_backward: no forward pass has run at this size"):
        t.backward(torch.zeros(1, 35, 1, 1, device="cuda"))
    with pytest.raises(_ffi.Y355Error, match="y355_bntrain_sgd_step: no backward pass has run"):
        t.update()
    z = np.zeros(256, np.float32)
    assert t._lib.y355_bntrain_load_bn(t._h, 10, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0) == -1
    assert t._lib.y355_bntrain_last_error().decode() == "y355_bntrain_load_bn: layer index must be 1..9"
    after = [t.get_bn(k) for k in range(1, 10)]
    assert all(same(a[i], b[i]) for a, b in zip(after, before) for i in range(4)) and all(a[4] == 0 for a in after)
    t.forward_backward(x, BC.labels(tag))
    assert same_lists(all_grads(t), run(tag)["flat"])
    t.close()


@functools.lru_cache(maxsize=None)
def overfit():
    """ten steps on one fixed batch; lr chosen on the CPU with the emulation so that ITS total loss falls by at least 30 %.
    -> (lr, the emulation's losses, the GPU's losses, the trainer's state_dict and fused state dicts after the steps)"""
    tag = "b64_b2_c20"
    size, B, C = BC.CASES[tag]
    target = TR.targets(size, BC.labels(tag))
    lr = emu = None
    for cand in (1e-3, 3e-4, 3e-3, 1e-4):
        emu = BR.emulate_steps(BC.params(tag), BC.images(tag), target, size, C, cand, 10)
        print("emulation lr", cand, emu)
        if np.isfinite(emu).all() and emu[-1] <= 0.7 * emu[0]:
            lr = cand
            break
    assert lr is not None, "no candidate lr makes the emulation's loss fall by 30 %"
    t = trainer(tag, lr=lr)
    x, labels = dev(BC.images(tag)), BC.labels(tag)
    got = [float(t.step(x, labels)[3]) for _ in range(10)]
    out = dict(lr=lr, emu=emu, got=got, sd=t.state_dict(), fused=t.fused_state_dict(), fused_corrected=t.fused_state_dict(corrected=True))
    t.close()
    return out


def test_overfit_run_reduces_the_loss():
    o = overfit()
    print("gpu lr", o["lr"], o["got"])
    assert np.isfinite(o["got"]).all() and o["got"][-1] < o["got"][0]
    assert o["got"][-1] <= 0.85 * o["got"][0]                                # the emulation fell by 30 %


def test_hand_over_to_the_folded_trainer():
    """fused_state_dict() after the ten steps loads into a SlimTrainer; with corrected=True its P on the same batch lies in
    section 6's interval around the BatchNorm network's eval-mode float64 forward taken layer by layer: every folded layer
    on the folded trainer's own A_{k-1}"""
    from yolo355 import train as T
    tag = "b64_b2_c20"
    size, B, C = BC.CASES[tag]
    o = overfit()
    assert sorted(o["fused"]) == sorted(n for k in range(1, 11) for n in BC.keys(k))
    s = T.SlimTrainer(size, C, BC.ANCHORS, B, 1e-3)
    s.load_state_dict(o["fused"])                                            # the reference's fold loads as it is
    s.load_state_dict(o["fused_corrected"])
    P = s.forward(dev(BC.images(tag))).cpu().numpy().astype(np.float64)
    A = [TR.bf16_bits_to_f64(s.get_tensor(T.ACT, k)) for k in range(10)]
    sd = {k: v.numpy() for k, v in o["sd"].items()}
    for k in range(1, 11):
        kw, kb = BC.keys(k)
        wf, bf = o["fused_corrected"][kw].numpy(), o["fused_corrected"][kb].numpy()
        if k <= 9:                                                           # the fold is the eval-mode BatchNorm in float64, within fp32 rounding
            g, be, mu, var = (sd[n].astype(np.float64) for n in BC.bn_keys(k))
            scale = g / np.sqrt(var + 1e-5)
            assert np.allclose(wf, sd[kw] * scale[:, None, None, None], rtol=1e-6, atol=1e-9)
            assert np.allclose(bf, (sd[kb] - mu) * scale + be, rtol=1e-5, atol=1e-6)
        Wb = TR.bf16_bits_to_f64(s.get_packed(k))
        o_ = dict(s2=0, k=3, act=None if k == 10 else 0.125, cin=CIN[k - 1])
        z, zc, S, e = BL.conv_terms(o_, A[k - 1][:, :CIN[k - 1]], Wb, bf)
        got = torch.from_numpy(P) if k == 10 else A[k]
        st = BL.interval_stats(got, z, e, S, 1 if k < 10 and BC.POOL[k - 1] else 0, fp32_out=(k == 10))
        assert st["bad"] == 0, (k, st)
    want = BR.eval_forward_f64(sd, BC.images(tag)).numpy()
    d = BC.rel_l2(P, want)
    print("hand-over: relative L2 distance of the folded trainer's P from the eval-mode float64 forward %.4g" % d)
    assert d < 0.05                                                          # bf16 storage of nine activations and ten weight tensors
    s.close()


def test_three_kinds_of_handle_in_one_process():
    """a SlimBNTrainer, a SlimTrainer and an engine: each gives what it gives alone"""
    from oracle import yolo_oracle as O
    from yolo355 import synth, train as T
    from yolo355.engine import Engine
    from yolo355.prep import RangeTracker
    import train_cases as TC
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0))
    xc, xe = synth.make_images(1, 1, 96, 96, "blocks"), synth.make_images(3, 2, 96, 96, "blocks")

    def engine():
        eng = Engine([96, 96], 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=2)
        eng.load_quantized(ql)
        eng.calibrate(xc, [RangeTracker() for _ in range(11)])
        return eng

    def folded():
        csize, B, C = TC.CASES["t48x80_b3_c2"]
        s = T.SlimTrainer(csize, C, TC.ANCHORS, B, 1e-3)
        s.load_weights(TC.weights("t48x80_b3_c2"))
        return s

    eng = engine()
    alone = eng.forward(xe)
    eng.close()
    s = folded()
    s.forward_backward(dev(TC.images("t48x80_b3_c2")), TC.labels("t48x80_b3_c2"))
    s_alone = [g for k in range(1, 11) for g in s.get_grad(k)]
    s.close()
    tag = "b48x80_b3_c2"
    t, s, eng = trainer(tag), folded(), engine()
    t.forward_backward(dev(BC.images(tag)), BC.labels(tag))
    s.forward_backward(dev(TC.images("t48x80_b3_c2")), TC.labels("t48x80_b3_c2"))
    dets = eng.forward(xe)
    assert same_lists(all_grads(t), run(tag)["flat"]) and same(np.array(t.losses), run(tag)["losses"])
    assert same_lists([g for k in range(1, 11) for g in s.get_grad(k)], s_alone)
    for (b0, s0, c0), (b1, s1, c1) in zip(alone, dets):
        assert np.array_equal(b0, b1) and np.array_equal(s0, s1) and np.array_equal(c0, c1)
    eng.close()
    s.close()
    t.close()


def test_from_model_and_step_frame_list():
    from yolo355 import bntrain as T, synth
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2
    tag = "b64_b2_c20"
    size, B, C = BC.CASES[tag]
    model = SlimYOLOv2("cuda:0", input_size=size, num_classes=C, trainable=True, anchor_size=BC.ANCHORS)
    model.load_state_dict(BC.state_dict(tag), strict=False)
    frames = [f for f in synth.make_frames_u8(5, B, 50, 70, "blocks")]
    labels = [np.array(l, np.float64).reshape(-1, 5) for l in BC.labels(tag)]
    layers = BC.params(tag)
    out = []
    for _ in range(2):
        t = T.SlimBNTrainer.from_model(model, B, 1e-4)
        assert all(same(t.get_layer(k)[0], layers[k - 1]["w"]) for k in range(1, 11)) and t.input_size == size
        assert all(same(t.get_bn(k)[i], layers[k - 1]["bn"][i]) for k in range(1, 10) for i in range(4))
        losses = t.step_frame_list(frames, labels, seed=3)
        out.append(([float(v) for v in losses], [t.get_layer(k)[0] for k in (1, 10)] + list(t.get_bn(5)[:4])))
        assert all(v.dtype == torch.float32 and v.dim() == 0 for v in losses) and np.isfinite(out[-1][0]).all()
        assert not same(t.get_layer(10)[0], layers[9]["w"]) and not same(t.get_bn(5)[0], layers[4]["bn"][0])
        t.close()
    assert out[0][0] == out[1][0] and same_lists(out[0][1], out[1][1])
