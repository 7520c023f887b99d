"""The BatchNorm training step without a GPU: tests/bntrain_ref.py's float64 restatement against the reference's own backward()
(tests/golden/bntrain.npz, tests/golden/gen_golden_bntrain.py) and against torch's float64 autograd of nn.BatchNorm2d in
training mode; the fp32 emulation of the contract at the recorded distance from the reference; the
NumPy restatements the GPU is compared with bit for bit against torch; the surface of the companion library
libyolo355_bntrain.so (header, exports and ctypes signatures agree, the header is C99 and C++11, the other libraries know
nothing of it, arguments are refused before any HIP call, the host check builds and passes under the sanitizers as a
stand-alone program); fuse_state_dict against prep.fuse_conv_and_bn; LrSchedule at closed-form points.  No GPU."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import bntrain_cases as BC
import bntrain_ref as BR
import train_ref as TR
from yolo355 import _ffi
from yolo355 import bntrain as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")
WHAT = ("dw", "db", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "bntrain.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def restated(tag, contract):
    """bntrain_ref.step on a case: computed once, left unchanged.  The float64 form takes the fixture's undecided LeakyReLU
    sides and pooling windows, where the reference's fp32 forward cannot tell two values apart."""
    size, B, C = BC.CASES[tag]
    sides = picks = None
    if not contract:
        with np.load(os.path.join(ROOT, "tests", "golden", "bntrain.npz")) as z:
            sides = z["bntrain/%s/sides" % tag] if "bntrain/%s/sides" % tag in z.files else None
            picks = z["bntrain/%s/picks" % tag] if "bntrain/%s/picks" % tag in z.files else None
    return BR.step(BC.params(tag), BC.images(tag), TR.targets(size, BC.labels(tag)), size, C, contract, sides, picks)


def kept(tag, k, grads):
    """[dw (the fixture's elements), db, dgamma, dbeta] of layer k (pred: the first two)"""
    g = grads[k - 1]
    return [g[0].reshape(-1)[BC.sample_index(g[0].size, tag)], g[1]] + ([g[2], g[3]] if k <= 9 else [])


# ------------------------------------------------------------------------------------------------ against the reference
def test_fixture_is_complete_and_small(gold):
    for tag in BC.TAGS:
        assert gold["bntrain/%s/losses" % tag].shape == (4,) and gold["bntrain/%s/losses" % tag].dtype == np.float32
        for k, name in enumerate(BC.LAYERS, 1):
            L = BC.params(tag)[k - 1]
            assert gold["bntrain/%s/dw/%s" % (tag, name)].shape == (BC.sample_index(L["w"].size, tag).size,)
            assert gold["bntrain/%s/db/%s" % (tag, name)].shape == L["b"].shape
            assert gold["bntrain/%s/emu_relerr/%s" % (tag, name)].shape == (4,) and gold["bntrain/%s/gap/%s" % (tag, name)].shape == (4,)
            if k <= 9:
                for what in ("dgamma", "dbeta", "running_mean", "running_var"):
                    assert gold["bntrain/%s/%s/%s" % (tag, what, name)].shape == L["b"].shape
    sizes = {f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.endswith(".npz")}
    assert sizes["bntrain.npz"] < sizes["fp32.npz"] == max(sizes.values())


def test_cases_are_what_they_claim():
    for tag in BC.SMALLEST:
        (h, w), B, _ = BC.CASES[tag]
        assert B * (h // 16) * (w // 16) == 2
    (h, w), B, _ = BC.CASES[BC.DEEP]
    assert [(B * (h // d) * (w // d)) % 2 for d in BC.DIV[:9]] == [0, 0, 0, 0, 0, 0, 1, 1, 1]
    for tag in BC.TAGS:
        for k in range(1, 10):
            g, be, mu, var = BC.params(tag)[k - 1]["bn"]
            assert (g != 1).all() and (be != 0).all() and (mu != 0).all() and (var != 1).all()      # none at BatchNorm2d's defaults
    for k in range(1, 10):
        zero, neg = BC.planted_channels(k)
        L = BC.params(BC.PLANTED)[k - 1]
        assert not L["w"][zero].any() and L["bn"][0][neg] < 0 and (np.delete(L["bn"][0], neg) > 0).all()


@pytest.mark.parametrize("tag", BC.TAGS)
def test_float64_restatement_equals_the_reference(gold, tag):
    """grad_ref.assert_maps' bound for fp32 against float64: twice the recorded gap, never more than 1e-5 of the largest
    |gradient| of the tensor.  Two exceptions, both the reference's own fp32 error.  (1) The conv biases of layers 1..9: the
    batch mean removes a bias, their gradient is zero and the reference holds rounding residue; only the gap is asked.
    (2) The two cases with N = 2 at layers 7..9: two values per channel normalise to +-sqrt(var / (var + eps)) whatever they
    are, so everything below layer 9 is (dY_1 - dY_2) / 2 * eps / (var + eps), a difference of fp32 terms that cancel to
    1e-5 / var of their size; the reference's rounding, 2^-24 of the terms, is 2^-24 var / 1e-5 of the result -- up to 1e-2
    for var up to 1.7, which takes the place of 1e-5 there."""
    r = restated(tag, False)
    want = gold["bntrain/%s/losses" % tag].astype(np.float64)
    print(tag, "losses", r["losses"], want)
    assert (np.abs(r["losses"] - want) <= 1e-5 * np.abs(want)).all()
    cap = 1e-2 if tag in BC.SMALLEST else 1e-5
    for k, name in enumerate(BC.LAYERS, 1):
        gap = gold["bntrain/%s/gap/%s" % (tag, name)]
        for i, got in enumerate(kept(tag, k, r["grads"])):
            ref = gold["bntrain/%s/%s/%s" % (tag, WHAT[i], name)].astype(np.float64)
            err = np.abs(got - ref).max()
            bound = 2.0 * float(gap[i]) if (i == 1 and k <= 9) else min(2.0 * float(gap[i]), cap * float(np.abs(ref).max()))
            print(tag, name, WHAT[i], "err %.3g bound %.3g" % (err, bound))
            assert err <= bound, (tag, name, WHAT[i], err, bound)
    run = BR.running_after(BC.params(tag), r["stats"])
    for k, name in enumerate(BC.LAYERS[:9], 1):
        sg = gold["bntrain/%s/stat_gap/%s" % (tag, name)]
        for i, what in enumerate(("running_mean", "running_var")):
            ref = gold["bntrain/%s/%s/%s" % (tag, what, name)].astype(np.float64)
            # the reference's fp32 forward: a convolution sums up to K = 2304 terms, K 2^-24 = 1.4e-4 at worst
            assert np.abs(run[k][i] - ref).max() <= min(2.0 * float(sg[i]), 1e-4 * float(np.abs(ref).max())), (tag, name, what)


@pytest.mark.parametrize("tag", BC.TAGS)
def test_emulation_reproduces_the_recorded_distance(gold, tag):
    """the fp32 emulation of the contract lies where the GPU has to lie: within 2 * emu_relerr + 1e-6 of the reference per
    tensor (on the machine that wrote the fixture its distance IS emu_relerr)"""
    r = restated(tag, True)
    want = gold["bntrain/%s/losses" % tag].astype(np.float64)
    assert (np.abs(r["losses"] - want) <= 0.01 * np.abs(want)).all(), (r["losses"], want)
    for k, name in enumerate(BC.LAYERS, 1):
        rel = gold["bntrain/%s/emu_relerr/%s" % (tag, name)]
        for i, got in enumerate(kept(tag, k, r["grads"])):
            if i == 1 and k <= 9:
                continue                                                       # rounding residue on both sides
            d = BC.rel_l2(got, gold["bntrain/%s/%s/%s" % (tag, WHAT[i], name)])
            print(tag, name, WHAT[i], "emulation %.4g recorded %.4g" % (d, rel[i]))
            assert rel[i] > 0 and d <= 2 * rel[i] + 1e-6


def test_explicit_backward_equals_float64_autograd():
    """every op of the restated backward pass against torch's own differentiation of conv2d + nn.functional.batch_norm in
    training mode + leaky_relu + max_pool2d, in float64; and the running statistics torch leaves behind"""
    import torch.nn.functional as F
    tag = BC.PLANTED
    layers = BC.params(tag)
    ps = [tuple(None if v is None else v.clone().requires_grad_(True) for v in p) for p in BR.tensors(layers, torch.float64)]
    x = torch.from_numpy(BC.images(tag)).double()
    a, bufs = x, {}
    for k in range(1, 10):
        w, b, g, be = ps[k - 1]
        rm, rv = (torch.from_numpy(np.array(v)).double() for v in layers[k - 1]["bn"][2:])
        a = F.leaky_relu(F.batch_norm(F.conv2d(a, w, b, 1, 1), rm, rv, g, be, True, 0.1, 1e-5), 0.125)
        bufs[k] = (rm, rv)
        if BC.POOL[k - 1]:
            a = F.max_pool2d(a, 2, 2)
    P = F.conv2d(a, ps[9][0], ps[9][1], 1, 1)
    dP = torch.from_numpy(BC.synth.uniform_pm1(9, tuple(P.shape)).astype(np.float64))
    P.backward(dP)
    with torch.no_grad():
        det = [tuple(None if v is None else v.detach() for v in p) for p in ps]
        A, I, cache, P2 = BR.forward(det, x, False)
        grads, _, _ = BR.backward(det, A, I, cache, dP, False)
    assert float((P2 - P.detach()).abs().max().detach()) <= 1e-11 * float(P.detach().abs().max())
    run = BR.running_after(layers, {k: (c["mean64"].numpy(), c["var64"].numpy(), c["N"]) for k, c in cache.items()})
    for k in range(1, 11):
        for i, got in enumerate(grads[k - 1]):
            if got is None:
                continue
            want = ps[k - 1][i].grad
            err = float((got - want).abs().max())
            assert err <= 1e-10 * max(float(want.abs().max()), 1e-30) + 1e-13 * float(grads[k - 1][0].abs().max()), (k, WHAT[i], err)
        if k <= 9:
            assert np.abs(run[k][0] - bufs[k][0].numpy()).max() <= 1e-13 and np.abs(run[k][1] - bufs[k][1].numpy()).max() <= 1e-12


def test_numpy_restatements_are_the_torch_ops():
    """normalise_pool and bn_apply (what the GPU's A_k, I_k and G_k are compared with bit for bit) against the same fp32
    operations in torch; rb_bits against torch's bfloat16; the first maximum on ties and under a negative gamma"""
    rng = np.random.RandomState(5)
    Z = BR.bits_to_f32(BR.rb_bits(rng.randn(2, 8, 6, 10).astype(np.float32)))
    Z[:, 3] = Z[0, 3, 0, 0]                                                    # a constant channel: var = 0, four-way ties
    assert np.array_equal(BR.rb_bits(Z), torch.from_numpy(Z).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    v = rng.randn(1000).astype(np.float32)
    assert np.array_equal(BR.rb_bits(v), torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    s = BR.batch_stats_f64(Z)
    mean, invstd = s["mean"].astype(np.float32), s["invstd"].astype(np.float32)
    assert s["var"][3] == 0.0 and mean[3] == Z[0, 3, 0, 0]
    gamma, beta = (1 + 0.3 * rng.randn(8)).astype(np.float32), (0.2 * rng.randn(8)).astype(np.float32)
    gamma[5] = -abs(gamma[5])
    A, I = BR.normalise_pool(Z, mean, invstd, gamma, beta, True)
    c = lambda a: torch.from_numpy(np.asarray(a, np.float32)).view(1, -1, 1, 1)
    zt = torch.from_numpy(Z)
    xhat = (zt - c(mean)) * c(invstd)
    y = xhat * c(gamma) + c(beta)
    m, pos = TR.pool_first(TR.leaky(y))
    assert np.array_equal(A, m.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)) and np.array_equal(I, pos.numpy())
    assert not I[:, 3].any()                                                   # the first of four equal values
    zw = TR.windows(zt)[:, 5]
    assert torch.equal(torch.from_numpy(I[:, 5]).long(), torch.where(zw == zw.amin(-1, keepdim=True), torch.arange(4), torch.tensor(4)).amin(-1))
    A1, I1 = BR.normalise_pool(Z, mean, invstd, gamma, beta, False)
    assert I1 is None and np.array_equal(A1, TR.leaky(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    dY = BR.bits_to_f32(BR.rb_bits(rng.randn(*Z.shape).astype(np.float32)))
    db64, dg64, e_db, e_dg = BR.bn_sums_f64(dY, Z, mean, invstd)
    dgamma, dbeta = dg64.astype(np.float32), db64.astype(np.float32)
    assert dgamma[3] == 0.0 and np.allclose(dg64, (torch.from_numpy(dY).double() * xhat.double()).sum((0, 2, 3)).numpy(), rtol=0, atol=1e-12)
    N = 2 * 6 * 10
    G = BR.bn_apply(dY, Z, mean, invstd, dgamma, dbeta, gamma, N)
    t = torch.from_numpy(dY) - c(dbeta / np.float32(N))
    t = t - xhat * c(dgamma / np.float32(N))
    want = (t * c(gamma * invstd)).to(torch.bfloat16)
    assert np.array_equal(G, want.view(torch.int16).numpy().view(np.uint16))
    # ... and the per-element form is batch_norm's gradient: float64 autograd on the same dY
    zr = zt.double().requires_grad_(True)
    torch.nn.functional.batch_norm(zr, None, None, c(gamma).double().view(-1), c(beta).double().view(-1), True, 0.1, 1e-5).backward(torch.from_numpy(dY).double())
    assert float((want.double() - zr.grad).abs().max()) <= 2.0 ** -8 * float(zr.grad.abs().max())
    assert BR.within_one_rounding(np.float32(0.1), 0.1, 0).all() and not BR.within_one_rounding(np.float32(0.1) + np.float32(1e-8), 0.1, 0).any()


def test_emulated_steps_reduce_the_loss():
    tag = "b64_b2_c20"
    size, B, C = BC.CASES[tag]
    losses = BR.emulate_steps(BC.params(tag), BC.images(tag), TR.targets(size, BC.labels(tag)), size, C, 1e-3, 4)
    assert np.isfinite(losses).all() and losses[3] < losses[0], losses


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


NAMES = sorted("y355_bntrain_" + n for n in (
    "create", "destroy", "set_size", "layer_shape", "load_layer", "get_layer", "forward", "pred", "backward", "get_grad", "get_momentum", "get_packed",
    "wgrad_plan", "sgd_step", "tensor_shape", "get_tensor", "last_error", "load_bn", "get_bn", "get_bn_grad", "get_bn_momentum", "get_batch_stats",
    "stats_plan"))


def test_header_library_and_signatures_agree():
    names = T.declared_symbols()
    assert set(names) == set(T._SIGS) and names == NAMES
    assert _exports(T.LIB_PATH) == names
    lib = T.lib()
    text = re.sub(r"/\*.*?\*/", "", open(T.HEADER_PATH).read(), flags=re.S)
    for n in names:
        assert hasattr(lib, n)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(T._SIGS[n][1]), n
    for name, value in (("ACT", T.ACT), ("IDX", T.IDX), ("GRAD", T.GRAD), ("Z", T.Z), ("DY", T.DY), ("LAYERS", T.NUM_LAYERS), ("BN_LAYERS", T.NUM_BN)):
        assert int(re.search(r"#define Y355_BNTRAIN_%s (\d+)" % name, text).group(1)) == value
    assert float(re.search(r"#define Y355_BNTRAIN_EPS (\S+)", text).group(1)) == T.EPS == BR.EPS
    assert float(re.search(r"#define Y355_BNTRAIN_MOMENTUM (\S+)", text).group(1)) == T.BN_MOMENTUM == BR.MOMENTUM


def test_header_is_c99_and_cxx11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_bntrain.h"\nint main(void) {\n  y355_bntrain *h = 0;\n'
                   "  return h == 0 && Y355_BNTRAIN_LAYERS == 10 && Y355_BNTRAIN_BN_LAYERS == 9 && Y355_BNTRAIN_ENOTREADY == -3 && Y355_BNTRAIN_DY == 4 ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_other_libraries_know_nothing_of_it():
    from yolo355 import anchors, augment, grad, loss, train
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, augment.LIB_PATH, grad.LIB_PATH, train.LIB_PATH):
        assert not [n for n in _exports(path) if n.startswith("y355_bntrain_")]
    assert not [n for n in _exports(T.LIB_PATH) if not n.startswith("y355_bntrain_")]
    assert len(_exports(train.LIB_PATH)) == 17                                # the move to train_core.h added no export
    needed = subprocess.run(["readelf", "-d", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libyolo355" not in needed.replace("libyolo355_bntrain.so", "")


def test_arguments_are_refused_before_any_hip_call():
    """without a handle (no GPU here): create's rules and the null-handle refusals, each with its own text"""
    lib = T.lib()
    err = lambda: lib.y355_bntrain_last_error().decode()
    h = ctypes.c_void_p()
    for args, text in (((60, 64, 2, 5, 1), "multiples of 16"), ((64, 100, 2, 5, 1), "multiples of 16"), ((64, 64, 0, 5, 1), "num_classes must be 1..200"),
                       ((64, 64, 2, 17, 1), "num_anchors must be 1..16"), ((64, 64, 2, 5, 0), "max_batch must be 1..1024")):
        assert lib.y355_bntrain_create(*args, ctypes.byref(h)) == -1 and text in err() and not h.value
    assert lib.y355_bntrain_create(64, 64, 2, 5, 1, None) == -1 and err() == "y355_bntrain_create: null argument"
    assert lib.y355_bntrain_set_size(None, 64, 64) == -1 and err() == "y355_bntrain_set_size: null handle"
    assert lib.y355_bntrain_forward(None, None, 1, None) == -1 and err() == "y355_bntrain_forward: null argument"
    assert lib.y355_bntrain_backward(None, None, None) == -1 and err() == "y355_bntrain_backward: null argument"
    assert lib.y355_bntrain_sgd_step(None, 0.1, 0.9, 0.0, None) == -1 and err() == "y355_bntrain_sgd_step: null handle"
    assert lib.y355_bntrain_load_layer(None, 1, None, None) == -1 and err() == "y355_bntrain_load_layer: null handle"
    assert lib.y355_bntrain_load_bn(None, 1, None, None, None, None, 0) == -1 and err() == "y355_bntrain_load_bn: null handle"
    assert lib.y355_bntrain_get_bn(None, 1, None, None, None, None, None) == -1 and err() == "y355_bntrain_get_bn: null handle"
    assert lib.y355_bntrain_get_bn_grad(None, 1, None, None) == -1 and err() == "y355_bntrain_get_bn_grad: null handle"
    assert lib.y355_bntrain_get_batch_stats(None, 1, None, None, None) == -1 and err() == "y355_bntrain_get_batch_stats: null handle"
    plan = (ctypes.c_int32 * 3)(7, 7, 7)
    assert lib.y355_bntrain_stats_plan(None, 1, 1, plan) == -1 and err() == "y355_bntrain_stats_plan: null handle" and list(plan) == [7, 7, 7]
    lib.y355_bntrain_destroy(None)


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-bntrain: tests/bntrain_host_check.cpp, a stand-alone program, with the library's host code under
    -fsanitize=address,undefined: the create rules, the all-or-none buffers, BatchNorm2d's initial values, every refusal on a
    live handle (the N < 2 rule among them), set_size, and y355_bntrain_stats_plan on the two shapes tools/bntrain_bench.py
    times, which the program prints: the first layer's reduction runs over 2432 and 10 880 pixels a workgroup there"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-bntrain", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "bntrain_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "bntrain_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line and "-ffp-contract=off" in line
    plans = {}
    for l in r.stdout.splitlines():
        m = re.match(r"stats plan (\d+) x (\d+) x (\d+):", l)
        if m:
            plans[tuple(int(v) for v in m.groups())] = [tuple(int(v) for v in p) for p in re.findall(r"\{N (\d+), runs (\d+), chunk (\d+), last (\d+)\}", l)]
    assert all(len(p) == 9 for p in plans.values())
    assert [p[2] for p in plans[(64, 416, 416)]] == [10880, 2816, 768, 768, 256, 256, 128, 128, 128]
    assert [p[2] for p in plans[(32, 240, 320)]] == [2432, 640, 256, 256, 128, 128, 128, 128, 128]
    assert plans[(2, 16, 16)][6:] == [(2, 1, 128, 2)] * 3


# ------------------------------------------------------------------------------------------------ the Python side
def test_fused_state_dict_is_prep_s_fold_under_the_folded_trainer_s_keys():
    from yolo355 import prep, train
    tag = "b64_b2_c20"
    sd = BC.state_dict(tag)
    for corrected in (False, True):
        f = T.fuse_state_dict(sd, corrected=corrected)
        assert list(f) == [n for k in range(1, 11) for n in train.layer_keys(k)] and all(v.dtype == torch.float32 for v in f.values())
        for k in range(1, 10):
            L = BC.params(tag)[k - 1]
            conv, bn = torch.nn.Conv2d(L["w"].shape[1], L["w"].shape[0], 3, 1, 1), torch.nn.BatchNorm2d(L["w"].shape[0])
            with torch.no_grad():
                for dst, src in ((conv.weight, L["w"]), (conv.bias, L["b"]), (bn.weight, L["bn"][0]), (bn.bias, L["bn"][1]), (bn.running_mean, L["bn"][2]),
                                 (bn.running_var, L["bn"][3])):
                    dst.copy_(torch.from_numpy(np.array(src)))
            want = prep.fuse_conv_and_bn(conv, bn, corrected=corrected)
            kw, kb = train.layer_keys(k)
            assert torch.equal(f[kw], want.weight.detach()) and torch.equal(f[kb], want.bias.detach()), (k, corrected)
        assert torch.equal(f["pred.weight"], sd["pred.weight"]) and torch.equal(f["pred.bias"], sd["pred.bias"])
    a, b = T.fuse_state_dict(sd), T.fuse_state_dict(sd, corrected=True)
    assert torch.equal(a["conv5.convs.0.weight"], b["conv5.convs.0.weight"]) and not torch.equal(a["conv5.convs.0.bias"], b["conv5.convs.0.bias"])
    assert T.bn_keys(4) == ("conv3_2.convs.1.weight", "conv3_2.convs.1.bias", "conv3_2.convs.1.running_mean", "conv3_2.convs.1.running_var",
                            "conv3_2.convs.1.num_batches_tracked")
    assert [T.bn_keys(k)[:4] for k in range(1, 10)] == [BC.bn_keys(k) for k in range(1, 10)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            T.SlimBNTrainer([64, 64], 2, BC.ANCHORS, 2, 1e-3)


def test_lr_schedule_at_closed_form_points():
    base, E = 1e-3, 100
    s = T.LrSchedule(base, E, 160, (60, 90))
    assert s.epoch_start(0) == base
    assert s.iteration(0, 0) == 0.0                                            # the warm-up's first iteration
    assert s.iteration(0, 50) == base * (50 / 200.0) ** 4
    assert s.iteration(1, 0) == base * 0.5 ** 4 == base / 16                   # its middle
    assert s.iteration(1, 99) == base * (199 / 200.0) ** 4                     # its last
    assert s.epoch_start(2) == base * (199 / 200.0) ** 4 and s.iteration(2, 0) == base     # the hand-over
    assert s.iteration(2, 1) == base and s.iteration(3, 0) == base
    for e in range(3, 60):
        assert s.epoch_start(e) == base
    assert s.epoch_start(60) == base * 0.1 and s.iteration(60, 5) == base * 0.1
    assert s.epoch_start(61) == base * 0.1
    assert s.epoch_start(90) == base * 0.1 * 0.1 and s.epoch_start(159) == base * 0.1 * 0.1
    c = T.LrSchedule(base, E, 160, (60, 90), cos=True)
    assert c.epoch_start(20) == base                                           # up to epoch 20 the step rule
    first = c.epoch_start(21)
    assert first == 1e-5 + 0.5 * (base - 1e-5) * (1 + math.cos(math.pi / 140)) and 0.999 * base < first < base
    assert c.epoch_start(90) == 1e-5 + 0.5 * (base - 1e-5) * (1 + math.cos(math.pi * 70 / 140))      # the middle: half way down
    assert abs(c.epoch_start(90) - (1e-5 + 0.5 * (base - 1e-5))) < 1e-18
    assert c.epoch_start(140) == 1e-5 + 0.5 * (base - 1e-5) * (1 + math.cos(math.pi * 120 / 140))    # the branch's last epoch
    assert c.epoch_start(141) == 1e-5 and c.epoch_start(159) == 1e-5 and c.iteration(159, 3) == 1e-5  # the tail
    n = T.LrSchedule(base, E, 160, (1,), warm_up=False)
    assert n.iteration(0, 0) == base and n.epoch_start(1) == base * 0.1 and n.iteration(1, 0) == base * 0.1
    w = T.LrSchedule(base, 10, 160, (60, 90), wp_epoch=1)
    assert w.iteration(0, 5) == base * 0.5 ** 4 and w.iteration(1, 0) == base
