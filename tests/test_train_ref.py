"""The training step without a GPU: tests/train_ref.py's float64 restatement against the reference's own backward()
(tests/golden/train.npz, tests/golden/gen_golden_train.py) and against torch's float64 autograd; the fp32 emulation of the
contract within the distance from the reference the GPU is held to; the NumPy SGD against
torch.optim.SGD; and the surface of the companion library libyolo355_train.so: header, exports and ctypes signatures agree,
the header is C99 and C++11, the other libraries know nothing of it, arguments are refused before any HIP call, the host
check builds and passes under the sanitizers as a stand-alone program.  No GPU."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import train_cases as TC
import train_ref as TR
from yolo355 import _ffi
from yolo355 import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "train.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def restated(tag, contract):
    """(losses, grads, P) of train_ref.step on a case: computed once, left unchanged.  The float64 form takes the fixture's
    undecided LeakyReLU sides (gen_golden_train.py: none but in t416x448_b3_c2, two elements), where the reference's fp32
    forward cannot tell a pre-activation from zero and the gradient below jumps by a factor of 8."""
    size, B, C = TC.CASES[tag]
    sides = None
    if not contract:
        with np.load(os.path.join(ROOT, "tests", "golden", "train.npz")) as z:
            sides = z["train/%s/sides" % tag] if "train/%s/sides" % tag in z.files else None
    return TR.step(TC.weights(tag), TC.images(tag), TR.targets(size, TC.labels(tag)), size, C, contract, sides)


# ------------------------------------------------------------------------------------------------ against the reference
def test_fixture_is_complete_and_small(gold):
    for tag in TC.TAGS:
        C = TC.CASES[tag][2]
        assert gold["train/%s/losses" % tag].shape == (4,) and gold["train/%s/losses" % tag].dtype == np.float32
        for k, name in enumerate(TC.LAYERS, 1):
            w, b = TC.weights(tag)[k - 1]
            assert w.shape[0] == (5 * (5 + C) if name == "pred" else w.shape[0])
            n = TC.sample_index(w.size, tag).size
            if TC.TAGS.index(tag) < 3:
                assert n == w.size if w.size <= 20000 else n <= 16384
            else:                                                              # the added cases keep at most 512, never fewer than half of that
                assert n == w.size if w.size <= 512 else 256 <= n <= 512
            assert gold["train/%s/dw/%s" % (tag, name)].shape == (n,) and gold["train/%s/db/%s" % (tag, name)].shape == b.shape
            assert gold["train/%s/emu_relerr/%s" % (tag, name)].shape == (2,) and gold["train/%s/gap/%s" % (tag, name)].shape == (2,)
            assert float(gold["train/%s/dw_norm/%s" % (tag, name)]) > 0
    sizes = {f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.endswith(".npz")}
    assert sizes["train.npz"] < max(v for f, v in sizes.items() if f != "train.npz")


@pytest.mark.parametrize("tag", TC.TAGS)
def test_float64_restatement_equals_the_reference(gold, tag):
    """grad_ref.assert_maps' bound for fp32 against float64: twice the recorded gap, never more than 1e-5 of the largest
    |gradient| of the tensor"""
    out, grads, _ = restated(tag, False)
    want = gold["train/%s/losses" % tag].astype(np.float64)
    print(tag, "losses", out, want)
    assert (np.abs(out - want) <= 1e-5 * np.abs(want)).all()
    for k, name in enumerate(TC.LAYERS, 1):
        dw, db = grads[k - 1]
        gw, gb, gap = gold["train/%s/dw/%s" % (tag, name)], gold["train/%s/db/%s" % (tag, name)], gold["train/%s/gap/%s" % (tag, name)]
        for what, got, ref, g in (("dw", dw.reshape(-1)[TC.sample_index(dw.size, tag)], gw, gap[0]), ("db", db, gb, gap[1])):
            err, bound = np.abs(got - ref.astype(np.float64)).max(), min(2.0 * float(g), 1e-5 * float(np.abs(ref).max()))
            print(tag, name, what, "err %.3g bound %.3g" % (err, bound))
            assert err <= bound, (tag, name, what, err, bound)


@pytest.mark.parametrize("tag", TC.TAGS)
def test_emulation_of_the_contract_within_the_gpu_s_bound(gold, tag):
    """the fp32 emulation (bf16 activations, weights and gradients) lies where the GPU has to lie: within 2 * emu_relerr + 1e-6
    of the reference per layer (on the machine that wrote the fixture its distance IS emu_relerr); the recorded distances are
    those of bf16 storage, not of a wrong gradient"""
    out, grads, _ = restated(tag, True)
    want = gold["train/%s/losses" % tag].astype(np.float64)
    assert (np.abs(out - want) <= 0.01 * np.abs(want)).all(), (out, want)
    for k, name in enumerate(TC.LAYERS, 1):
        dw, db = grads[k - 1]
        rel = gold["train/%s/emu_relerr/%s" % (tag, name)]
        assert (rel > 0).all() and (rel < 0.5).all(), (tag, name, rel)
        dw_s = dw.reshape(-1)[TC.sample_index(dw.size, tag)]
        got = (TC.rel_l2(dw_s, gold["train/%s/dw/%s" % (tag, name)]), TC.rel_l2(db, gold["train/%s/db/%s" % (tag, name)]))
        print(tag, name, "emulation %.4g %.4g recorded %.4g %.4g" % (got + tuple(rel)))
        assert got[0] <= 2 * rel[0] + 1e-6 and got[1] <= 2 * rel[1] + 1e-6


def test_explicit_backward_equals_float64_autograd():
    """every op of the backward pass against torch's own differentiation of the forward, in float64"""
    tag = "t48x80_b3_c2"
    size, B, C = TC.CASES[tag]
    ws = [(torch.from_numpy(w).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)) for w, b in TC.weights(tag)]
    x = torch.from_numpy(TC.images(tag)).double()
    A, I, P = TR.forward(ws, x, False)
    dP = torch.from_numpy(TC.synth.uniform_pm1(9, tuple(P.shape)).astype(np.float64))
    P.backward(dP)
    with torch.no_grad():
        grads, G = TR.backward([(w.detach(), b.detach()) for w, b in ws], [a.detach() for a in A], I, dP, False)
    for k, ((w, b), (dw, db)) in enumerate(zip(ws, grads), 1):
        for what, got, want in (("dw", dw, w.grad), ("db", db, b.grad)):
            err = float((got - want).abs().max())
            assert err <= 1e-12 * max(float(want.abs().max()), 1e-30), (k, what, err)


def test_pool_takes_the_first_maximum_and_unpool_inverts_it():
    v = torch.tensor([[[[1.0, 1.0, 0.0, 3.0], [1.0, 1.0, 3.0, 3.0], [-2.0, -1.0, 5.0, 4.0], [-1.0, -3.0, 4.0, 5.0]]]], dtype=torch.float64)
    m, pos = TR.pool_first(v)
    assert m.tolist() == [[[[1.0, 3.0], [-1.0, 5.0]]]] and pos.tolist() == [[[[0, 1], [1, 0]]]]
    mt, it = torch.nn.functional.max_pool2d(v, 2, 2, return_indices=True)            # torch takes the first one too
    y, xx = it // 4, it % 4
    assert torch.equal(mt, m) and torch.equal(((y % 2) * 2 + xx % 2).to(torch.uint8), pos)
    u = TR.unpool(m, pos)
    assert u.tolist() == [[[[1.0, 0.0, 0.0, 3.0], [0.0, 0.0, 0.0, 0.0], [0.0, -1.0, 5.0, 0.0], [0.0, 0.0, 0.0, 0.0]]]]
    big = torch.from_numpy(TC.synth.uniform_pm1(3, (2, 3, 6, 10)).astype(np.float64))
    m, pos = TR.pool_first(big)
    assert torch.equal(TR.pool_first(TR.unpool(m, pos).where(TR.unpool(torch.ones_like(m), pos) > 0, torch.tensor(-9.0, dtype=torch.float64)))[0], m)
    assert torch.equal(TR.leaky(torch.tensor([-8.0, 0.0, 2.0])), torch.tensor([-1.0, 0.0, 2.0]))
    assert torch.equal(TR.slope_mask(torch.tensor([-8.0, 0.0, 2.0])), torch.tensor([0.125, 0.125, 1.0]))          # > 0, not >= 0


def test_numpy_sgd_equals_torch_sgd():
    """three steps (the first without a momentum buffer) against torch.optim.SGD in float64 started from the fp32 state of
    every step: four roundings per element, 4 u (|p| + lr (|buf| + |g| + weight_decay |p|))"""
    lr, mom, wd = 0.01, 0.9, 5e-4
    p = TC.synth.uniform_pm1(11, (257,))
    buf = None
    for it in range(3):
        g = TC.synth.uniform_pm1(12 + it, (257,)) * np.float32(3.0)
        q = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
        opt = torch.optim.SGD([q], lr=lr, momentum=mom, weight_decay=wd)
        if buf is not None:
            opt.state[q]["momentum_buffer"] = torch.from_numpy(buf.astype(np.float64))
        q.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        bound = TR.sgd_bound(p, g, np.zeros_like(p) if buf is None else buf, lr, wd)
        p2, buf2 = TR.sgd(p, g, buf, lr, mom, wd, it == 0)
        assert p2.dtype == np.float32 and buf2.dtype == np.float32
        assert (np.abs(p2.astype(np.float64) - q.detach().numpy()) <= bound).all()
        assert (np.abs(buf2.astype(np.float64) - opt.state[q]["momentum_buffer"].numpy()) <= bound / lr).all()
        assert not np.array_equal(p2, p)
        p, buf = p2, buf2


def test_emulated_steps_reduce_the_loss():
    tag = "t64_b2_c20"
    size, B, C = TC.CASES[tag]
    losses = TR.emulate_steps(TC.weights(tag), TC.images(tag), TR.targets(size, TC.labels(tag)), size, C, 1e-4, 3)
    assert losses[2] < losses[1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


NAMES = ["y355_train_backward", "y355_train_create", "y355_train_destroy", "y355_train_forward", "y355_train_get_grad", "y355_train_get_layer",
         "y355_train_get_momentum", "y355_train_get_packed", "y355_train_get_tensor", "y355_train_last_error", "y355_train_layer_shape",
         "y355_train_load_layer", "y355_train_pred", "y355_train_set_size", "y355_train_sgd_step", "y355_train_tensor_shape", "y355_train_wgrad_plan"]


def test_header_library_and_signatures_agree():
    names = T.declared_symbols()
    assert set(names) == set(T._SIGS) and names == NAMES
    assert _exports(T.LIB_PATH) == names
    lib = T.lib()
    text = open(T.HEADER_PATH).read()
    import re
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in names:
        assert hasattr(lib, n)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(T._SIGS[n][1]), n


def test_header_is_c99_and_cxx11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_train.h"\nint main(void) {\n  y355_train *h = 0;\n'
                   "  return h == 0 && Y355_TRAIN_LAYERS == 10 && Y355_TRAIN_ENOTREADY == -3 ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_other_libraries_know_nothing_of_it():
    from yolo355 import anchors, augment, grad, loss
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, augment.LIB_PATH, grad.LIB_PATH):
        assert not [n for n in _exports(path) if n.startswith("y355_train_")]
    assert not [n for n in _exports(T.LIB_PATH) if not n.startswith("y355_train_")]
    needed = subprocess.run(["readelf", "-d", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libyolo355" not in needed.replace("libyolo355_train.so", "")


def test_arguments_are_refused_before_any_hip_call():
    """without a handle (no GPU here): create's rules and the null-handle refusals, each with its own text"""
    lib = T.lib()
    err = lambda: lib.y355_train_last_error().decode()
    h = ctypes.c_void_p()
    for args, text in (((60, 64, 2, 5, 1), "multiples of 16"), ((64, 100, 2, 5, 1), "multiples of 16"), ((64, 64, 0, 5, 1), "num_classes must be 1..200"),
                       ((64, 64, 2, 17, 1), "num_anchors must be 1..16"), ((64, 64, 2, 5, 0), "max_batch must be 1..1024")):
        assert lib.y355_train_create(*args, ctypes.byref(h)) == -1 and text in err() and not h.value
    assert lib.y355_train_create(64, 64, 2, 5, 1, None) == -1 and err() == "y355_train_create: null argument"
    assert lib.y355_train_set_size(None, 64, 64) == -1 and err() == "y355_train_set_size: null handle"
    assert lib.y355_train_forward(None, None, 1, None) == -1 and err() == "y355_train_forward: null argument"
    assert lib.y355_train_backward(None, None, None) == -1 and err() == "y355_train_backward: null argument"
    assert lib.y355_train_sgd_step(None, 0.1, 0.9, 0.0, None) == -1 and err() == "y355_train_sgd_step: null handle"
    assert lib.y355_train_load_layer(None, 1, None, None) == -1 and err() == "y355_train_load_layer: null handle"
    plan = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert lib.y355_train_wgrad_plan(None, 1, 1, plan) == -1 and err() == "y355_train_wgrad_plan: null handle" and list(plan) == [7, 7, 7, 7]
    lib.y355_train_destroy(None)


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-train: tests/train_host_check.cpp, a stand-alone program, with the library's host code under
    -fsanitize=address,undefined: the create rules, the all-or-none buffers, every refusal on a live handle, set_size, and
    y355_train_wgrad_plan -- its refusals, its rule on every layer, and the plans of the two shapes tools/train_bench.py times
    (20 classes), which the program asserts and prints: every layer's run is 160 to 5408 pixels long there, 5 to 169 steps of 32"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-train", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "train_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "train_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line
    import re
    plans = {}
    for l in r.stdout.splitlines():
        m = re.match(r"wgrad plan (\d+) x (\d+) x (\d+):", l)
        if m:
            plans[tuple(int(v) for v in m.groups())] = [tuple(int(v) for v in p) for p in
                                                        re.findall(r"\{npix (\d+), max_runs (\d+), runs (\d+), chunk (\d+), last (\d+)\}", l)]
    assert all(len(p) == 10 for p in plans.values())
    assert [p[3] for p in plans[(64, 416, 416)]] == [5408, 1376, 704, 1376, 704, 1376, 704, 1376, 1376, 704]
    assert [p[3] for p in plans[(32, 240, 320)]] == [1216, 320, 160, 320, 160, 320, 160, 320, 320, 160]
    for shape in ((64, 416, 416), (32, 240, 320)):                             # the deployed regime: several steps a wave, runs near the cap
        assert all(chunk >= 160 and 0.9 * cap <= runs <= cap and 0 < last <= chunk for _, cap, runs, chunk, last in plans[shape])
    assert all(p == (q[0], q[1], 1, 32, q[0]) for p, q in zip(plans[(1, 16, 16)][6:], [(1, 64), (1, 32), (1, 32), (1, 64)]))


def test_python_side_without_a_gpu():
    assert [T.layer_keys(k) for k in (1, 4, 10)] == [("conv1.convs.0.weight", "conv1.convs.0.bias"), ("conv3_2.convs.0.weight", "conv3_2.convs.0.bias"),
                                                    ("pred.weight", "pred.bias")]
    assert T.LAYER_NAMES == TC.LAYERS and [T.layer_keys(k) for k in range(1, 11)] == [TC.keys(k) for k in range(1, 11)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            T.SlimTrainer([64, 64], 2, TC.ANCHORS, 1, 1e-3)
