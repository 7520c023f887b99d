"""The float64 restatement of the quantisation-aware training step (tests/qtrain_ref.py) on the CPU: its forward is the
integer oracle's forward_backbone_int(saturate=True) map for map, with the oracle's saturation counts and maxima; its weight
rule is prep.quantize_folded's on the cases' weights and is defined where torch's is not; its straight-through backward written
out equals torch.autograd on the autograd.Function form; and the cases satisfy the conditions tests/test_qtrain.py relies on."""
import numpy as np
import pytest
import torch

import qtrain_cases as QC
import qtrain_ref as QR
import train_ref as TR
from oracle import yolo_oracle as O


@pytest.mark.parametrize("tag,eset", QC.PAIRS, ids=QC.PAIR_IDS)
def test_forward_is_the_integer_oracle(tag, eset):
    """A_k 2^e_a[k] and P 2^e_a[10] equal the oracle's saturated maps; the clipped counts are its sat, the maxima its trackers'
    inputs; accumulator and t stay below 2^24 and the two exponent rules agree (QC.check)"""
    la, lt = QC.check(tag, eset)
    print(tag, eset, "log2 acc_max %.2f log2 t_max %.2f" % (la, lt))
    sa, r = QC.exponents(tag, eset), QC.oracle(tag, eset)
    ql = QR.quantize_masters(QC.weights(tag))
    for L, M in zip(QC.qlayers(tag), ql):
        assert L["e_w"] == M["e_w"] and L["e_b"] == M["e_b"] and np.array_equal(L["q_w"], M["q_w"]) and np.array_equal(L["q_b"], M["q_b"])
    f = QR.forward(ql, QC.images(tag), sa)
    for k in range(1, 10):
        assert np.array_equal(np.ldexp(f["A"][k].numpy(), sa[k]), r["maps"][k - 1].astype(np.float64)), (tag, eset, k)
    assert np.array_equal(np.ldexp(f["P"].numpy(), sa[10]), r["pred_q"].astype(np.float64))
    assert f["clipped"].tolist() == list(r["sat"])
    assert np.array_equal(f["max_abs"], r["max_abs"])
    for k in range(1, 11):                                   # the state byte's clip bit is the output map's saturation
        clip = (f["S"][k].numpy() & QR.S_CLIP) != 0
        assert int(clip.sum()) == r["sat_out"][k - 1] and (np.abs(r["maps"][k - 1])[clip] == 127).all()


def test_every_tracker_clips_in_one_of_the_clip_cases():
    """the condition on the chosen cases: under "cal+1" each of the eleven trackers has a clipped element in t64_b2_c20 or
    t16_b5_c2; under "cal" the calibrated batch itself never clips"""
    sat = np.array([QC.oracle(tag, "cal+1")["sat"] for tag in QC.CLIP_TAGS])
    print("clipped per tracker", sat.tolist())
    assert (sat.max(0) > 0).all()
    for tag in QC.TAGS:
        assert not any(QC.oracle(tag, "cal")["sat"])


def test_zero_activations_take_either_slope():
    """why the state byte and not the sign of A: quantised activations that are exactly 0 come from z <= 0 and from z > 0"""
    tag = QC.ENGINE_TAG
    f = QR.forward(QR.quantize_masters(QC.weights(tag)), QC.images(tag), QC.exponents(tag, "cal"))
    both = 0
    for k in range(1, 10):
        zero = f["A"][k] == 0
        neg = (f["S"][k].long() & QR.S_NEG) != 0
        print("layer", k, "zeros %.4f of them from z > 0 %.4f" % (float(zero.double().mean()), float((zero & ~neg).sum()) / max(int(zero.sum()), 1)))
        both += int(bool((zero & neg).any()) and bool((zero & ~neg).any()))
    assert both >= 5


def test_exponent_rule():
    """the exact rule against torch's on ordinary maxima and where the issue defines it: m = 0, exact powers of two (s is then
    127 2^-j, never a power of two itself), denormals (127 / m overflows: 127)"""
    assert QC.exact_exponent(0.0) == 0
    rng = np.random.RandomState(5)
    for m in np.abs(rng.standard_normal(200)).astype(np.float32) * np.float32(3.0) + np.float32(1e-3):
        assert QC.exact_exponent(m) == O.floor_log2_scale(m)[0], m
    for j in range(-100, 100, 7):
        assert QC.exact_exponent(np.float32(2.0 ** j)) == 6 - j
    assert QC.exact_exponent(np.float32(1e-40)) == 127 and QC.exact_exponent(np.float32(2.0 ** -149)) == 127
    assert QC.exact_exponent(np.finfo(np.float32).max) == -122
    q, e = QR.quantize_tensor(np.zeros((4, 3, 3, 3), np.float32))
    assert e == 0 and not q.any()
    q, e = QR.quantize_tensor(np.array([0.5, -1.0, 0.26], np.float32))
    assert e == 6 and q.tolist() == [32, -64, 17]
    # just below a power of two of the scale: m a little above 127 / 2^(e+1); the exact rule keeps e
    m = np.nextafter(np.float32(127.0 / 8.0), np.float32(100.0))
    assert QC.exact_exponent(m) == 2
    from yolo355 import prep
    for tag in QC.TAGS:
        want = prep.quantize_folded(QC.weights(tag))
        for L, M in zip(want, QR.quantize_masters(QC.weights(tag))):
            assert L["e_w"] == M["e_w"] and L["e_b"] == M["e_b"] and np.array_equal(L["q_w"], M["q_w"]) and np.array_equal(L["q_b"], M["q_b"])


@pytest.mark.parametrize("tag,eset", [("t16x32_b3_c20", "cal+1"), ("t48x80_b3_c2", "cal")], ids=["t16x32_b3_c20-cal+1", "t48x80_b3_c2-cal"])
def test_written_out_backward_is_autograd_of_the_function(tag, eset):
    """the explicit straight-through backward equals torch.autograd through FakeQuant / StePow2, the where of the slope and
    the gather of the first maximum, to float64 rounding"""
    from yolo355 import synth
    sa = QC.exponents(tag, eset)
    ql = QR.quantize_masters(QC.weights(tag))
    f = QR.forward(ql, QC.images(tag), sa)
    dP = synth.uniform_pm1(9, tuple(f["P"].shape)).astype(np.float32)
    grads, G = QR.backward(ql, f["A"], f["S"], dP)
    auto, P = QR.autograd_grads(QC.weights(tag), QC.images(tag), sa, dP)
    assert torch.equal(P, f["P"])
    for k, ((dw, db), (aw, ab)) in enumerate(zip(grads, auto), 1):
        assert float(dw.abs().max()) > 0
        assert QC.TC.rel_l2(dw.numpy(), aw.numpy()) < 1e-12 and QC.TC.rel_l2(db.numpy(), ab.numpy()) < 1e-12, (tag, k)
    for k in range(1, 10):                                   # clipped elements carry no gradient, unselected positions none
        fac = QR.state_factor(f["S"][k])
        g = TR.pool_first(G[k].abs())[0] if QC.TC.POOL[k - 1] else G[k]
        assert not g[fac == 0].any()


# ------------------------------------------------------------------------------------------------ the library without a GPU
import ctypes      # noqa: E402
import os          # noqa: E402
import re          # noqa: E402
import shutil      # noqa: E402
import subprocess  # noqa: E402

from yolo355 import _ffi, qtrain as Q     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")
NAMES = sorted("y355_qtrain_" + n for n in (
    "backward", "create", "destroy", "forward", "get_act_exponents", "get_act_stats", "get_grad", "get_layer", "get_momentum", "get_packed",
    "get_qbias", "get_tensor", "get_weight_exponents", "last_error", "layer_shape", "load_layer", "pred", "set_act_exponents", "set_size", "sgd_step",
    "tensor_shape", "wgrad_plan"))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree():
    names = Q.declared_symbols()
    assert set(names) == set(Q._SIGS) and names == NAMES
    assert _exports(Q.LIB_PATH) == names
    lib = Q.lib()
    text = re.sub(r"/\*.*?\*/", "", open(Q.HEADER_PATH).read(), flags=re.S)
    for n in names:
        assert hasattr(lib, n)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert (0 if args.strip() == "void" else len(args.split(","))) == len(Q._SIGS[n][1]), n
    assert (Q.STATE, Q.S_POS, Q.S_NEG, Q.S_CLIP, Q.MAX_ACT_EXPONENT) == tuple(
        int(re.search(r"#define Y355_QTRAIN_%s (\d+)" % n, text).group(1)) for n in ("STATE", "S_POS", "S_NEG", "S_CLIP", "MAX_ACT_EXPONENT"))


def test_header_is_c99_and_cxx11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_qtrain.h"\nint main(void) {\n  y355_qtrain *h = 0;\n'
                   "  return h == 0 && Y355_QTRAIN_LAYERS == 10 && Y355_QTRAIN_TRACKERS == 11 && Y355_QTRAIN_ENOTREADY == -3 ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_library_stands_alone():
    from yolo355 import anchors, augment, bntrain, grad, loss, train
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, augment.LIB_PATH, grad.LIB_PATH, train.LIB_PATH, bntrain.LIB_PATH):
        assert not [n for n in _exports(path) if n.startswith("y355_qtrain_")]
    assert not [n for n in _exports(Q.LIB_PATH) if not n.startswith("y355_qtrain_")]
    needed = subprocess.run(["readelf", "-d", Q.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libyolo355" not in needed.replace("libyolo355_qtrain.so", "")


def test_arguments_are_refused_before_any_hip_call():
    """without a handle: create's rules and the null refusals, each with the family's prefix"""
    lib = Q.lib()
    err = lambda: lib.y355_qtrain_last_error().decode()
    h = ctypes.c_void_p()
    for args, text in (((60, 64, 2, 5, 1), "multiples of 16"), ((64, 64, 0, 5, 1), "num_classes must be 1..200"), ((64, 64, 2, 17, 1), "num_anchors must be 1..16"),
                       ((64, 64, 2, 5, 0), "max_batch must be 1..1024")):
        assert lib.y355_qtrain_create(*args, ctypes.byref(h)) == -1 and err().startswith("y355_qtrain_create: ") and text in err() and not h.value
    assert lib.y355_qtrain_forward(None, None, 1, None) == -1 and err() == "y355_qtrain_forward: null argument"
    assert lib.y355_qtrain_backward(None, None, None) == -1 and err() == "y355_qtrain_backward: null argument"
    assert lib.y355_qtrain_set_act_exponents(None, None) == -1 and err() == "y355_qtrain_set_act_exponents: null argument"
    assert lib.y355_qtrain_get_act_stats(None, None, None) == -1 and err() == "y355_qtrain_get_act_stats: null handle"
    assert lib.y355_qtrain_get_weight_exponents(None, None) == -1 and err() == "y355_qtrain_get_weight_exponents: null argument"
    assert lib.y355_qtrain_get_qbias(None, 1, None) == -1 and err() == "y355_qtrain_get_qbias: null handle"
    assert lib.y355_qtrain_sgd_step(None, 0.1, 0.9, 0.0, None) == -1 and err() == "y355_qtrain_sgd_step: null handle"
    lib.y355_qtrain_destroy(None)


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-qtrain: tests/qtrain_host_check.cpp, a stand-alone program, with the library's host code under
    -fsanitize=address,undefined: the create rules, the all-or-none buffers, every refusal on a live handle leaving its state
    alone, and the exponent rule at m = 0, powers of two and denormals"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-qtrain", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "qtrain_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "qtrain_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line


def test_python_side_without_a_gpu():
    from yolo355 import prep
    from yolo355.models.slim_yolo_v2 import _TRACKERS
    assert Q.TRACKER_NAMES == list(_TRACKERS) and issubclass(Q.SlimQatTrainer, Q.Trainer)
    tr = [prep.RangeTracker(scale=torch.tensor([2.0 ** e * 1.5]), first_a=1) for e in range(11)]
    assert Q._exponent_list(tr) == list(range(11)) and Q._exponent_list(range(11)) == list(range(11))
    sd = {n + ".scale": t.scale for n, t in zip(Q.TRACKER_NAMES, tr)}
    assert Q._exponent_list(sd) == list(range(11))
    with pytest.raises(ValueError):
        Q._exponent_list([1, 2, 3])
    with pytest.raises(KeyError):
        Q._exponent_list({"a_tracker_in.scale": torch.ones(1)})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            Q.SlimQatTrainer([64, 64], 2, QC.ANCHORS, 1, 1e-3)
