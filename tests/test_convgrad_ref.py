"""The float64 restatement of the convolution-gradient contract (tests/convgrad_ref.py) on the CPU: its hand-written backward
with G unrounded equals torch.autograd on every case of the table, its output size is torch's; and libyolo355_convgrad.so
without a GPU: header, exports and signatures, the library standing alone, the refusals made before any HIP call, the host
check under the sanitizers, and the Python side."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import convgrad_ref as R
from yolo355 import _ffi, convgrad as CG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")
NAMES = sorted("y355_convgrad_" + n for n in ("backward", "create", "destroy", "forward", "last_error", "out_size", "wgrad_plan"))


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_written_out_backward_is_autograd(name, slope):
    """float64, G unrounded: forward and (dx, dw, db) equal torch.autograd.grad of leaky_relu / relu / identity of F.conv2d
    within 1e-12 relative"""
    c = R.CASES[name]
    x, w, b, dy = (t.double() for t in R.inputs(name))
    z, y = R.forward(x, w, b, c.geo, slope)
    G = R.grad_out(dy, y, slope, round_g=False)
    dx, dw, db = R.backward(x, w, G, c.geo)
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    ya = R.torch_forward(xa, wa, ba, c.geo, slope)
    gx, gw, gb = torch.autograd.grad(ya, (xa, wa, ba), dy)
    assert rel(y, ya.detach()) < 1e-12
    for mine, want in ((dx, gx), (dw, gw), (db, gb)):
        assert float(want.abs().max()) > 0 and rel(mine, want) < 1e-12, (name, slope)


@pytest.mark.parametrize("name", list(R.CASES))
def test_out_size_is_torch(name):
    c = R.CASES[name]
    g = CG.Geom(*c.geo)
    y = R.torch_forward(torch.zeros(1, 1, c.H, c.W), torch.zeros(1, 1, c.geo.kh, c.geo.kw), None, c.geo, 1.0)
    assert CG.out_size(g, c.H, c.W) == tuple(y.shape[2:]) == R.out_size(c.geo, c.H, c.W)


def test_every_case_is_listed_once_and_within_the_limits():
    assert set(R.TABLE + R.RUNS + R.EDGES + ("s2k1", "s2p0")) == set(R.CASES)
    for c in R.CASES.values():
        CG.geometry((c.geo.kh, c.geo.kw), (c.geo.stride_h, c.geo.stride_w), 0, (c.geo.dil_h, c.geo.dil_w))      # raises past a limit
        assert max(c.geo[6:]) <= 64 and 1 <= c.cin <= CG.MAX_CHANNELS and 1 <= c.cout <= CG.MAX_CHANNELS
    at = lambda i: max(c.geo[i] for c in R.CASES.values())
    assert (at(0), at(1), at(2), at(4), at(5), at(6)) == (32, 32, 16, 32, 32, 64)       # every limit of the geometry is reached
    cp = lambda n: (n + 7) // 8 * 8
    assert (cp(R.CASES["mix"].cin), cp(R.CASES["mix"].cout)) == (24, 40)


@pytest.mark.parametrize("name", list(R.CASES) + ["dead"])
def test_helpers_of_the_exact_checks_agree_with_the_restatement(name):
    """pixel / patch: a one-hot G at the case's last flat pixel makes dw[co] the patch; dead_taps: exactly the taps whose rows
    of S (dw of absolute values under G = 1) are zero -- 'dead' is a 3x3 whose outer columns lie 8 pixels beside a 5-wide map"""
    c = R.Case(R.geo(3, 1, (1, 1, 8, 8), (1, 8)), 2, 3, 1, 6, 5) if name == "dead" else R.CASES[name]
    x, w, _, dy = (t.double() for t in R.make_inputs(c, 7))
    ho, wo = R.out_size(c.geo, c.H, c.W)
    q = c.B * ho * wo - 1
    bi, oy, ox = R.pixel(c, q)
    assert (bi, oy, ox) == (c.B - 1, ho - 1, wo - 1) and R.pixel(c, (c.B - 1) * ho * wo + wo - 1) == (c.B - 1, 0, wo - 1)
    one = torch.zeros_like(dy)
    one[bi, c.cout - 1, oy, ox] = 1.0
    dw = R.backward(x, w, one, c.geo)[1]
    assert torch.equal(dw[c.cout - 1].float(), R.patch(c, x, bi, oy, ox)) and not dw[:c.cout - 1].any()
    S = R.backward(x.abs(), w.abs(), torch.ones_like(dy), c.geo)[1]
    dead = torch.from_numpy(R.dead_taps(c.geo, c.H, c.W))
    assert torch.equal(S.sum((0, 1)) == 0, dead) and (S[:, :, ~dead] > 0).all()
    if name == "dead":
        assert dead.tolist() == [[True, False, True]] * 3


@pytest.mark.parametrize("k,d", [(2, 1), (4, 1), (4, 3), ((2, 6), (3, 2)), (3, 2), ((5, 4), 1)])
def test_same_padding_is_torch(k, d):
    """'same' through the conv_geometry rules, even kernels included: torch's output shape and torch's values (the odd pixel
    goes bottom / right)"""
    g = CG.geometry(k, 1, "same", d)
    kh, kw = (k, k) if isinstance(k, int) else k
    x, w = torch.randn(1, 2, 9, 7, dtype=torch.float64), torch.randn(3, 2, kh, kw, dtype=torch.float64)
    want = F.conv2d(x, w, None, 1, "same", d)
    assert CG.out_size(g, 9, 7) == tuple(want.shape[2:]) == (9, 7)
    assert g.astuple() == tuple(R.geo(k, 1, "same", d))
    assert rel(R.forward(x, w, None, R.Geo(*g.astuple()), 1.0)[0], want) < 1e-12


def test_geometry_rules():
    assert CG.geometry(3, 2, 1).astuple() == (3, 3, 2, 2, 1, 1, 1, 1, 1, 1)
    assert CG.geometry((5, 3), (1, 2), (2, 1), (2, 1)).astuple() == (5, 3, 1, 2, 2, 1, 2, 2, 1, 1)
    assert CG.geometry(1, padding="valid").astuple() == (1, 1, 1, 1, 1, 1, 0, 0, 0, 0)
    for bad in (dict(kernel_size=33), dict(kernel_size=3, stride=17), dict(kernel_size=3, dilation=33), dict(kernel_size=3, padding=65)):
        with pytest.raises(NotImplementedError):
            CG.geometry(**bad)
    lib = CG.lib()
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    g = CG.Geom(7, 7, 1, 1, 1, 1, 0, 0, 0, 0)
    assert lib.y355_convgrad_out_size(ctypes.byref(g), 6, 9, ctypes.byref(ho), ctypes.byref(wo)) == -1
    assert "larger than the padded input" in lib.y355_convgrad_last_error().decode()
    # the same verdicts and sizes as the operator API's y355_conv_geom_out_size
    main = _ffi.lib()
    for geom in [CG.Geom(*c.geo) for c in R.CASES.values()] + [g, CG.Geom(0, 3, 1, 1, 1, 1, 0, 0, 0, 0)]:
        for H, W in ((6, 9), (13, 10), (1, 1), (40, 3)):
            a, b = ctypes.c_int(), ctypes.c_int()
            rc_main = main.y355_conv_geom_out_size(ctypes.byref(geom), H, W, ctypes.byref(a), ctypes.byref(b))
            rc = lib.y355_convgrad_out_size(ctypes.byref(geom), H, W, ctypes.byref(ho), ctypes.byref(wo))
            assert rc == rc_main and (rc != 0 or (ho.value, wo.value) == (a.value, b.value))


# ------------------------------------------------------------------------------------------------ the library without a GPU
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree():
    names = CG.declared_symbols()
    assert set(names) == set(CG._SIGS) and names == NAMES
    assert _exports(CG.LIB_PATH) == names
    lib = CG.lib()
    text = re.sub(r"/\*.*?\*/", "", open(CG.HEADER_PATH).read(), flags=re.S)
    for n in names:
        assert hasattr(lib, n)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert (0 if args.strip() == "void" else len(args.split(","))) == len(CG._SIGS[n][1]), n
    assert CG.MAX_CHANNELS == int(re.search(r"#define Y355_CONVGRAD_MAX_CHANNELS (\d+)", text).group(1))
    # the geometry struct is the operator API's, field for field
    main = re.sub(r"/\*.*?\*/", "", open(_ffi.HEADER_PATH).read(), flags=re.S)
    fields = lambda t, n: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\}" % n, t, flags=re.S).group(1)).strip()
    assert fields(text, "y355_convgrad_geom") == fields(main, "y355_conv_geom")


def test_header_is_c99_and_cxx11(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_convgrad.h"\nint main(void) {\n  y355_convgrad *h = 0;\n  y355_convgrad_geom g = {3, 3, 1, 1, 1, 1, 1, 1, 1, 1};\n'
                   "  return h == 0 && g.kh == 3 && Y355_CONVGRAD_EHIP == -2 && Y355_CONVGRAD_MAX_CHANNELS == 4096 ? 0 : 1;\n}\n")
    for cc, std, extra, out in (("gcc", "-std=c99", [], "use.o"), ("g++", "-std=c++11", ["-x", "c++"], "use_cc.o")):
        r = subprocess.run([cc, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                           ["-c", str(src), "-o", str(tmp_path / out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_the_library_stands_alone():
    from yolo355 import anchors, augment, bntrain, grad, loss, qtrain, train
    for path in (_ffi.LIB_PATH, loss.LIB_PATH, anchors.LIB_PATH, augment.LIB_PATH, grad.LIB_PATH, train.LIB_PATH, bntrain.LIB_PATH, qtrain.LIB_PATH):
        assert not [n for n in _exports(path) if n.startswith("y355_convgrad_")]
    assert not [n for n in _exports(CG.LIB_PATH) if not n.startswith("y355_convgrad_")]
    needed = subprocess.run(["readelf", "-d", CG.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libyolo355" not in needed.replace("libyolo355_convgrad.so", "")


def test_arguments_are_refused_before_any_hip_call():
    lib = CG.lib()
    err = lambda: lib.y355_convgrad_last_error().decode()
    h = ctypes.c_void_p()
    g3 = CG.Geom(3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
    for (dev, cin, cout, geom, slope), text in (((-1, 3, 16, g3, 1.0), "device_id must be >= 0"), ((0, 0, 16, g3, 1.0), "cin and cout must be 1..4096"),
                                                ((0, 3, 4097, g3, 1.0), "cin and cout must be 1..4096"), ((0, 3, 16, g3, -1.0), "neg_slope must be finite"),
                                                ((0, 3, 16, CG.Geom(3, 33, 1, 1, 1, 1, 1, 1, 1, 1), 1.0), "kernel size must be 1..32"),
                                                ((0, 3, 16, CG.Geom(3, 3, 1, 17, 1, 1, 1, 1, 1, 1), 1.0), "stride must be 1..16"),
                                                ((0, 3, 16, CG.Geom(3, 3, 1, 1, 0, 1, 1, 1, 1, 1), 1.0), "dilation must be 1..32"),
                                                ((0, 3, 16, CG.Geom(3, 3, 1, 1, 1, 1, 1, 65, 1, 1), 1.0), "padding must be 0..64")):
        assert lib.y355_convgrad_create(dev, cin, cout, ctypes.byref(geom), slope, ctypes.byref(h)) == -1
        assert err().startswith("y355_convgrad_create: ") and text in err() and not h.value
    assert lib.y355_convgrad_forward(None, None, None, None, 1, 4, 4, None, None) == -1 and err() == "y355_convgrad_forward: null argument"
    assert lib.y355_convgrad_backward(None, None, None, None, None, 1, 4, 4, None, None, None, None) == -1
    assert err() == "y355_convgrad_backward: null argument"
    assert lib.y355_convgrad_wgrad_plan(None, 1, 4, 4, None) == -1 and err() == "y355_convgrad_wgrad_plan: null argument"
    lib.y355_convgrad_destroy(None)


def test_host_check_under_the_sanitizers(tmp_path):
    """make -C csrc hostcheck-convgrad: tests/convgrad_host_check.cpp, a stand-alone program, with the library's host code under
    -fsanitize=address,undefined: the create rules, every refusal, the plan, every allocation failed in turn"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.fail("hipcc is needed to build the host check")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "hostcheck-convgrad", "BUILD=" + str(tmp_path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "convgrad_host_check ok" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if "convgrad_host_check.cpp" in l and "-o" in l][0]
    assert "-fsanitize=address,undefined" in line and "-Xarch_host" in line


def test_python_side_without_a_gpu():
    import torch.nn as nn
    from yolo355.utils import modules as M
    net = nn.Sequential()
    net.add_module("c1", M.Conv2d(3, 16, 3, padding=1, stride=2, leakyReLU=True))
    net.add_module("c2", M.Conv2d_fuse(16, 32, 1, leakyReLU=True))
    net.add_module("c3", M.Conv2d_fuse_nobias(32, 32, 3, padding="same", dilation=2))
    net.add_module("pred", nn.Conv2d(32, 35, 1))
    t = CG.trainable(net)
    assert list(t) == ["c1", "c2", "c3", "pred"]
    for name, wrapper in t.items():                               # the wrapper's parameters ARE the block's
        block = net.get_submodule(name)
        assert wrapper.convs is (block.convs if hasattr(block, "convs") else block)
        assert [id(p) for p in wrapper.parameters()] == [id(p) for p in block.parameters()]
        if hasattr(block, "convs"):
            assert list(wrapper.state_dict()) == list(block.state_dict())
    assert [CG._split(w.convs)[3] for w in t.values()] == [0.125, 0.125, 0.0, 1.0]
    assert CG._split(t["c1"].convs)[1] is net.c1.convs[1] and CG._split(t["c2"].convs)[1] is None
    with pytest.raises(TypeError):
        CG.TrainableConv(nn.Sequential(nn.ReLU()))
    with pytest.raises(ValueError, match="CUDA float32"):
        CG.conv2d(torch.zeros(1, 3, 4, 4), torch.zeros(8, 3, 3, 3))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU is visible"):
            CG.ConvGrad(3, 16, CG.geometry(3, 1, 1))
