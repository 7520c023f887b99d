"""libyolo355_convgrad.so on the GPU against the float64 restatement of its contract (tests/convgrad_ref.py): every element of
y, dx, dw and db of the table's cases inside the interval 2 K u S 1.001 + u |value|; the exact properties (zeros of dx where
no window reaches, an all-zero dy, a one-hot dy, the same bits from run to run and on two streams); the refusals; conv2d under
torch.autograd; and a four-block net of the drop-ins trained through TrainableConv with yolo355.grad.YoloCriterion and
torch.optim.SGD."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convgrad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def CG():
    from yolo355 import convgrad
    return convgrad


@functools.lru_cache(maxsize=None)
def handle(name, slope):
    c = R.CASES[name]
    return CG().ConvGrad(c.cin, c.cout, CG().Geom(*c.geo), slope, DEV)


@functools.lru_cache(maxsize=None)
def operands(name):
    """the case's inputs once: float32 on the CPU and on the GPU, and the rounded operands in float64"""
    x, w, b, dy = R.inputs(name)
    return dict(cpu=(x, w, b, dy), gpu=tuple(t.to(DEV) for t in (x, w, b, dy)), xr=R.rb(x).double(), wr=R.rb(w).double())


def run(name, slope, bias=True, h=None):
    """(y, dx, dw, db) of the C ABI on the case, as CPU tensors"""
    h = h or handle(name, slope)
    x, w, b, dy = operands(name)["gpu"]
    y = h.forward(x, w, b if bias else None)
    dx, dw, db = h.backward(x, w, None if slope == 1.0 else y, dy, True, True, bias)
    return tuple(None if t is None else t.cpu() for t in (y, dx, dw, db))


def inside(got, want, K, S, what):
    err = (got.double() - want).abs()
    lim = R.bound(K, S, want)
    worst = float((err / lim.clamp_min(1e-300)).max())
    print("%s: max err %.3g, worst err / bound %.3g" % (what, float(err.max()), worst))
    assert torch.isfinite(got).all() and (err <= lim).all(), what


@pytest.mark.parametrize("slope", R.SLOPES)
@pytest.mark.parametrize("name", R.TABLE + ("s2k1", "s2p0"))
def test_every_element_against_float64(name, slope):
    c, o = R.CASES[name], operands(name)
    x, w, b, dy = o["cpu"]
    g, taps = c.geo, c.geo.kh * c.geo.kw
    ho, wo = R.out_size(g, c.H, c.W)
    for bias in (True, False):
        y, dx, dw, db = run(name, slope, bias)
        b64 = b.double() if bias else None
        z64, y64 = R.forward(o["xr"], o["wr"], b64, g, slope)
        S = R.forward(o["xr"].abs(), o["wr"].abs(), None if b64 is None else b64.abs(), g, 1.0)[0]
        inside(y, y64, c.cin * taps + (1 if bias else 0) + 1, S, "%s slope %g bias %d y" % (name, slope, bias))
        # the mask from the GPU's own y: a sign that flipped at |z| <= e is not counted twice
        G = R.grad_out(dy, y, slope).double()
        dx64, dw64, db64 = R.backward(o["xr"], o["wr"], G, g)
        Sx, Sw, Sb = R.backward(o["xr"].abs(), o["wr"].abs(), G.abs(), g)
        inside(dx, dx64, c.cout * taps + 1, Sx, "%s slope %g bias %d dx" % (name, slope, bias))
        inside(dw, dw64, c.B * ho * wo + 1, Sw, "%s slope %g bias %d dw" % (name, slope, bias))
        if bias:
            inside(db, db64, c.B * ho * wo + 1, Sb, "%s slope %g db" % (name, slope))
        else:
            assert db is None
        assert float(dw64.abs().max()) > 0 and float(dx64.abs().max()) > 0


def test_case_h_has_three_runs_and_a_shorter_last_one():
    c = R.CASES["h"]
    plan = handle("h", 0.125).wgrad_plan(c.B, c.H, c.W)
    print(plan)
    assert plan["npix"] == c.B * c.H * c.W and plan["runs"] >= 3 and 0 < plan["last"] < plan["chunk"] and plan["chunk"] % 32 == 0
    assert (plan["runs"] - 1) * plan["chunk"] + plan["last"] == plan["npix"]
    cf = R.CASES["f"]                                               # many k-steps, one run
    assert handle("f", 0.125).wgrad_plan(cf.B, cf.H, cf.W)["runs"] == 1


def raw_backward(h, x, w, y, dy, fill=float("nan")):
    """the C call into tensors that held `fill`: what comes back was written by the call"""
    CGm = CG()
    B, _, H, W = x.shape
    dx, dw = torch.full_like(x, fill), torch.full_like(w, fill)
    db = torch.full((w.shape[0],), fill, device=x.device)
    CGm.check(h._lib.y355_convgrad_backward(h._h, x.data_ptr(), w.data_ptr(), None if y is None else y.data_ptr(), dy.data_ptr(), B, H, W,
                                            dx.data_ptr(), dw.data_ptr(), db.data_ptr(), CGm._stream(x.device)))
    return dx.cpu(), dw.cpu(), db.cpu()


@pytest.mark.parametrize("name", ["s2k1", "s2p0", "c", "d"])
def test_dx_is_zero_where_no_window_reaches(name):
    c = R.CASES[name]
    x, w, b, dy = operands(name)["gpu"]
    h = handle(name, 1.0)
    dx, _, _ = raw_backward(h, x, w, None, dy)
    m = torch.from_numpy(R.untouched(c.geo, c.H, c.W))
    print(name, "untouched pixels", int(m.sum()))
    if name.startswith("s2"):
        assert int(m.sum()) > 0
    assert torch.isfinite(dx).all()                                 # every element was written
    assert (dx[:, :, m] == 0).all() and (dx[:, :, ~m] != 0).any()


@pytest.mark.parametrize("name", ["a", "c", "d", "h"])
def test_zero_dy_gives_zero_gradients(name):
    x, w, b, dy = operands(name)["gpu"]
    h = handle(name, 0.125)
    y = h.forward(x, w, b)
    for t in raw_backward(h, x, w, y, torch.zeros_like(dy)):
        assert (t == 0).all()


@pytest.mark.parametrize("name,at", [("d", (1, 5, 3, 2)), ("a", (0, 15, 0, 10)), ("c", (1, 31, 6, 4)), ("h", (0, 7, 8, 8))])
def test_one_hot_dy_makes_dw_the_rounded_patch(name, at):
    """dy = 1 at one output element: dw[co] is the rb(x) patch under that window bit for bit (zeros where the window leaves
    the map), every other row of dw is zero, db is the one-hot"""
    c, o = R.CASES[name], operands(name)
    x, w, b, dy = o["gpu"]
    one = torch.zeros_like(dy)
    one[at] = 1.0
    dx, dw, db = raw_backward(handle(name, 1.0), x, w, None, one)
    _, dw64, db64 = R.backward(o["xr"], o["wr"], one.cpu().double(), c.geo)
    bi, co, oy, ox = at
    g = c.geo
    patch = torch.zeros(c.cin, g.kh, g.kw)
    for ky in range(g.kh):
        for kx in range(g.kw):
            iy, ix = oy * g.stride_h + ky * g.dil_h - g.pad_top, ox * g.stride_w + kx * g.dil_w - g.pad_left
            if 0 <= iy < c.H and 0 <= ix < c.W:
                patch[:, ky, kx] = o["xr"][bi, :, iy, ix].float()
    assert torch.equal(dw64.float()[co], patch)                      # the restatement agrees with the patch written out
    assert torch.equal(dw, dw64.float()) and torch.equal(db, db64.float())
    assert float(dw[co].abs().max()) > 0 and int((dw != 0).flatten(1).any(1).sum()) == 1


@pytest.mark.parametrize("name", ["f", "h", "d"])
def test_two_runs_and_two_streams_give_the_same_bits(name):
    c = R.CASES[name]
    first = run(name, 0.125)
    again = run(name, 0.125)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    handles = [CG().ConvGrad(c.cin, c.cout, CG().Geom(*c.geo), 0.125, DEV) for _ in streams]
    outs = []
    for s, h in zip(streams, handles):                               # both enqueued before either is awaited
        with torch.cuda.stream(s):
            x, w, b, dy = operands(name)["gpu"]
            y = h.forward(x, w, b)
            outs.append((y,) + h.backward(x, w, y, dy))
    torch.cuda.synchronize()
    for got in outs:
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, first))
    for h in handles:
        h.close()


def test_refusals():
    from yolo355 import _ffi
    M = CG()
    x, w, b, dy = operands("a")["gpu"]
    with pytest.raises(NotImplementedError):
        M.geometry(33, 1, 1)
    for geom, text in ((M.Geom(33, 3, 1, 1, 1, 1, 1, 1, 1, 1), "kernel size must be 1..32"), (M.Geom(3, 3, 1, 1, 1, 1, 1, 1, 65, 1), "padding must be 0..64")):
        with pytest.raises(_ffi.Y355Error, match=text):
            M.ConvGrad(3, 16, geom, 1.0, DEV)
    with pytest.raises(_ffi.Y355Error, match="no such device"):
        M.ConvGrad(3, 16, M.geometry(3, 1, 1), 1.0, "cuda:%d" % torch.cuda.device_count())
    h = handle("a", 0.125)
    y = h.forward(x, w, b)
    with pytest.raises(_ffi.Y355Error, match="y is needed unless neg_slope is 1") as e:
        h.backward(x, w, None, dy)
    assert e.value.code == -1
    big = M.ConvGrad(3, 16, M.Geom(12, 3, 1, 1, 1, 1, 1, 1, 1, 1), 1.0, DEV)       # 12 rows of kernel on 9 + 2 rows of map
    with pytest.raises(_ffi.Y355Error, match="larger than the padded input"):
        big.forward(x, torch.zeros(16, 3, 12, 3, device=DEV), None)
    big.close()
    for bad in (x.cpu(), x.double(), x[:, :2]):
        with pytest.raises(ValueError):
            h.forward(bad, w, b)
    with pytest.raises(ValueError):
        h.backward(x, w, y, dy[:, :, :-1])
    assert torch.equal(h.forward(x, w, b), y)                        # the handle is as it was


@pytest.mark.parametrize("name,slope", [("d", 0.1), ("c", 0.0), ("b", 1.0), ("a", 0.125)])
def test_conv2d_under_autograd_is_the_c_abi(name, slope):
    M = CG()
    c = R.CASES[name]
    g = c.geo
    want = run(name, slope)
    x, w, b = (t.clone().requires_grad_(True) for t in operands(name)["gpu"][:3])
    dy = operands(name)["gpu"][3]
    geom = M.Geom(*g)
    y = M._Conv2dFn.apply(x, w, b, geom, slope)
    y.backward(dy)
    for got, ref in zip((y.detach(), x.grad, w.grad, b.grad), want):
        assert torch.equal(got.cpu(), ref)
    h = M._handle_for(geom, c.cin, c.cout, slope, x.device)
    assert h.last_request == (True, True, True)
    # only what autograd needs is asked of the library: a first layer needs no dx, a convolution without bias no db
    x0 = operands(name)["gpu"][0]
    w.grad = None
    M._Conv2dFn.apply(x0, w, None, geom, slope).backward(dy)
    assert h.last_request == (False, True, False) and w.grad is not None
    M._Conv2dFn.apply(x, w.detach(), b.detach(), geom, slope).backward(dy)
    assert h.last_request == (True, False, False)
    if g.pad_top == g.pad_bottom and g.pad_left == g.pad_right:      # the public signature, where nn.Conv2d's padding can say it
        y2 = M.conv2d(x0, w.detach(), b.detach(), stride=(g.stride_h, g.stride_w), padding=(g.pad_top, g.pad_left), dilation=(g.dil_h, g.dil_w),
                      neg_slope=slope)
        assert torch.equal(y2.cpu(), want[0])


# ------------------------------------------------------------------------------------------------------------ a composed net
A, C, SIZE, STRIDE = 3, 2, [64, 64], 2
ANCHORS = [[2.0, 3.0], [5.0, 4.0], [9.0, 12.0]]                      # grid units (one level)
LABELS = [[[0.10, 0.15, 0.45, 0.60, 0], [0.55, 0.50, 0.95, 0.90, 1]], [[0.30, 0.25, 0.70, 0.80, 1]]]


class Net(nn.Module):
    def __init__(self):
        from yolo355.utils import modules as Mod
        super().__init__()
        self.c1 = Mod.Conv2d(3, 16, 3, padding=1, stride=2, leakyReLU=True)
        self.c2 = Mod.Conv2d_fuse(16, 32, 1, leakyReLU=True)
        self.c3 = Mod.Conv2d_fuse(32, 32, 3, padding="same", dilation=2, leakyReLU=True)
        self.pred = nn.Conv2d(32, A * (5 + C), 1)


class EmuConv(torch.autograd.Function):
    """the contract in the tensors' own type (float64, or float32 for the CPU emulation): operands rounded to bf16, G rounded"""

    @staticmethod
    def forward(ctx, x, w, b, g, slope):
        xr, wr = R.rb(x.detach().float()).to(x.dtype), R.rb(w.detach().float()).to(x.dtype)
        _, y = R.forward(xr, wr, b.detach(), g, slope)
        ctx.save_for_backward(xr, wr, y)
        ctx.g, ctx.slope = g, slope
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, wr, y = ctx.saved_tensors
        G = R.grad_out(dy, y, ctx.slope).to(dy.dtype)
        dx, dw, db = R.backward(xr, wr, G, ctx.g)
        return dx, dw, db, None, None


def emulate(net, x, dtype, crit):
    """(gradients by parameter name, total loss) of the first step in `dtype` on the CPU; the loss and its gradient map are the
    GPU library's on the emulation's prediction"""
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in net.named_parameters()}
    c1, c2, c3 = net.c1.convs[0], net.c2.convs[0], net.c3.convs[0]
    geo_of = lambda conv: R.Geo(*CG().geometry(conv.kernel_size, conv.stride, conv.padding, conv.dilation).astuple())
    a = EmuConv.apply(x.to(dtype), p["c1.convs.0.weight"], p["c1.convs.0.bias"], geo_of(c1), 1.0)
    a = F.leaky_relu(F.batch_norm(a, None, None, p["c1.convs.1.weight"], p["c1.convs.1.bias"], True, 0.1, net.c1.convs[1].eps), 0.125)
    a = EmuConv.apply(a, p["c2.convs.0.weight"], p["c2.convs.0.bias"], geo_of(c2), 0.125)
    a = EmuConv.apply(a, p["c3.convs.0.weight"], p["c3.convs.0.bias"], geo_of(c3), 0.125)
    pred = EmuConv.apply(a, p["pred.weight"], p["pred.bias"], geo_of(net.pred), 1.0)
    out, _, gmaps = crit.handle.forward_backward(pred.detach().float().to(DEV))
    names = list(p)
    grads = torch.autograd.grad(pred, [p[k] for k in names], gmaps[0].cpu().to(dtype))
    return dict(zip(names, grads)), float(out[3])


def test_four_block_net_trains_through_trainable_conv():
    """Conv2d (BN in training mode) -> Conv2d_fuse 1x1 -> Conv2d_fuse 3x3 dilation 2 'same' -> pred on a 2 x 3 x 64 x 64 input:
    per parameter the relative L2 distance of the GPU gradient from the float64 emulation is at most 2 d_emu + 1e-6, d_emu the
    distance of the float32 CPU emulation; three SGD steps lower the loss; the inference drop-in sees the new parameters"""
    from yolo355 import grad as G, synth
    M = CG()
    torch.manual_seed(3)
    net = Net().to(DEV)
    net.train()
    t = M.trainable(net)
    assert list(t) == ["c1", "c2", "c3", "pred"]
    x = torch.from_numpy(synth.uniform_pm1(77, (2, 3, 64, 64)))
    xg = x.to(DEV)
    crit = G.YoloCriterion(SIZE, STRIDE, ANCHORS, C, max_batch=2, max_labels_per_image=16)
    crit.handle.set_labels(LABELS)
    g64, loss64 = emulate(net, x, torch.float64, crit)
    g32, loss32 = emulate(net, x, torch.float32, crit)

    net.eval()
    x2 = torch.from_numpy(synth.uniform_pm1(78, (1, 16, 8, 8))).to(DEV)
    before = net.c2(x2).clone()                                      # the inference drop-in, before the updates
    net.train()

    forward = lambda: t["pred"](t["c3"](t["c2"](t["c1"](xg))))
    opt = torch.optim.SGD(net.parameters(), lr=2e-4)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = crit(forward(), label_lists=LABELS)[3]
        loss.backward()
        losses.append(float(loss.detach()))
        if step == 0:
            rel = lambda a, b: float((a.double() - b).norm() / b.norm())
            for k, p in net.named_parameters():
                d_gpu, d_emu = rel(p.grad.cpu(), g64[k]), rel(g32[k], g64[k])
                print("DIST %-20s gpu %.4g  float32 emulation %.4g" % (k, d_gpu, d_emu))
            for k, p in net.named_parameters():
                assert float(g64[k].norm()) > 0
                assert rel(p.grad.cpu(), g64[k]) <= 2 * rel(g32[k], g64[k]) + 1e-6, k
        opt.step()
    with torch.no_grad():
        losses.append(float(crit(forward(), label_lists=LABELS)[3]))
    print("losses", losses, "emulation", loss64, loss32)
    assert losses[3] < losses[0]

    net.eval()
    after = net.c2(x2)
    conv = net.c2.convs[0]
    ref = R.forward(R.rb(x2.cpu()).double(), R.rb(conv.weight.detach().cpu()).double(), conv.bias.detach().cpu().double(), R.geo(1), 0.125)[1]
    assert not torch.equal(before, after)
    assert ((after.cpu().double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all()       # the bf16 route rounds its result
    crit.close()
