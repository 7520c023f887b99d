"""libyolo355_convgrad.so on the GPU against the float64 restatement of its contract (tests/convgrad_ref.py): every element of
y, dx, dw and db of the table's cases inside the interval 2 K u S 1.001 + u |value|; the exact properties (zeros of dx where
no window reaches, an all-zero dy, a one-hot dy, the same bits from run to run and on two streams); the refusals; conv2d under
torch.autograd; and a four-block net of the drop-ins trained through TrainableConv with yolo355.grad.YoloCriterion and
torch.optim.SGD.  Beside the table: the run-length cases (R.RUNS), whose weight gradient walks two and three iterations of 32
pixels per run, with exact checks aimed at what the loop carries from one iteration to the next; the geometry's limits
(R.EDGES); and the thirteen convolutions yolo355.tools.convgrad_bench times, at a small map."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convgrad_ref as R
from yolo355.tools.convgrad_bench import tiny_v3_layers

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


def every_element(c, o, slope, bias, got, name):
    """y, dx (None: not asked for), dw and db (None without bias) of one call on the case c with the operands o, each element
    inside the interval of its float64 value"""
    y, dx, dw, db = got
    x, w, b, dy = o["cpu"]
    g, taps = c.geo, c.geo.kh * c.geo.kw
    ho, wo = R.out_size(g, c.H, c.W)
    b64 = b.double() if bias else None
    z64, y64 = R.forward(o["xr"], o["wr"], b64, g, slope)
    S = R.forward(o["xr"].abs(), o["wr"].abs(), None if b64 is None else b64.abs(), g, 1.0)[0]
    inside(y, y64, c.cin * taps + (1 if bias else 0) + 1, S, "%s slope %g bias %d y" % (name, slope, bias))
    # the mask from the GPU's own y: a sign that flipped at |z| <= e is not counted twice
    G = R.grad_out(dy, y, slope).double()
    dx64, dw64, db64 = R.backward(o["xr"], o["wr"], G, g)
    Sx, Sw, Sb = R.backward(o["xr"].abs(), o["wr"].abs(), G.abs(), g)
    if dx is not None:
        inside(dx, dx64, c.cout * taps + 1, Sx, "%s slope %g bias %d dx" % (name, slope, bias))
    inside(dw, dw64, c.B * ho * wo + 1, Sw, "%s slope %g bias %d dw" % (name, slope, bias))
    if bias:
        inside(db, db64, c.B * ho * wo + 1, Sb, "%s slope %g db" % (name, slope))
    else:
        assert db is None
    assert float(dw64.abs().max()) > 0 and float(dx64.abs().max()) > 0


# the table and the two stride-2 cases at every slope; the run-length cases at two (their float64 references are the largest);
# the geometry edges at every slope (p64 is in both lists: every slope)
ELEMENT_CASES = ([(n, s) for n in R.TABLE + ("s2k1", "s2p0") for s in R.SLOPES] + [(n, s) for n in R.RUNS if n not in R.EDGES for s in R.RUN_SLOPES] +
                 [(n, s) for n in R.EDGES for s in R.SLOPES])


@pytest.mark.parametrize("name,slope", ELEMENT_CASES)
def test_every_element_against_float64(name, slope):
    c, o = R.CASES[name], operands(name)
    for bias in (True, False):
        every_element(c, o, slope, bias, run(name, slope, bias), name)


@pytest.mark.parametrize("name", R.RUNS)
def test_run_length_cases_run_the_pixel_loop_more_than_once(name):
    """every run but the last takes two iterations of 32 pixels (three in r2), there are several runs, and the last one is
    shorter and ends inside a lane's group of eight"""
    c = R.CASES[name]
    plan = handle(name, 1.0).wgrad_plan(c.B, c.H, c.W)
    print(name, plan)
    assert plan["npix"] == c.B * int(np.prod(R.out_size(c.geo, c.H, c.W))) and (plan["runs"] - 1) * plan["chunk"] + plan["last"] == plan["npix"]
    assert plan["chunk"] >= 64
    assert plan["runs"] >= 2
    assert 0 < plan["last"] < plan["chunk"]
    assert plan["last"] % 8 != 0
    if name == "r2":
        assert plan["chunk"] >= 96


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


@pytest.mark.parametrize("name", ["s2k1", "s2p0", "c", "d", "s16", "s53", "mix", "d32"])
def test_dx_is_zero_where_no_window_reaches(name):
    c = R.CASES[name]
    x, w, b, dy = operands(name)["gpu"]
    h = handle(name, 1.0)
    dx, _, _ = raw_backward(h, x, w, None, dy)
    m = torch.from_numpy(R.untouched(c.geo, c.H, c.W))
    print(name, "untouched pixels", int(m.sum()))
    if name.startswith("s2") or name in ("s16", "s53"):
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


# -------------------------------------------------------------------------------- the pixel loop, iteration after iteration
# r1 and r4: runs of 64 pixels, two iterations of 32 each.  A dy of a few ones leaves at most one fp32 addition per element of
# dw, and operands of ones leave small integers, so no order of summation can change a bit: a pixel dropped, counted twice or
# read at another pixel's place at an iteration or run boundary shows as a wrong bit, not as a figure inside an interval.
def one_hot_backward(name, ats):
    """(dx, dw, db) at slope 1 from NaN-filled tensors for dy = 1 at the flat output pixels and channels `ats` = [(q, co)]"""
    c = R.CASES[name]
    x, w, b, dy = operands(name)["gpu"]
    one = torch.zeros_like(dy)
    for q, co in ats:
        bi, oy, ox = R.pixel(c, q)
        one[bi, co, oy, ox] = 1.0
    return raw_backward(handle(name, 1.0), x, w, None, one)


ONE_HOTS = ([(n, w) for n in ("r1", "r4") for w in ("first_iteration", "second_iteration_first_pixel", "second_iteration_first_group_end",
                                                   "last_pixel_of_last_run")] + [("r2", "first_pixel_of_image_1"), ("r3", "first_pixel_of_image_1")])


@pytest.mark.parametrize("name,where", ONE_HOTS)
def test_one_hot_dy_in_a_later_iteration_makes_dw_the_rounded_patch(name, where):
    """dy = 1 at one pixel: dw[co] is the rb(x) patch under that pixel's window bit for bit, every other row is zero, db is the
    one-hot.  The pixels: in run 1 (the second run) one that the loop meets in its first iteration, with another iteration to
    follow (chunk + 3), and two that it meets in its second, the first of the iteration (chunk + 32) and the last of the first
    lane group's eight (chunk + 39); the last pixel of the last run; in r2 and r3, whose 169 pixels per image are no multiple
    of 8, the first pixel of image 1, which a lane group of a later iteration reaches by walking over the image boundary"""
    c, o = R.CASES[name], operands(name)
    plan = handle(name, 1.0).wgrad_plan(c.B, c.H, c.W)
    hwo = int(np.prod(R.out_size(c.geo, c.H, c.W)))
    q = {"first_iteration": plan["chunk"] + 3, "second_iteration_first_pixel": plan["chunk"] + 32, "second_iteration_first_group_end": plan["chunk"] + 39,
         "last_pixel_of_last_run": plan["npix"] - 1, "first_pixel_of_image_1": hwo}[where]
    assert plan["chunk"] >= 64 and q < plan["npix"]
    if "iteration" in where:
        assert q // plan["chunk"] == 1
    if where == "first_pixel_of_image_1":
        assert hwo % 8 != 0 and q % plan["chunk"] >= 32
    co = q * 7 % c.cout
    dx, dw, db = one_hot_backward(name, [(q, co)])
    want = torch.zeros_like(dw)
    want[co] = R.patch(c, o["xr"], *R.pixel(c, q))
    hot = torch.zeros(c.cout)
    hot[co] = 1.0
    print(name, where, "pixel", q, R.pixel(c, q), "co", co, "nonzeros of the patch", int((want != 0).sum()))
    assert int((want[co] != 0).sum()) >= c.cin * min(4, c.geo.kh * c.geo.kw)       # a corner's window keeps four taps of nine
    assert torch.equal(dw, want) and torch.equal(db, hot) and torch.isfinite(dx).all()


@pytest.mark.parametrize("name", ["r1", "r4", "r2"])
def test_two_ones_in_two_iterations_of_one_run_add_their_patches(name):
    """dy = 1 at pixels chunk + 3 and chunk + 35 of one output channel -- the same lane and element in the first and in the
    second iteration of run 1: dw[co] = fl32(patch1 + patch2), one fp32 addition of two bf16 values per element, db[co] = 2"""
    c, o = R.CASES[name], operands(name)
    plan = handle(name, 1.0).wgrad_plan(c.B, c.H, c.W)
    q1, q2, co = plan["chunk"] + 3, plan["chunk"] + 35, c.cout - 3
    assert plan["chunk"] >= 64 and q2 < 2 * plan["chunk"] <= plan["npix"]
    dx, dw, db = one_hot_backward(name, [(q1, co), (q2, co)])
    p1, p2 = R.patch(c, o["xr"], *R.pixel(c, q1)), R.patch(c, o["xr"], *R.pixel(c, q2))
    want = torch.zeros_like(dw)
    want[co] = p1 + p2                                               # float32: rounded once
    two = torch.zeros(c.cout)
    two[co] = 2.0
    assert int(((p1 != 0) & (p2 != 0)).sum()) >= c.cin * 4 and not torch.equal(p1, p2)
    assert torch.equal(dw, want) and torch.equal(db, two) and torch.isfinite(dx).all()


@pytest.mark.parametrize("name", ["r1", "r4", "r2", "r3"])
def test_ones_count_the_pixels_under_every_tap(name):
    """x = 1 and dy = 1 everywhere: db[co] is the number of output pixels and dw[co, ci, tap] the number of them whose tap lies
    inside the map -- integers below 2^24, exact in fp32 in any order; the float64 restatement on the same tensors counts them"""
    c = R.CASES[name]
    x, w, b, dy = operands(name)["gpu"]
    dx, dw, db = raw_backward(handle(name, 1.0), torch.ones_like(x), w, None, torch.ones_like(dy))
    _, dw64, db64 = R.backward(torch.ones(x.shape, dtype=torch.float64), operands(name)["wr"], torch.ones(dy.shape, dtype=torch.float64), c.geo)
    npix = c.B * int(np.prod(R.out_size(c.geo, c.H, c.W)))
    assert torch.equal(dw64, dw64.round()) and 0 < float(dw64.min()) and float(dw64.max()) <= npix < 2 ** 24
    assert (float(dw64.min()) < npix) == (c.geo.kh * c.geo.kw > 1) and (db64 == npix).all()      # the border taps of a 3x3 miss some pixels
    print(name, "pixels", npix, "counts", sorted(set(dw64.flatten().tolist())), "worst difference", float((dw.double() - dw64).abs().max()))
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64) and torch.isfinite(dx).all()


# ------------------------------------------------------------------------------------------- the pad and dilation limits
@pytest.mark.parametrize("name", ["p64", "d32"])
def test_windows_wholly_in_the_padding_give_the_bias(name):
    """where S, the forward of |x|, |w| without bias, is zero, the window lies wholly in the padding: y is float32(bias) where
    that is positive and float32(bias) * float32(slope) elsewhere, bit for bit, and zero without bias"""
    c, o = R.CASES[name], operands(name)
    x, w, b, dy = o["gpu"]
    empty = R.forward(o["xr"].abs(), o["wr"].abs(), None, c.geo, 1.0)[0] == 0
    print(name, "outputs wholly in the padding", int(empty.sum()), "of", empty.numel())
    assert empty.any() and not empty.all()
    if name == "p64":
        assert 2 * int(empty.sum()) > empty.numel()
    bf = o["cpu"][2]
    assert (bf > 0).any() and (bf < 0).any()
    for slope in R.SLOPES:
        want = torch.where(bf > 0, bf, bf * torch.tensor(slope, dtype=torch.float32)).view(1, -1, 1, 1).expand(empty.shape)
        y = handle(name, slope).forward(x, w, b).cpu()
        assert torch.equal(y[empty], want[empty]), slope
        assert (handle(name, slope).forward(x, w, None).cpu()[empty] == 0).all(), slope


@pytest.mark.parametrize("name", ["p64", "d32"])
def test_taps_that_never_meet_the_map_have_zero_rows_of_dw(name):
    """R.dead_taps from the geometry (none in p64, whose every tap meets the map under some window)"""
    c = R.CASES[name]
    x, w, b, dy = operands(name)["gpu"]
    dead = torch.from_numpy(R.dead_taps(c.geo, c.H, c.W))
    print(name, "taps that never meet the map", int(dead.sum()), "of", dead.numel())
    if name == "p64":
        assert not dead.any()
    dx, dw, db = raw_backward(handle(name, 1.0), x, w, None, dy)
    assert torch.isfinite(dw).all() and (dw[:, :, dead] == 0).all() and (dw[:, :, ~dead] != 0).flatten(0, 1).any(0).all()


# ------------------------------------------------------------------------------- the thirteen convolutions the bench times
LAYERS = tiny_v3_layers(20, 32, 32)


@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_the_benchmarked_convolutions_against_float64(layer):
    """YOLOv3tiny's convolutions as yolo355.tools.convgrad_bench runs them -- conv2d under autograd, stride 1, padding k // 2,
    bias, the first layer without x.grad -- at 1 x 32 x 32 (maps 32 x 32 down to 1 x 1), slope 0.1, operands from the CPU
    generator: y and the three gradients inside the interval of test_every_element_against_float64"""
    M = CG()
    name, cin, cout, k, h, w = layer
    c = R.Case(R.geo(k, 1, k // 2), cin, cout, 1, h, w)
    cpu = R.make_inputs(c, 50000 + 1000 * LAYERS.index(layer))
    o = dict(cpu=cpu, xr=R.rb(cpu[0]).double(), wr=R.rb(cpu[1]).double())
    x, wt, b, dy = (t.to(DEV) for t in cpu)
    first = cin == 3
    x.requires_grad_(not first)
    wt.requires_grad_(True)
    b.requires_grad_(True)
    y = M.conv2d(x, wt, b, 1, k // 2, neg_slope=0.1)
    y.backward(dy)
    hnd = M._handle_for(M.geometry(k, 1, k // 2), cin, cout, 0.1, x.device)
    print(name, hnd.wgrad_plan(1, h, w), "asked", hnd.last_request)
    assert hnd.last_request == (not first, True, True) and (x.grad is None) == first
    every_element(c, o, 0.1, True, (y.detach().cpu(), None if first else x.grad.cpu(), wt.grad.cpu(), b.grad.cpu()), name)


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
