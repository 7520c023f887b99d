"""TEST INFRASTRUCTURE -- layer-local float64 reference of the bf16 form of the five y355_net graphs (csrc/net.hip) and the
per-element interval check that judges the engine's tensors with it.

After a forward, every tensor read with get_tensor holds the engine's own bf16 values, exactly.  For every op of the graph
the op is recomputed in float64 FROM THE ENGINE'S OWN INPUT TENSORS and the engine's output is checked element by element
against an interval derived from the fp32 arithmetic of that one op.  Nothing accumulates across layers.

Op tables: int8_wide_ref.GRAPHS for yolo_v2 / yolo_v3 / yolo_v3_spp; kSlimOps and kTinyOps of csrc/net_arch.h are restated
here (slim_graph, tiny_graph) in the same form.  A conv whose input tensor is -1 reads the network input (conv1f / frontb).

THE ROUNDING CONTRACT of the bf16 path (read from y355_net_load_layer_f32, y355_convg_pack / y355_pack_conv1f /
y355_pack_frontb / y355_convpxb_pack, and the epilogues of convg.hip, convr.hip, convpxb.hip, frontb.hip, netops.hip; the same
paragraph is DESIGN.md section 6, "Rounding contract of the bf16 path"):
  input     the fp32 network input is rounded to bf16, round-to-nearest-even (RNE): by the input op (input_bf16_kernel) of the
            DarkNet graphs, by the patch load of conv1_bf16_kernel / frontb_kernel in slim and tiny.  Padding is zero.
  weights   Wb = RNE-bf16 of the BN-folded fp32 weight the caller hands to y355_net_load_layer_f32 (y355_bf16_rne in every
            packer; the fold itself is the caller's, in float64, rounded once to fp32).
  bias      kept as the fp32 value given (zero when absent); never rounded to bf16.
  sum       products of bf16 operands accumulated in fp32 by v_mfma_f32_16x16x32_bf16 from a zero accumulator (convpxb.hip: from
            the bias as the C operand); the bias otherwise added in fp32 after the sum.
  pool      a fused 2x2 / stride 2 max-pool is taken on the fp32 accumulators BEFORE bias and LeakyReLU (both monotone, so the
            value is that of pooling the activated map).
  slope     LeakyReLU in fp32 with the fp32 constant 0.1f or 0.125f (act_slope): x >= 0 ? x : x * slope, one rounding.
  residual  the residual tensor's bf16 value, exact in fp32, is added in fp32 AFTER the activation (one rounding).
  output    RNE to bf16 (the __bf16 conversion), once; prediction maps are stored as the fp32 value, unrounded.
  between   frontb.hip rounds conv1's pooled map to bf16 (RNE) in LDS exactly where the two-launch path stores it.
  pool, reorg, SPP  exact selections of bf16 values; SPP windows are clipped to the map, the stride-1 pool of YOLOv3tiny takes
            the zero halo as its padding (right and bottom).
  upsample  bilinear x2, align_corners: ratio r = fl((n-1)/(2n-1)), s = fl(r * y), y0 = int(s), l = s - y0 (exact), h = fl(1 - l),
            v = hy*(hx*f00 + lx*f01) + ly*(hx*f10 + lx*f11) in fp32, RNE to bf16.

THE BOUND of a convolution, per output element, with u = 2^-24 (the unit round-off of fp32 RNE):
  z   = float64 of: conv(X, Wb) + b, LeakyReLU with float64(float32(slope)), + residual
  S   = conv(|X|, |Wb|) + |b|, computed in float32 and multiplied by 1.001 (it is only a tolerance)
  K   = cin * k^2 + 1 terms
  e   = 2 K u S 1.001  +  u |z before the residual|  +  u |z|        (the last term only where a residual is added)
  The first term is the textbook bound (K - 1) u S for summing K exact products in any order with rounded fp32 additions
  (products of two bf16 values are exact in fp32), DOUBLED so that an adder that truncates instead of rounding is still covered:
  the guide states that the f32 MFMA is an fma chain and says nothing about the bf16 one.  The second term is the slope
  multiplication's rounding, the third the residual addition's.
  bf16 output:  rb(z - e) <= got <= rb(z + e), rb = RNE to bf16; with a fused pool both sides take the maximum over the window
  (rb and max are monotone).  fp32 output: |got - z| <= e.
  rho: the smallest c for which got lies in [rb(z - c u S), rb(z + c u S)]: the distance from z to got's rounding cell (the set
  of reals that round to got) over u S; with a pool, the smallest c for which some window element reaches the cell from below
  and none lies beyond it above.

THE BOUND of the bilinear x2: e = c u max|the four taps| 1.001 with c = 6 + 4 (Hin + Win - 2), from the kernel's own operation count:
  blend: 6 multiplications and 3 additions (an fma contraction only removes roundings), each at most u times a value bounded by
         max|taps| = M because the weights of each axis sum to 1: inner sums 2 u M, outer products and sum 2 u M;        4 u M
  h = fl(1 - l): one rounding per axis, u h M each;                                                                       2 u M
  s = fl(fl((n-1)/(2n-1)) * y): two roundings, |s^ - s| <= 2 u (n - 1) per axis; the blend is piecewise linear in s with
         slope at most 2 M (a difference of two taps);                                            4 u M (Hin - 1) + 4 u M (Win - 1)
  A wrong cell (int(s^) != floor(s)) can happen only where s is an integer, i.e. in the last row / column (s = n - 1: fractional
  parts are multiples of 1 / (2n - 1), far above 2 u n); the reference therefore takes y0 = min(floor(s), n - 2) so that its four
  taps are the ones either choice blends.

Other ops: input got == rb(x); pool / reorg / SPP array_equal with the float64 op on the engine's input.
Channels of an output tensor that no op writes (padding: DarkNet-53's first map holds 32 real channels of 64) must be zero.
Every channel range of a concat buffer is compared with the reference of the op that owns it (the tensors are read once,
after the forward, so a range another op overwrote fails at its owner).
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

import int8_wide_ref as R

U = 2.0 ** -24
L100, L125, NONE = R.L100, R.L125, R.NONE
FAMILY = {1: "FIRST", 2: "FRONT", 3: "RING", 5: "GENERIC4", 6: "GENERIC8", 7: "THIN"}
CONV_FAMILIES = ("FIRST", "FRONT", "RING", "THIN", "GENERIC4", "GENERIC8")


# ---------------------------------------------------------------------------------------------------- op tables
def slim_graph():
    """kSlimOps / kSlimT of csrc/net_arch.h"""
    g = R.Graph()
    for C, d in [(16, 2), (32, 4), (64, 4), (64, 8), (128, 8), (128, 16), (256, 16), (256, 16), (256, 16), (None, 16)]:
        g.T(C, d)
    g.conv(-1, 0, 0, 3, 16, 3, L125, pool=1)
    for i, (ci, co, pool) in enumerate([(16, 32, 1), (32, 64, 0), (64, 64, 1), (64, 128, 0), (128, 128, 1), (128, 256, 0),
                                        (256, 256, 0), (256, 256, 0)]):
        g.conv(i, i + 1, 0, ci, co, 3, L125, pool=pool)
    g.conv(8, 9, 0, 256, None, 3, NONE)
    g.pred = [9]
    g.strides = [16]
    return g


def tiny_graph():
    """kTinyOps / kTinyT of csrc/net_arch.h; tensor 4 is the concat buffer [C_4 (256) | up(conv_1x1_2) (128)]"""
    g = R.Graph()
    for C, d in [(16, 2), (32, 4), (64, 8), (128, 16), (384, 16), (256, 32), (512, 32), (512, 32), (1024, 32), (256, 32),
                 (128, 32), (256, 16), (512, 32), (None, 16), (None, 32)]:
        g.T(C, d)
    g.conv(-1, 0, 0, 3, 16, 3, L100, pool=1)
    g.conv(0, 1, 0, 16, 32, 3, L100, pool=1)
    g.conv(1, 2, 0, 32, 64, 3, L100, pool=1)
    g.conv(2, 3, 0, 64, 128, 3, L100, pool=1)
    g.conv(3, 4, 0, 128, 256, 3, L100)
    g.add("pool", 4, 5, C=256)
    g.conv(5, 6, 0, 256, 512, 3, L100)
    g.add("pool", 6, 7, s1=1)                    # ZeroPad2d((0, 1, 0, 1)) + MaxPool(2, 1)
    g.conv(7, 8, 0, 512, 1024, 3, L100)
    g.conv(8, 9, 0, 1024, 256, 3, L125)
    g.conv(9, 10, 0, 256, 128, 1, L125)
    g.add("up", 10, 4, choff=256)
    g.conv(4, 11, 0, 384, 256, 3, L125)
    g.conv(9, 12, 0, 256, 512, 3, L125)
    g.conv(12, 14, 0, 512, None, 1, NONE)
    g.conv(11, 13, 0, 256, None, 1, NONE)
    g.pred = [13, 14]
    g.strides = [16, 32]
    return g


GRAPHS = dict(R.GRAPHS, slim_yolo_v2=slim_graph, tiny_yolo_v3=tiny_graph)


def fold_layers(layers):
    """[(w fp32, b fp32)] of synth.make_fp32_model's layers: the float64 fold the drop-ins and tests/test_fp32_models.py hand
    to load_layer (W g, (b - mean) g + beta, g = gamma / sqrt(var + eps)), rounded once to fp32"""
    from oracle import fp32_oracle as FP
    out = []
    for L in layers:
        w, b = L["w"].astype(np.float64), L["b"].astype(np.float64)
        if L["bn"] is not None:
            g, be, mu, var = (a.astype(np.float64) for a in L["bn"])
            s = g / np.sqrt(var + FP.EPS)
            w, b = w * s[:, None, None, None], (b - mu) * s + be
        out.append((w.astype(np.float32), b.astype(np.float32)))
    return out


# ---------------------------------------------------------------------------------------------------- bf16 on the bit pattern
_BF16_MAX = float.fromhex("0x1.fep127")


def t64(a):
    if isinstance(a, torch.Tensor):
        return a.double()
    return torch.from_numpy(np.array(a, dtype=np.float64))


def rb(x):
    """round-to-nearest-even of float64 values to bf16 (1 + 8 + 7 bits), returned as float64: on the float64 bit pattern the low
    45 of the 52 fraction bits go, with the carry running into the exponent; below 2^-126 (bf16 subnormals) the grid is 2^-133"""
    x = t64(x).contiguous()
    bits = x.view(torch.int64)
    r = (bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) & ~((1 << 45) - 1)
    r = r.view(torch.float64)
    sub = torch.round(x * 2.0 ** 133) * 2.0 ** -133          # torch.round: half to even
    r = torch.where(x.abs() < 2.0 ** -126, sub, r)
    return torch.where(r.abs() > _BF16_MAX, torch.sign(r) * float("inf"), r)


def trunc_bf16(x):
    """truncation (round toward zero) to bf16: what the contract does NOT allow (mutation 7)"""
    x = t64(x).contiguous()
    return (x.view(torch.int64) & ~((1 << 45) - 1)).view(torch.float64)


def bf16_cell(g):
    """(lo, hi): the reals that round (RNE) to the bf16 value g -- half a step either side, a quarter below a power of two"""
    g = t64(g)
    a = g.abs()
    m, ex = torch.frexp(a)                                     # a = m 2^ex, m in [0.5, 1): one step is 2^(ex - 8)
    step = torch.clamp(torch.ldexp(torch.ones_like(a), ex - 8), min=2.0 ** -133)
    out = step / 2
    inn = torch.where((m == 0.5) & (a > 2.0 ** -126), step / 4, step / 2)
    zero = a == 0
    out = torch.where(zero, torch.full_like(a, 2.0 ** -134), out)
    inn = torch.where(zero, torch.full_like(a, 2.0 ** -134), inn)
    neg = g < 0
    return g - torch.where(neg, out, inn), g + torch.where(neg, inn, out)


def bf16_next(g, up=True):
    """the neighbouring bf16 value above (below) g, normal range"""
    lo, hi = bf16_cell(g)
    return rb(hi + (hi - t64(g)) * 0.5) if up else rb(lo - (t64(g) - lo) * 0.5)


# ---------------------------------------------------------------------------------------------------- one op in float64
def _slope64(act):
    return None if act is None else float(np.float32(act))


def _windows(t, pool):
    """[B, C, Ho, Wo, n]: the n elements the output element takes its maximum over"""
    if not pool:
        return t.unsqueeze(-1)
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def conv_terms(o, X, w32, b32, res=None):
    """z, z before the residual, S and e of a convolution on its pre-pool grid (module docstring)"""
    Wb = rb(t64(w32))
    b = t64(b32)
    stride, pad = (2 if o["s2"] else 1), o["k"] // 2
    a = F.conv2d(X, Wb, b, stride, pad)
    sl = _slope64(o["act"])
    zc = a if sl is None else torch.where(a >= 0, a, a * sl)
    z = zc if res is None else zc + res
    S = F.conv2d(X.abs().float(), Wb.abs().float(), b.abs().float(), stride, pad).double() * 1.001
    K = o["cin"] * o["k"] ** 2 + 1
    e = 2 * K * U * S * 1.001 + U * zc.abs()
    if res is not None:
        e = e + U * z.abs()
    return z, zc, S, e


def interval_stats(got, z, e, S, pool=0, fp32_out=False, extra=None, want_mask=False):
    """the interval check and rho of one op's own channels.  got [B,C,Ho,Wo] float64; z, e, S on the pre-pool grid; extra: a
    further tolerance added to both sides (the fused front end's intermediate rounding)"""
    zw, ew, sw = _windows(z, pool), _windows(e, pool), _windows(S, pool)
    if extra is not None:
        ew = ew + _windows(extra, pool)
    tw = torch.clamp(U * sw, min=1e-300)
    xw = torch.zeros_like(zw) if extra is None else _windows(extra, pool)
    if fp32_out:
        bad = (got - zw[..., 0]).abs() > ew[..., 0]
        rho = torch.clamp((got - zw[..., 0]).abs() - xw[..., 0], min=0) / tw[..., 0]
        exact = got == zw[..., 0].float().double()
    else:
        lo, hi = rb((zw - ew).amax(-1)), rb((zw + ew).amax(-1))
        bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
        clo, chi = bf16_cell(got)
        up = ((clo.unsqueeze(-1) - zw - xw) / tw).amin(-1)          # some window element reaches the cell from below
        dn = ((zw - xw - chi.unsqueeze(-1)) / tw).amax(-1)          # none lies beyond it
        rho = torch.clamp(torch.maximum(up, dn), min=0)
        exact = got == rb(zw.amax(-1))
    n = got.numel()
    flat = rho.flatten()
    k = min(n, max(1, int(np.ceil(0.999 * n))))
    st = dict(n=n, bad=int(bad.sum()), first=[tuple(int(v) for v in c) for c in torch.nonzero(bad)[:5]],
              exact=float(exact.double().mean()), rho_max=float(flat.max()), rho_999=float(torch.kthvalue(flat, k).values))
    if want_mask:
        st["mask"] = bad.numpy()
    return st


def upsample_terms(X):
    """z and e of the bilinear x2 (align_corners) of X [B,C,H,W] float64"""
    B, C, H, W = X.shape
    assert H >= 2 and W >= 2

    def axis(n):
        s = torch.arange(2 * n, dtype=torch.float64) * (n - 1) / (2 * n - 1)
        i0 = torch.clamp(torch.floor(s), max=n - 2).long()
        return i0, s - i0

    y0, ly = axis(H)
    x0, lx = axis(W)
    ly, lx = ly.view(1, 1, -1, 1), lx.view(1, 1, 1, -1)
    r0, r1 = X[:, :, y0], X[:, :, y0 + 1]
    f00, f01, f10, f11 = r0[:, :, :, x0], r0[:, :, :, x0 + 1], r1[:, :, :, x0], r1[:, :, :, x0 + 1]
    z = (1 - ly) * ((1 - lx) * f00 + lx * f01) + ly * ((1 - lx) * f10 + lx * f11)
    M = torch.stack([f00.abs(), f01.abs(), f10.abs(), f11.abs()]).amax(0)
    c = 6 + 4 * (H + W - 2)
    return z, c * U * M * 1.001, M


def pool_ref(X, s1=False):
    if s1:
        return F.max_pool2d(F.pad(X, (0, 1, 0, 1)), 2, 1)
    return F.max_pool2d(X, 2, 2)


def _exact_stats(got, want, want_mask=False):
    bad = got != want
    st = dict(n=got.numel(), bad=int(bad.sum()), first=[tuple(int(v) for v in c) for c in torch.nonzero(bad)[:5]],
              exact=float((~bad).double().mean()), rho_max=0.0, rho_999=0.0)
    if want_mask:
        st["mask"] = bad.numpy()
    return st


# ---------------------------------------------------------------------------------------------------- the whole graph
def owned_channels(g, t):
    """boolean per channel of tensor t: some op writes it"""
    C = g.C[t]
    own = np.zeros(0 if C is None else C, bool)
    if C is None:
        return own
    for o in g.ops:
        if o["o"] != t:
            continue
        if o["op"] == "conv":
            own[o["choff"]:o["choff"] + o["cout"]] = True
        elif o["op"] == "input":
            own[:3] = True
        elif o["op"] == "spp":
            own[o["C"]:4 * o["C"]] = True
        elif o["op"] == "reorg":
            own[o["choff"]:o["choff"] + 4 * g.C[o["i"]]] = True
        elif o["op"] == "up":
            own[o["choff"]:o["choff"] + g.C[o["i"]]] = True
        else:
            own[:] = True
    return own


def op_name(g, idx):
    o = g.ops[idx]
    if o["op"] == "conv":
        return "op %d conv%dx%d%s%s%s layer %d (t%d[:%d] -> t%d[%d:])" % (
            idx, o["k"], o["k"], " +pool" if o["pool"] else "", " /2" if o["s2"] else "", " +res t%d" % o["res"] if o["res"] >= 0 else "",
            o["layer"], o["i"], o["cin"], o["o"], o["choff"])
    return "op %d %s (t%d -> t%d)" % (idx, o["op"], o["i"], o["o"])


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        if a is not None:
            h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    return h.hexdigest()


def check_op(g, idx, x, weights, T, want_mask=False):
    """the report of op idx of graph g on tensors T (fp32 [B,C,H,W] per tensor, the engine's values) and network input x"""
    o = g.ops[idx]
    kind = o["op"]
    out = t64(T[o["o"]])
    if kind == "conv":
        X = rb(t64(x)) if o["i"] < 0 else t64(T[o["i"]])[:, :o["cin"]]
        w32, b32 = weights[o["layer"]]
        res = t64(T[o["res"]]) if o["res"] >= 0 else None
        z, zc, S, e = conv_terms(o, X, w32, b32, res)
        cout = w32.shape[0]
        st = interval_stats(out[:, o["choff"]:o["choff"] + cout], z, e, S, o["pool"], g.C[o["o"]] is None, want_mask=want_mask)
    elif kind == "input":
        st = _exact_stats(out[:, :3], rb(t64(x)), want_mask)
    elif kind == "pool":
        X = t64(T[o["i"]])
        st = _exact_stats(out, pool_ref(X[:, :o.get("C", X.shape[1])], bool(o.get("s1"))), want_mask)
    elif kind == "reorg":
        r = t64(R.reorg(np.asarray(T[o["i"]]), o["s"]))
        st = _exact_stats(out[:, o["choff"]:o["choff"] + r.shape[1]], r, want_mask)
    elif kind == "spp":
        C = o["C"]
        want = torch.cat([F.max_pool2d(out[:, :C], k, 1, k // 2) for k in (5, 9, 13)], 1)
        st = _exact_stats(out[:, C:4 * C], want, want_mask)
    elif kind == "up":
        z, e, M = upsample_terms(t64(T[o["i"]]))
        st = interval_stats(out[:, o["choff"]:o["choff"] + z.shape[1]], z, e, M, want_mask=want_mask)
    else:
        raise ValueError(kind)
    own = owned_channels(g, o["o"])
    st["pad_bad"] = int((out[:, torch.from_numpy(~own)] != 0).sum()) if own.size and not own.all() else 0
    st.update(op=idx, name=op_name(g, idx), kind=kind, layer=o.get("layer", -1))
    return st


def check_graph(arch, x, weights, T, routes=None, ops=None, cache=None):
    """reports of the ops of a graph (all, or those in `ops`).  routes: y355_net_layer_route per weight slot of the forward
    that wrote T.  cache: a dict that remembers an op's report by the bytes of its inputs and output (a second forward through
    the same kernels on the same inputs costs a hash, not a convolution)."""
    g = GRAPHS[arch]()
    reports = []
    for idx, o in enumerate(g.ops):
        if ops is not None and idx not in ops:
            continue
        key = None
        if cache is not None:
            key = (arch, idx, _digest(x if o["i"] < 0 else T[o["i"]], T[o["res"]] if o.get("res", -1) >= 0 else None, T[o["o"]]))
        if key is not None and key in cache:
            st = dict(cache[key])
        else:
            st = check_op(g, idx, x, weights, T)
            if key is not None:
                cache[key] = dict(st)
        st["family"] = FAMILY.get(routes[st["layer"]] & 0xff, "?%d" % routes[st["layer"]]) if (routes is not None and st["layer"] >= 0) else st["kind"].upper()
        st["route"] = routes[st["layer"]] if (routes is not None and st["layer"] >= 0) else 0
        reports.append(st)
    return reports


def check_front(arch, x, weights, T1, want_mask=False):
    """the fused front end (frontb.hip) of slim / tiny: tensor 1 from the network input through both layers.  The intermediate
    map is conv1's pooled float64 value rounded to bf16 where frontb.hip rounds it; where that value lies within its own e of a
    rounding boundary the kernel's intermediate may be the other neighbour, one bf16 step u1 away, and the bound of conv2 grows
    by conv(u1, |W2b|)."""
    g = GRAPHS[arch]()
    o0, o1 = g.ops[0], g.ops[1]
    X = rb(t64(x))
    z1, _, S1, e1 = conv_terms(o0, X, *weights[o0["layer"]])
    zw, ew = _windows(z1, 1), _windows(e1, 1)
    mid = rb(zw.amax(-1))
    u1 = rb((zw + ew).amax(-1)) - rb((zw - ew).amax(-1))                # one step where the rounding is ambiguous, else 0
    w2, b2 = weights[o1["layer"]]
    z2, _, S2, e2 = conv_terms(o1, mid, w2, b2)
    extra = F.conv2d(u1, rb(t64(w2)).abs(), None, 1, 1)
    st = interval_stats(t64(T1)[:, :w2.shape[0]], z2, e2, S2, 1, extra=extra, want_mask=want_mask)
    st.update(op=1, name="fused front end (network input -> t1)", kind="conv", layer=o1["layer"], family="FRONT", route=2, pad_bad=0,
              ambiguous=float((u1 > 0).double().mean()))
    return st


def describe(reports):
    """the failure message: op, route family and coordinates (b, c, y, x) of the first elements outside their interval"""
    lines = []
    for r in reports:
        if r["bad"] or r.get("pad_bad"):
            lines.append("%s on %s: %d of %d elements outside their interval, first at (b, c, y, x) = %s; %d nonzero padding values" % (
                r["name"], r["family"], r["bad"], r["n"], r["first"], r.get("pad_bad", 0)))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- CPU emulation
def emulate_op(g, idx, x, weights, T, slope=None, wmod=None, bmod=None, res_shift=0, trunc=False, up_align=True, pool_shift=0):
    """the bf16 path of one op on the CPU: torch float32 on the bf16-rounded operands, the contract's rounding points, RNE to
    bf16 -- a legitimate fp32 accumulation in another order.  Returns the op's own channels (fp32 array).  The keyword
    arguments are the mutations of tests/test_bf16_layers_ref.py."""
    o = g.ops[idx]
    kind = o["op"]
    if kind == "conv":
        X = rb(t64(x)).float() if o["i"] < 0 else torch.from_numpy(T[o["i"]][:, :o["cin"]].copy())
        w32, b32 = weights[o["layer"]]
        w = rb(t64(w32 if wmod is None else wmod(w32.copy()))).float()
        b = torch.from_numpy(b32 if bmod is None else bmod(b32.copy()))
        y = F.conv2d(X, w, b, 2 if o["s2"] else 1, o["k"] // 2)
        act = o["act"] if slope is None else slope
        if act is not None:
            y = torch.where(y >= 0, y, y * torch.tensor(np.float32(act)))
        if o["res"] >= 0:
            r = torch.from_numpy(T[o["res"]].copy())
            if res_shift:
                r = torch.roll(r, res_shift, 3)
            y = y + r
        if o["pool"]:
            y = F.max_pool2d(torch.roll(y, -pool_shift, 3) if pool_shift else y, 2, 2)
        if g.C[o["o"]] is None:
            return y.numpy()
        return (trunc_bf16(y) if trunc else rb(y)).float().numpy()
    if kind == "input":
        return rb(t64(x)).float().numpy()
    if kind == "pool":
        X = torch.from_numpy(T[o["i"]][:, :o.get("C", T[o["i"]].shape[1])].copy())
        return pool_ref(torch.roll(X, -pool_shift, 3) if pool_shift else X, bool(o.get("s1"))).numpy()
    if kind == "reorg":
        return R.reorg(T[o["i"]], o["s"])
    if kind == "spp":
        X = torch.from_numpy(T[o["o"]][:, :o["C"]].copy())
        return torch.cat([F.max_pool2d(X, k, 1, k // 2) for k in (5, 9, 13)], 1).numpy()
    if kind == "up":
        y = F.interpolate(torch.from_numpy(T[o["i"]].copy()), scale_factor=2.0, mode="bilinear", align_corners=up_align)
        return rb(y).float().numpy()
    raise ValueError(kind)


def place(g, idx, T, y):
    """write an op's own channels y into its output tensor"""
    o = g.ops[idx]
    off = {"conv": o.get("choff", 0), "reorg": o.get("choff", 0), "up": o.get("choff", 0), "spp": o.get("C", 0)}.get(o["op"], 0)
    T[o["o"]][:, off:off + y.shape[1]] = y


def emulate(arch, x, weights, predc):
    """every tensor of the graph, the emulated outputs chained as inputs"""
    g = GRAPHS[arch]()
    B, _, H, W = x.shape
    T = [np.zeros(R._shape(g, t, B, H, W, predc), np.float32) for t in range(len(g.C))]
    for idx in range(len(g.ops)):
        place(g, idx, T, emulate_op(g, idx, x, weights, T))
    return T


# ---------------------------------------------------------------------------------------------------- cases
# (tag, arch, [H, W], B): the smallest sizes that still reach the kernels production uses (maps below 13 x 13 select the small
# tile, so the stride-32 layers run their production kernels only from 416 on)
CASES = [
    ("slim_320x416_b1", "slim_yolo_v2", [320, 416], 1),
    ("slim_96x160_b2", "slim_yolo_v2", [96, 160], 2),
    ("tiny_416_b1", "tiny_yolo_v3", [416, 416], 1),
    ("tiny_224x320_b2", "tiny_yolo_v3", [224, 320], 2),
    ("v2_416_b1", "yolo_v2", [416, 416], 1),
    ("v2_224x320_b2", "yolo_v2", [224, 320], 2),
    ("v3_224x320_b2", "yolo_v3", [224, 320], 2),
    ("v3_416_b1", "yolo_v3", [416, 416], 1),         # the stride-32 layers of DarkNet-53 reach their eight-wave kernels only here
    ("spp_416_b1", "yolo_v3_spp", [416, 416], 1),
]
ARCHS = ("slim_yolo_v2", "tiny_yolo_v3", "yolo_v2", "yolo_v3", "yolo_v3_spp")
SMALLEST = {"slim_yolo_v2": "slim_96x160_b2", "tiny_yolo_v3": "tiny_224x320_b2", "yolo_v2": "v2_224x320_b2",
            "yolo_v3": "v3_224x320_b2", "yolo_v3_spp": "spp_416_b1"}
# weights of slim / tiny: the FP32_CASES row (tests/cases.py) whose model the graph takes; the wide families: class, classes,
# seed and gain of tests/test_int8_wide_models.py
_FP32_ROW = {"slim_yolo_v2": "slim_voc", "tiny_yolo_v3": "tiny_b2"}
_WIDE = {"yolo_v2": ("myYOLOv2", 20, 4100, 2.0), "yolo_v3": ("myYOLOv3", 20, 4200, 1.3), "yolo_v3_spp": ("myYOLOv3Spp", 20, 4300, 1.3)}
_MODELS = {}


def model_of(arch):
    """dict(weights [(w fp32, b fp32)] per weight slot, anchors, classes, predc) of a graph, built once"""
    if arch in _MODELS:
        return _MODELS[arch]
    from yolo355 import synth
    if arch in _FP32_ROW:
        from cases import FP32_CASES, fp32_anchors
        row = next(c for c in FP32_CASES if c[0] == _FP32_ROW[arch])
        classes = row[3]
        anchors = fp32_anchors(arch, classes)
        A = len(anchors) if arch == "slim_yolo_v2" else len(anchors) // 2
        layers = synth.make_fp32_model(arch, row[4], classes, A, pred_gain=row[7], obj_bias=row[8])
        m = dict(weights=fold_layers(layers), anchors=anchors, classes=classes, predc=A * (5 + classes), seed=row[4])
    else:
        from test_int8_wide_models import _model
        from yolo355.utils.modules import folded_f32
        cls, classes, seed, gain = _WIDE[arch]
        net, anchors = _model(arch, cls, [416, 416], classes, seed, gain)
        m = dict(weights=[folded_f32(c) for c in net._conv_modules()], anchors=anchors, classes=classes,
                 predc=net.anchor_number * (5 + classes), seed=seed)
    _MODELS[arch] = m
    return m


def images_of(arch, size, B):
    """synth.make_images with the noise pattern, one seed per image: no two pixels are equal, so a swapped row or column shows"""
    from yolo355 import synth
    seed = model_of(arch)["seed"]
    return np.concatenate([synth.make_images(seed + 1 + i, 1, size[0], size[1], pattern="noise") for i in range(B)])
