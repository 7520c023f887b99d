"""TEST INFRASTRUCTURE -- host restatement of the BatchNorm training step of csrc/bntrain.hip, on the ops
of tests/train_ref.py.

`step` chains one forward in training mode + loss gradient + backward of the ten-layer network in two forms:

  contract=False   plain float64 arithmetic: the restatement that is pinned to the reference's own backward()
                   (tests/golden/bntrain.npz) and to torch's float64 autograd;
  contract=True    the emulation of the contract in fp32: A_0 = rb(x), rb(W_k), Z_k = rb(...), statistics and the two
                   backward sums in float64 rounded once, every per-element operation a separately rounded fp32 operation,
                   A_k = rb(...), dY_k = rb(...), G_k = rb(...); convolution sums in fp32 (torch's order, not the GPU's).

The per-element operations are also restated on NumPy float32 arrays (normalise_pool, bn_apply), which the GPU's A_k, I_k and
G_k are compared with bit for bit, and the statistics in float64 NumPy with their summation bounds (batch_stats_f64,
bn_sums_f64).  `sgd` is train_ref's."""
import numpy as np
import torch

import bntrain_cases as BC
import train_ref as TR

U = TR.U
EPS, MOMENTUM = 1e-5, 0.1
SLOPE = np.float32(0.125)
sgd = TR.sgd


# ---------------------------------------------------------------------------------------------------- NumPy, as the GPU does it
def f32(a):
    return np.asarray(a, np.float32)


def bits_to_f32(a):
    """uint16 bf16 bit patterns -> float32 (exact)"""
    return (np.ascontiguousarray(a).astype(np.uint32) << 16).view(np.float32)


def rb_bits(a):
    """float32 -> the bf16 bit patterns of round-to-nearest-even (no NaN in the tests' data)"""
    u = np.ascontiguousarray(f32(a)).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _c(v):
    return f32(v).reshape(1, -1, 1, 1)


def xhat32(Z, mean, invstd):
    """(Z - mean) * invstd, two fp32 roundings; Z float32 [B, C, h, w], the statistics [C]"""
    return (f32(Z) - _c(mean)) * _c(invstd)


def normalise_pool(Z, mean, invstd, gamma, beta, pool):
    """(A bits uint16, I uint8 or None) from Z float32 NCHW: xhat, y = xhat * gamma + beta, LeakyReLU, the 2x2 pool on the fp32
    values with the first maximum's position, rb"""
    y = xhat32(Z, mean, invstd) * _c(gamma) + _c(beta)
    v = np.where(y > 0, y, y * SLOPE).astype(np.float32)
    if not pool:
        return rb_bits(v), None
    B, C, H, W = v.shape
    w = v.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    pos = np.argmax(w, -1)                                   # the first one on ties
    return rb_bits(np.take_along_axis(w, pos[..., None], -1)[..., 0]), pos.astype(np.uint8)


def bn_apply(dY, Z, mean, invstd, dgamma, dbeta, gamma, N):
    """G bits uint16: m1 = dbeta / N, m2 = dgamma / N, t = dY - m1, t = t - xhat * m2, t * (gamma * invstd), rb; all fp32"""
    n = np.float32(N)
    m1, m2 = f32(dbeta) / n, f32(dgamma) / n
    t = f32(dY) - _c(m1)
    t = t - xhat32(Z, mean, invstd) * _c(m2)
    return rb_bits(t * _c(f32(gamma) * f32(invstd)))


def batch_stats_f64(Z):
    """float64 statistics of Z (float32 or float64 NCHW) per channel and the bound of a float64 sum in any order:
    dict(N, mean, var, invstd, unbiased, e_mean, e_var, e_invstd) -- e_*: N 2^-53 sum |terms|, propagated"""
    Z = np.asarray(Z, np.float64)
    N = Z.shape[0] * Z.shape[2] * Z.shape[3]
    s, q = Z.sum((0, 2, 3)), (Z * Z).sum((0, 2, 3))
    es, eq = N * 2.0 ** -53 * np.abs(Z).sum((0, 2, 3)), N * 2.0 ** -53 * q
    mean = s / N
    raw = q / N - mean * mean
    var = np.maximum(raw, 0.0)
    e_mean = es / N + 2.0 ** -52 * np.abs(mean)
    e_var = eq / N + 2 * np.abs(mean) * e_mean + e_mean ** 2 + 2.0 ** -51 * (q / N + mean * mean)
    invstd = 1.0 / np.sqrt(var + EPS)
    e_invstd = 0.5 * invstd ** 3 * e_var * 1.001 + 2.0 ** -51 * invstd
    return dict(N=N, mean=mean, var=var, invstd=invstd, unbiased=var * N / (N - 1), e_mean=e_mean, e_var=e_var, e_invstd=e_invstd)


def within_one_rounding(got, want, e):
    """got (float32) is a float32 rounding of some value within e of want (float64): between fl(want - e) and fl(want + e)"""
    got, want, e = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(e, np.float64)
    lo, hi = (want - e).astype(np.float32).astype(np.float64), (want + e).astype(np.float32).astype(np.float64)
    return (got >= lo) & (got <= hi)


def running_f64(before, batch_value):
    return (1.0 - MOMENTUM) * np.asarray(before, np.float64) + MOMENTUM * np.asarray(batch_value, np.float64)


def bn_sums_f64(dY, Z, mean, invstd):
    """(dbeta, dgamma, e_dbeta, e_dgamma) in float64 from dY and Z (float32 NCHW) with xhat restated in fp32"""
    d = np.asarray(dY, np.float64)
    t = d * xhat32(Z, mean, invstd).astype(np.float64)
    N = d.shape[0] * d.shape[2] * d.shape[3]
    ax = (0, 2, 3)
    return d.sum(ax), t.sum(ax), N * 2.0 ** -53 * np.abs(d).sum(ax), N * 2.0 ** -53 * np.abs(t).sum(ax)


# ---------------------------------------------------------------------------------------------------- the network (torch)
def tensors(layers, dt):
    """[(w, b, gamma, beta)] (pred: gamma = beta = None) of a parameter list as tensors of type dt"""
    out = []
    for L in layers:
        t = lambda v: torch.from_numpy(np.array(v)).to(dt)
        out.append((t(L["w"]), t(L["b"]), t(L["bn"][0]) if L["bn"] else None, t(L["bn"][1]) if L["bn"] else None))
    return out


def _ch(v):
    return v.view(1, -1, 1, 1)


def bn_forward(Z, gamma, beta, contract):
    """-> (v, cache); v = leaky(xhat * gamma + beta) on the pre-pool grid"""
    N = Z.shape[0] * Z.shape[2] * Z.shape[3]
    Zd = Z.double()
    mean64 = Zd.sum((0, 2, 3)) / N
    var64 = ((Zd * Zd).sum((0, 2, 3)) / N - mean64 * mean64).clamp(min=0.0)
    if not contract:                                          # the two-pass form: no cancellation to speak of
        var64 = ((Zd - _ch(mean64)) ** 2).sum((0, 2, 3)) / N
    mean, invstd = mean64.to(Z.dtype), (1.0 / torch.sqrt(var64 + EPS)).to(Z.dtype)
    xhat = (Z - _ch(mean)) * _ch(invstd)
    y = xhat * _ch(gamma) + _ch(beta)
    return TR.leaky(y), dict(xhat=xhat, invstd=invstd, mean64=mean64, var64=var64, N=N)


def undecided_windows(I_lo, I_hi):
    """int64 [n, 3] = (k, flat index into I_k, the position I_lo took): the pooling windows in which two forwards of one input
    (fp32 and float64) select different positions -- two values fp32 cannot tell apart.  The gradient goes to one pixel or to
    its neighbour, so the float64 restatement that is compared with an fp32 run takes that run's position."""
    rows = []
    for k in sorted(I_hi):
        lo, hi = I_lo[k].reshape(-1), I_hi[k].reshape(-1)
        for i in torch.nonzero(lo != hi).reshape(-1).tolist():
            rows.append((k, i, int(lo[i])))
    return np.array(rows, np.int64).reshape(-1, 3)


def forward(ps, x, contract, picks=None):
    """-> (A [A_0..A_9], I {k: positions}, caches {k}, P).  ps: tensors(...) of x's type.  picks: rows of undecided_windows;
    those windows take the row's position."""
    rnd = TR.rb32 if contract else (lambda t: t)
    A, I, cache = [rnd(x)], {}, {}
    for k in range(1, 10):
        w, b, g, be = ps[k - 1]
        Z = rnd(TR.conv(A[-1], rnd(w), b))
        v, cache[k] = bn_forward(Z, g, be, contract)
        cache[k]["Z"] = Z
        if BC.POOL[k - 1]:
            win = TR.windows(v)
            v, I[k] = TR.pool_first(v)
            rows = [r for r in ([] if picks is None else np.asarray(picks).reshape(-1, 3).tolist()) if r[0] == k]
            if rows:
                I[k] = I[k].clone()
                for _, i, pos in rows:
                    I[k].view(-1)[i] = pos
                v = torch.gather(win, -1, I[k].long().unsqueeze(-1)).squeeze(-1)
        A.append(rnd(v))
    w, b, _, _ = ps[9]
    return A, I, cache, TR.conv(A[-1], rnd(w), b)


def bn_backward(dY, gamma, c, contract):
    """-> (G, dgamma, dbeta)"""
    rnd = TR.rb32 if contract else (lambda t: t)
    dbeta = dY.double().sum((0, 2, 3)).to(dY.dtype)
    dgamma = (dY.double() * c["xhat"].double()).sum((0, 2, 3)).to(dY.dtype)
    n = torch.tensor(float(c["N"]), dtype=dY.dtype)
    t = dY - _ch(dbeta / n)
    t = t - c["xhat"] * _ch(dgamma / n)
    return rnd(t * _ch(gamma * c["invstd"])), dgamma, dbeta


def backward(ps, A, I, cache, dP, contract, sides=None):
    """-> ([(dW_k, db_k, dgamma_k, dbeta_k)] for k = 1..10 (pred: the last two None), {k: G_k}, {k: dY_k}).  sides: rows of
    train_ref.undecided_sides; the slope of those elements is taken from the row, not from the sign of A."""
    rnd = TR.rb32 if contract else (lambda t: t)
    G, DY = {10: rnd(dP)}, {}
    grads = [None] * 10
    for k in range(10, 0, -1):
        dg = db = None
        if k <= 9:
            G[k], dg, db = bn_backward(DY[k], ps[k - 1][2], cache[k], contract)
        grads[k - 1] = TR.wgrad(G[k], A[k - 1]) + (dg, db)
        if k == 1:
            break
        mask = TR.slope_mask(A[k - 1])
        for t, i, positive in ([] if sides is None else np.asarray(sides).reshape(-1, 3).tolist()):
            if t == k - 1:
                mask.view(-1)[i] = 1.0 if positive else TR.SLOPE
        D = TR.dgrad(G[k], rnd(ps[k - 1][0])) * mask
        DY[k - 1] = rnd(TR.unpool(D, I[k - 1]) if BC.POOL[k - 2] else D)
    return grads, G, DY


def step(layers, x_np, target, size, C, contract, sides=None, picks=None):
    """One forward + loss + backward.  sides, picks: see backward and forward.  Returns dict(losses float64 [4], grads [(dW, db, dgamma, dbeta)] float64 numpy, P,
    stats {k: (mean64, var64, N)})."""
    dt = torch.float32 if contract else torch.float64
    ps = tensors(layers, dt)
    x = torch.from_numpy(np.asarray(x_np)).to(dt)
    A, I, cache, P = forward(ps, x, contract, picks)
    out, dP = TR.loss_and_dpred(P, target, size, C)
    dPt = torch.from_numpy(dP.astype(np.float32)).to(dt) if contract else torch.from_numpy(dP)
    grads, _, _ = backward(ps, A, I, cache, dPt, contract, sides)
    n64 = lambda v: None if v is None else v.double().numpy()
    return dict(losses=out, grads=[tuple(n64(v) for v in g) for g in grads], P=P.double().numpy(),
                stats={k: (c["mean64"].numpy(), c["var64"].numpy(), c["N"]) for k, c in cache.items()})


def running_after(layers, stats):
    """{k: (running_mean, running_var)} float64 after one forward in training mode"""
    out = {}
    for k, (mean, var, N) in stats.items():
        out[k] = (running_f64(layers[k - 1]["bn"][2], mean), running_f64(layers[k - 1]["bn"][3], var * N / (N - 1)))
    return out


def emulate_steps(layers, x_np, target, size, C, lr, n, momentum=0.9, weight_decay=5e-4):
    """n steps of the emulation on one fixed batch: the total loss before each update"""
    layers = [dict(L, w=f32(L["w"]).copy(), b=f32(L["b"]).copy(), bn=tuple(f32(v).copy() for v in L["bn"]) if L["bn"] else None) for L in layers]
    bufs = [[None] * 4 for _ in range(10)]
    losses = []
    for it in range(n):
        r = step(layers, x_np, target, size, C, True)
        losses.append(float(r["losses"][3]))
        for k in range(10):
            L, g = layers[k], r["grads"][k]
            L["w"], bufs[k][0] = sgd(L["w"], f32(g[0]), bufs[k][0], lr, momentum, weight_decay, it == 0)
            L["b"], bufs[k][1] = sgd(L["b"], f32(g[1]), bufs[k][1], lr, momentum, weight_decay, it == 0)
            if L["bn"]:
                ga, bufs[k][2] = sgd(L["bn"][0], f32(g[2]), bufs[k][2], lr, momentum, weight_decay, it == 0)
                be, bufs[k][3] = sgd(L["bn"][1], f32(g[3]), bufs[k][3], lr, momentum, weight_decay, it == 0)
                L["bn"] = (ga, be) + tuple(L["bn"][2:])
    return losses


# ---------------------------------------------------------------------------------------------------- eval mode (the hand-over)
def eval_forward_f64(sd, x_np):
    """P of the BatchNorm network in eval mode (running statistics) in float64, from a state_dict of numpy / torch values"""
    g = lambda key: torch.as_tensor(np.asarray(sd[key])).double()
    A = torch.from_numpy(np.asarray(x_np)).double()
    for k in range(1, 10):
        kw, kb = BC.keys(k)
        ga, be, mu, var = (g(n) for n in BC.bn_keys(k))
        z = TR.conv(A, g(kw), g(kb))
        v = TR.leaky((z - _ch(mu)) / torch.sqrt(_ch(var) + EPS) * _ch(ga) + _ch(be))
        A = TR.pool_first(v)[0] if BC.POOL[k - 1] else v
    kw, kb = BC.keys(10)
    return TR.conv(A, g(kw), g(kb))
