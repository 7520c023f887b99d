"""TEST INFRASTRUCTURE -- host restatement of the quantisation-aware training step of csrc/qtrain.hip
in NumPy / torch float64, where every value of the forward is exact.

    fq_e(v) = clip(rne(v 2^e), -127, 127) 2^-e            rne = round half to even (torch.round)

quantize_masters   the weight / bias rule: m = max|T|, e = the exponent field of fl32(127 / m), q = clip(rne(T 2^e))
forward            A_0 = fq(x); z = conv(A_{k-1}, Wq_k) + bq_k; v = leaky(z); the 2x2 maximum of v with the first position on
                   ties; A_k = fq(.); P = fq(conv + bq); the state bytes S_k (bits 0-1 the window position, bit 2 the
                   selected z <= 0, bit 3 clipped); per tracker max|v| and the count of |rne(v 2^e)| > 127 before the pool
backward           the straight-through rule written out: G_10 = dP [not clipped], G_{k-1} = unpool(conv_transpose(G_k, Wq_k))
                   (bit 2 ? 0.125 : 1) (bit 3 ? 0 : 1), dW_k, db_k from G_k and A_{k-1}; round_g=True rounds every G to bf16
                   as the GPU does (the emulation the whole-step tolerance is taken from)
FakeQuant / Net    the same rule as a torch.autograd.Function and the network built on it, for autograd to differentiate
"""
import numpy as np
import torch
import torch.nn.functional as F

import bf16_layer_ref as BL
import train_cases as TC
import train_ref as TR
from qtrain_cases import exact_exponent

S_POS, S_NEG, S_CLIP = 3, 4, 8
SLOPE = 0.125


def quantize_tensor(t):
    """(q int32, e) of an fp32 tensor by the exact rule; the integers and the scaling are exact in float64"""
    t = np.asarray(t, np.float32)
    e = exact_exponent(np.abs(t).max()) if t.size else 0
    q = np.clip(np.rint(np.ldexp(t.astype(np.float64), e)), -127, 127)
    return q.astype(np.int32), e


def quantize_masters(ws):
    """[(w, b)] fp32 masters -> [{q_w, e_w, q_b, e_b}]"""
    out = []
    for w, b in ws:
        qw, ew = quantize_tensor(w)
        qb, eb = quantize_tensor(b)
        out.append(dict(q_w=qw, e_w=ew, q_b=qb, e_b=eb))
    return out


def dequant(ql):
    """[(Wq, bq)] float64 tensors"""
    return [(torch.from_numpy(np.ldexp(L["q_w"].astype(np.float64), -L["e_w"])), torch.from_numpy(np.ldexp(L["q_b"].astype(np.float64), -L["e_b"])))
            for L in ql]


def fq(v, e):
    """(fq_e(v), clipped) of a float64 tensor"""
    r = torch.round(v * 2.0 ** e)
    return r.clamp(-127, 127) * 2.0 ** -e, r.abs() > 127


def forward(ql, x, e_a):
    """dict(A [A_0..A_9], S {k: uint8}, P, max_abs float32 [11], clipped int [11]) of the quantised layers ql on x (fp32
    array) at the activation exponents e_a"""
    wq = dequant(ql)
    x = torch.from_numpy(np.asarray(x, np.float32)).double()
    mx, nclip = [float(x.abs().max())], []
    a, c = fq(x, e_a[0])
    nclip.append(int(c.sum()))
    A, S = [a], {}
    for k in range(1, 11):
        z = TR.conv(A[-1], wq[k - 1][0], wq[k - 1][1])
        v = TR.leaky(z) if k < 10 else z
        mx.append(float(v.abs().max()))
        nclip.append(int((torch.round(v * 2.0 ** e_a[k]).abs() > 127).sum()))
        pos = torch.zeros((), dtype=torch.uint8)
        if k < 10 and TC.POOL[k - 1]:
            v, pos = TR.pool_first(v)
        a, c = fq(v, e_a[k])
        neg = (v <= 0).to(torch.uint8) * S_NEG if k < 10 else 0
        S[k] = (pos + neg + c.to(torch.uint8) * S_CLIP).to(torch.uint8)
        if k < 10:
            A.append(a)
    return dict(A=A, S=S, P=a, max_abs=np.array(mx, np.float32), clipped=np.array(nclip, np.int64))


def state_factor(S):
    """the factor of the data gradient an element's state byte stands for: (bit 2 ? 0.125 : 1) (bit 3 ? 0 : 1)"""
    S = S.long()
    return torch.where((S & S_NEG) != 0, SLOPE, 1.0).double() * ((S & S_CLIP) == 0).double()


def backward(ql, A, S, dP, round_g=False):
    """([(dW_k, db_k)], {k: G_k}) float64 by the straight-through rule; round_g: every G_k rounded to bf16"""
    wq = dequant(ql)
    rnd = BL.rb if round_g else (lambda t: t)
    G = {10: rnd(torch.as_tensor(dP).double() * ((S[10].long() & S_CLIP) == 0).double())}
    grads = [None] * 10
    for k in range(10, 0, -1):
        grads[k - 1] = TR.wgrad(G[k], A[k - 1])
        if k == 1:
            break
        D = TR.dgrad(G[k], wq[k - 1][0]) * state_factor(S[k - 1])
        G[k - 1] = rnd(TR.unpool(D, S[k - 1].long() & S_POS) if TC.POOL[k - 2] else D)
    return grads, G


class FakeQuant(torch.autograd.Function):
    """fq_e with the straight-through gradient: 1 where the element was not clipped, 0 where it was"""

    @staticmethod
    def forward(ctx, v, e):
        out, clipped = fq(v, e)
        ctx.save_for_backward(clipped)
        return out

    @staticmethod
    def backward(ctx, g):
        (clipped,) = ctx.saved_tensors
        return g * (~clipped).to(g.dtype), None


class StePow2(torch.autograd.Function):
    """the weight / bias quantiser: the exact rule forward, the gradient passed through"""

    @staticmethod
    def forward(ctx, t):
        q, e = quantize_tensor(t.detach().to(torch.float32).numpy())
        return torch.from_numpy(np.ldexp(q.astype(np.float64), -e)).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def net(ws, x, e_a):
    """P of the network on float64 leaf tensors ws [(W, b)] (the masters), built from FakeQuant / StePow2 for autograd; the
    pool takes the first maximum, the slope 0.125 applies to z <= 0"""
    a = FakeQuant.apply(torch.from_numpy(np.asarray(x, np.float32)).double(), e_a[0])
    for k in range(1, 11):
        w, b = ws[k - 1]
        z = F.conv2d(a, StePow2.apply(w), StePow2.apply(b), 1, 1)
        if k < 10:
            z = torch.where(z > 0, z, z * SLOPE)
            if TC.POOL[k - 1]:
                win = TR.windows(z)
                z = torch.gather(win, -1, TR.pool_first(z.detach())[1].long().unsqueeze(-1)).squeeze(-1)
        a = FakeQuant.apply(z, e_a[k])
    return a


def autograd_grads(ws_np, x, e_a, dP):
    """[(dW_k, db_k)] float64 of net by torch.autograd, for the upstream gradient dP"""
    ws = [(torch.from_numpy(np.asarray(w, np.float32)).double().requires_grad_(), torch.from_numpy(np.asarray(b, np.float32)).double().requires_grad_())
          for w, b in ws_np]
    P = net(ws, x, e_a)
    P.backward(torch.as_tensor(dP).double())
    return [(w.grad, b.grad) for w, b in ws], P.detach()


def emulate_steps(ws_np, x_np, e_a, target, size, C, lr, n, momentum=0.9, weight_decay=5e-4):
    """n steps of the restatement on one fixed batch (exact forward, G rounded to bf16, float64 sums, train_ref.sgd): the total
    loss of the quantised forward before each update, then the masters"""
    ws = [(np.array(w, np.float32), np.array(b, np.float32)) for w, b in ws_np]
    bufs = [(None, None)] * 10
    losses = []
    for it in range(n):
        ql = quantize_masters(ws)
        f = forward(ql, x_np, e_a)
        out, dP = TR.loss_and_dpred(f["P"], target, size, C)
        losses.append(float(out[3]))
        grads, _ = backward(ql, f["A"], f["S"], dP.astype(np.float32), round_g=True)
        for k in range(10):
            (w, b), (dw, db), (mw, mb) = ws[k], grads[k], bufs[k]
            w, mw = TR.sgd(w, dw.numpy().astype(np.float32), mw, lr, momentum, weight_decay, it == 0)
            b, mb = TR.sgd(b, db.numpy().astype(np.float32), mb, lr, momentum, weight_decay, it == 0)
            ws[k], bufs[k] = (w, b), (mw, mb)
    return losses, ws
