"""TEST INFRASTRUCTURE -- host restatement of the training step of csrc/train.hip.

Every op of the step once, on torch tensors of any floating type (float64 for the references the GPU's tensors are judged
with): the convolution with bias and LeakyReLU 0.125, the 2x2 max-pool with the window position of the FIRST maximum, the
weight / bias gradient, the data gradient with the slope mask, the scatter through the stored positions.  `step` chains them
into one forward + loss gradient + backward of the ten-layer network in two forms:

  contract=False   plain arithmetic in the tensors' type: in float64 the restatement that is pinned to the reference's own
                   backward() (tests/golden/train.npz);
  contract=True    the emulation of the contract in fp32: A_0 = rb(x), rb(W_k), A_k = rb(...), G_k = rb(...), sums in
                   fp32 (torch's order, not the GPU's).

The loss and its gradient with respect to P are loss_ref / grad_ref's float64 on P as fp32 (what libyolo355_grad.so gets).
`sgd` is torch.optim.SGD (dampening 0, no Nesterov) in separately rounded fp32 NumPy operations."""
import numpy as np
import torch
import torch.nn.functional as F

import grad_ref as GR
import loss_ref as R
import train_cases as TC

U = 2.0 ** -24
SLOPE = 0.125


def rb32(t):
    """RNE to bf16, in the tensor's type"""
    return t.to(torch.bfloat16).to(t.dtype)


def bf16_bits_to_f64(a):
    """uint16 bf16 bit patterns -> float64 tensor"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).astype(np.float64))


# ---------------------------------------------------------------------------------------------------- the ops
def conv(X, W, b):
    return F.conv2d(X, W, b, 1, 1)


def leaky(z):
    return torch.where(z > 0, z, z * SLOPE)


def windows(t):
    """[B, C, H/2, W/2, 4]: the 2x2 windows, positions row-major"""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def pool_first(v):
    """(max, position of the first maximum in {0,1,2,3}) of every 2x2 window"""
    w = windows(v)
    m = w.amax(-1)
    pos = torch.where(w == m.unsqueeze(-1), torch.arange(4).view(1, 1, 1, 1, 4), torch.tensor(4)).amin(-1)
    return m, pos.to(torch.uint8)


def unpool(v, pos):
    """v [B,C,h,w] written to position pos of its window on the [B,C,2h,2w] grid, zeros elsewhere"""
    B, C, h, w = v.shape
    sel = (torch.arange(4).view(1, 1, 1, 1, 4) == pos.long().unsqueeze(-1)).to(v.dtype) * v.unsqueeze(-1)
    return sel.reshape(B, C, h, w, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h, 2 * w)


def wgrad(G, A):
    """dW [cout,cin,3,3] = sum G[b,co,y,x] A[b,ci,y+dy-1,x+dx-1] (zero padding) and db [cout]"""
    cout, cin = G.shape[1], A.shape[1]
    dW = torch.nn.grad.conv2d_weight(A, (cout, cin, 3, 3), G, stride=1, padding=1)
    return dW, G.sum((0, 2, 3))


def dgrad(G, W):
    """conv_transpose(G, W) on the input's grid"""
    return F.conv_transpose2d(G, W, None, 1, 1)


def slope_mask(A):
    return torch.where(A > 0, torch.ones_like(A), torch.full_like(A, SLOPE))


# ---------------------------------------------------------------------------------------------------- the network
def forward(ws, x, contract):
    """-> (A [A_0..A_9], I {k: positions}, P).  ws: [(w, b)] tensors of x's type."""
    rnd = rb32 if contract else (lambda t: t)
    A, I = [rnd(x)], {}
    for k in range(1, 10):
        w, b = ws[k - 1]
        v = leaky(conv(A[-1], rnd(w), b))
        if TC.POOL[k - 1]:
            v, I[k] = pool_first(v)
        A.append(rnd(v))
    w, b = ws[9]
    return A, I, conv(A[-1], rnd(w), b)


def undecided_sides(A_lo, A_hi):
    """int64 [n, 3] = (t, flat index into A_t, 1 where A_lo took the positive side): the elements of A_1..A_9 at which two
    forwards of one input (fp32 and float64) lie on different sides of the LeakyReLU, whose pre-activation fp32 cannot tell
    from zero.  There the gradient jumps by a factor of 8 and the side an fp32 forward takes is rounding noise."""
    rows = []
    for t in range(1, 10):
        lo, hi = (A_lo[t] > 0).reshape(-1), (A_hi[t] > 0).reshape(-1)
        for i in torch.nonzero(lo != hi).reshape(-1).tolist():
            rows.append((t, i, int(lo[i])))
    return np.array(rows, np.int64).reshape(-1, 3)


def backward(ws, A, I, dP, contract, sides=None):
    """-> ([(dW_k, db_k)] for k = 1..10, {k: G_k}).  sides: rows of undecided_sides; the slope of those elements is taken
    from the row, not from the sign of A."""
    rnd = rb32 if contract else (lambda t: t)
    G = {10: rnd(dP)}
    grads = [None] * 10
    for k in range(10, 0, -1):
        grads[k - 1] = wgrad(G[k], A[k - 1])
        if k == 1:
            break
        mask = slope_mask(A[k - 1])
        for t, i, positive in ([] if sides is None else np.asarray(sides).reshape(-1, 3).tolist()):
            if t == k - 1:
                mask.view(-1)[i] = 1.0 if positive else SLOPE
        D = dgrad(G[k], rnd(ws[k - 1][0])) * mask
        G[k - 1] = rnd(unpool(D, I[k - 1]) if TC.POOL[k - 2] else D)
    return grads, G


def loss_and_dpred(P, target, size, C):
    """(float64 [4] losses, dP float64 numpy) of P (a tensor; taken as fp32, as the loss library gets it)"""
    p32 = P.detach().to(torch.float32).numpy()
    out, _ = R.loss([p32], target, TC.STRIDE, TC.ANCHORS, C, size, float(TC.STRIDE))
    dP = GR.map_grads([p32], target, TC.STRIDE, TC.ANCHORS, C, size, float(TC.STRIDE))[0]
    return np.asarray(out, np.float64), dP


def targets(size, label_lists):
    return R.make_targets(size, TC.STRIDE, label_lists, TC.ANCHORS, False)


def step(ws_np, x_np, target, size, C, contract, sides=None):
    """One forward + loss + backward.  contract=False: float64; True: the fp32 emulation.  sides: see backward.  Returns
    (losses float64 [4], [(dW, db)] numpy float64, P numpy)."""
    dt = torch.float32 if contract else torch.float64
    ws = [(torch.from_numpy(np.asarray(w)).to(dt), torch.from_numpy(np.asarray(b)).to(dt)) for w, b in ws_np]
    x = torch.from_numpy(np.asarray(x_np)).to(dt)
    A, I, P = forward(ws, x, contract)
    out, dP = loss_and_dpred(P, target, size, C)
    grads, _ = backward(ws, A, I, torch.from_numpy(dP.astype(np.float32)).to(dt) if contract else torch.from_numpy(dP), contract, sides)
    return out, [(dw.double().numpy(), db.double().numpy()) for dw, db in grads], P.double().numpy()


# ---------------------------------------------------------------------------------------------------- SGD
def sgd(p, g, buf, lr, momentum, weight_decay, first):
    """one parameter array: fp32 in, (p, buf) fp32 out; every operation rounded on its own"""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    lr, momentum, weight_decay = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    g = g + weight_decay * p
    buf = g if first else momentum * np.asarray(buf, np.float32) + g
    return p - lr * buf, buf


def sgd_bound(p, g, buf, lr, weight_decay):
    """four roundings per element per step"""
    p, g, buf = (np.abs(np.asarray(v, np.float64)) for v in (p, g, buf))
    return 4 * U * (p + lr * (buf + g + weight_decay * p))


def emulate_steps(ws_np, x_np, target, size, C, lr, n, momentum=0.9, weight_decay=5e-4):
    """n steps of the emulation on one fixed batch: the total loss before each update"""
    ws = [(np.array(w, np.float32), np.array(b, np.float32)) for w, b in ws_np]
    bufs = [(None, None)] * 10
    losses = []
    for it in range(n):
        out, grads, _ = step(ws, x_np, target, size, C, True)
        losses.append(float(out[3]))
        for k in range(10):
            (w, b), (dw, db), (mw, mb) = ws[k], grads[k], bufs[k]
            w, mw = sgd(w, dw.astype(np.float32), mw, lr, momentum, weight_decay, it == 0)
            b, mb = sgd(b, db.astype(np.float32), mb, lr, momentum, weight_decay, it == 0)
            ws[k], bufs[k] = (w, b), (mw, mb)
    return losses
