"""Per-channel power-of-two int8 weights (y355_net_load_layer_i8_pc), restated for the tests independently of yolo355.prep:
the quantizer of folded layers, the widening identity that makes the existing integer restatements (int8_wide_ref.py,
oracle/net_int8_oracle.py) the oracle of the new path, and the synthetic tensors of golden/quant_pc.npz."""
import math

import numpy as np

# (tag, seed, shape, gain): inputs of golden/quant_pc.npz (yolo355.synth.uniform_pm1 scaled per dim-0 slice so that the
# slices' maxima spread over several octaves); 4-D = conv weights, 2-D = a linear layer's, 1-D = biases
QUANT_PC_CASES = [("w4_a", 9101, (8, 3, 3, 3), 0.7), ("w4_b", 9102, (16, 8, 1, 1), 3.0), ("w2", 9103, (6, 10), 0.05),
                  ("b_a", 9104, (16,), 0.1), ("b_b", 9105, (5,), 40.0)]


def quant_pc_input(seed, shape, gain):
    from yolo355 import synth
    t = synth.uniform_pm1(seed, shape).astype(np.float32) * np.float32(gain)
    oct_ = (2.0 ** -((np.arange(shape[0]) * 5) % 7)).astype(np.float32)
    return (t * oct_.reshape((-1,) + (1,) * (len(shape) - 1))).astype(np.float32)


def floor_log2_scale(m):
    """e with 2^e = 2^floor(log2(127 / m)), in the reference's fp32 arithmetic (torch.log2 of an fp32 quotient)"""
    return int(math.floor(float(np.log2(np.float32(127.0) / np.float32(m)))))


def quantize_folded_pc(folded, max_spread=None, per_tensor_fn=None):
    """[(w, b)] -> [{q_w, e_w [cout], q_b, e_b}]: one exponent per output channel, floor(log2(127 / max|w[c]|)); an all-zero
    channel takes the layer's smallest exponent; exponents above min + max_spread are capped (weights rounded at the
    capped exponent).  The bias: one exponent, as the per-tensor recipe (per_tensor_fn(b) -> (q, e))."""
    out = []
    for w, b in folded:
        w = np.asarray(w, np.float32)
        mx = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
        e = np.array([floor_log2_scale(m) if m > 0 else 10 ** 6 for m in mx], np.int64)
        lo = int(e.min())
        e[mx == 0] = lo
        if max_spread is not None:
            e = np.minimum(e, lo + max_spread)
        q = np.rint(w.astype(np.float64) * (2.0 ** e.astype(np.float64)).reshape(-1, 1, 1, 1)).astype(np.int64)
        assert np.abs(q).max() <= 127
        qb, eb = per_tensor_fn(b)
        out.append(dict(q_w=q, e_w=e.astype(np.int32), q_b=qb, e_b=eb))
    return out


def widen(qlayers):
    """per-channel layers -> per-tensor layers of the same function: q_w[c] * 2^(E - e_w[c]) at exponent E = max_c e_w[c]
    (integers wider than int8: the restatements work in int64 and do not mind)"""
    out = []
    for L in qlayers:
        e = np.asarray(L["e_w"], np.int64).reshape(-1)
        if e.size == 1:
            out.append(dict(L, e_w=int(e[0])))
            continue
        E = int(e.max())
        qw = np.asarray(L["q_w"], np.int64) * (np.int64(1) << (E - e)).reshape(-1, 1, 1, 1)
        out.append(dict(q_w=qw, e_w=E, q_b=L["q_b"], e_b=L["e_b"]))
    return out


def spread_channels(folded, k):
    """scale output channel c of every folded layer (weights and bias alike: a BN gamma) by 2^-(c mod k)"""
    out = []
    for w, b in folded:
        s = (2.0 ** -(np.arange(w.shape[0]) % k)).astype(np.float32)
        out.append(((w * s[:, None, None, None]).astype(np.float32), (b * s).astype(np.float32)))
    return out


def max_spread_of(qlayers):
    return max(int(np.max(L["e_w"]) - np.min(L["e_w"])) for L in qlayers)


# SlimYOLOv2 as y355_net runs it in int8 (csrc/net_arch.h kSlimOps): a chain of 3x3 convs, (layer, pooled), LeakyReLU(0.125),
# the last one linear; tensor i is the output of layer i
SLIM_POOL = [1, 1, 0, 1, 0, 1, 0, 0, 0, 0]


def slim_forward_int(x_f32, qlayers, sa_in, sa):
    from oracle import net_int8_oracle as N
    x = np.asarray(x_f32, dtype=np.float32)
    r = np.rint(x * np.float32(2.0 ** sa_in))
    sat = int((np.abs(r) > 127).sum())
    q = np.clip(r, -127, 127).astype(np.int64)
    T, s_in = [], sa_in
    for i, L in enumerate(qlayers):
        q, s = N.conv_layer(q, s_in, L, sa[i], None if i == len(qlayers) - 1 else 0.125, SLIM_POOL[i] == 1)
        sat += s
        T.append(q)
        s_in = sa[i]
    return dict(t=T, sat=sat, sa=list(sa))
