"""CPU: the per-element bf16 checker of tests/bf16_layer_ref.py proved before it judges a kernel.

An emulation of the bf16 path (torch float32 convolutions on the bf16-rounded operands, the contract's rounding points, RNE to
bf16, outputs chained as inputs) must pass everywhere: the derived bound is not tighter than a legitimate fp32 accumulation in
another order.  Ten mutations of one op's emulated output must each be reported, with a reported element among the mutated ones.
rb and every part of the bound are pinned by hand-worked values."""
import numpy as np
import pytest
import torch

import bf16_layer_ref as L

torch.set_num_threads(min(16, torch.get_num_threads()))
_EMU = {}
CPU_B = {"yolo_v2": 1, "yolo_v3": 1}          # time: the float64 convolutions of the two at B = 2 alone take 13 s on 8 cores


def _emu(arch):
    """(graph, x, weights, emulated tensors) of the smallest case of a graph, computed once and left unchanged"""
    if arch not in _EMU:
        tag, _, size, B = next(c for c in L.CASES if c[0] == L.SMALLEST[arch])
        B = min(B, CPU_B.get(arch, B))
        m = L.model_of(arch)
        x = L.images_of(arch, size, B)
        T = L.emulate(arch, x, m["weights"], m["predc"])
        for t in T:
            t.setflags(write=False)
        _EMU[arch] = (L.GRAPHS[arch](), x, m["weights"], T)
    return _EMU[arch]


# ---------------------------------------------------------------------------------------------------- rb and the bound
def test_rb_hand_values():
    f = lambda v: float(L.rb(torch.tensor([v], dtype=torch.float64))[0])
    assert f(1.0) == 1.0 and f(-0.0) == 0.0 and f(3.140625) == 3.140625
    assert f(1.0 + 2.0 ** -8) == 1.0                    # tie between 1 and 1 + 2^-7: to the even mantissa
    assert f(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6    # tie between 1 + 2^-7 (odd) and 1 + 2^-6 (even)
    assert f(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0 + 2.0 ** -7        # just above the tie: up (a float32 round trip would lose the 2^-40)
    assert f(-(1.0 + 2.0 ** -8)) == -1.0 and f(-(1.0 + 3 * 2.0 ** -8)) == -(1.0 + 2.0 ** -6)
    assert f(2.0 - 2.0 ** -9) == 2.0                    # the carry runs into the exponent
    assert f(0.1) == 0.10009765625 and f(0.3) == 0.30078125
    assert f(2.0 ** -126) == 2.0 ** -126 and f(2.0 ** -134) == 0.0 and f(3 * 2.0 ** -134) == 2.0 ** -132      # subnormal grid 2^-133, ties to even
    assert f(float.fromhex("0x1.fep127")) == float.fromhex("0x1.fep127") and f(float.fromhex("0x1.ffp127")) == float("inf")
    # against the float32 bit trick of csrc/y355_common.h (y355_bf16_rne) on float32 values
    v = np.random.default_rng(0).normal(0, 3, 4000).astype(np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    want = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    assert np.array_equal(L.rb(v).numpy(), want.astype(np.float64))
    assert float(L.trunc_bf16(torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -30], dtype=torch.float64))[0]) == 1.0
    lo, hi = L.bf16_cell(torch.tensor([1.0, 1.5, -2.0, 0.0], dtype=torch.float64))
    assert lo.tolist() == [1.0 - 2.0 ** -9, 1.5 - 2.0 ** -8, -2.0 - 2.0 ** -7, -2.0 ** -134]
    assert hi.tolist() == [1.0 + 2.0 ** -8, 1.5 + 2.0 ** -8, -2.0 + 2.0 ** -8, 2.0 ** -134]
    assert L.bf16_next(torch.tensor([1.0, -1.0])).tolist() == [1.0 + 2.0 ** -7, -1.0 + 2.0 ** -8]


def test_bound_parts_hand_values():
    """one 1x1 conv, cin 2: X = (1, -2), Wb = (0.5, 0.25), b = -0.125 -> a = -0.125, S = 1 + 0.125 = 1.125, K = 3"""
    o = dict(op="conv", i=0, o=1, choff=0, layer=0, cin=2, cout=1, k=1, act=L.L100, pool=0, s2=0, res=-1)
    X = torch.tensor([1.0, -2.0], dtype=torch.float64).view(1, 2, 1, 1)
    w = np.array([0.5, 0.25], np.float32).reshape(1, 2, 1, 1)
    b = np.array([-0.125], np.float32)
    s = float(np.float32(0.1))
    assert s != 0.1
    z, zc, S, e = L.conv_terms(o, X, w, b)
    assert float(z) == -0.125 * s and float(zc) == float(z)
    assert float(S) == pytest.approx(1.125 * 1.001, rel=1e-7)
    assert float(e) == pytest.approx(2 * 3 * 2.0 ** -24 * 1.125 * 1.001 * 1.001 + 2.0 ** -24 * 0.125 * s, rel=1e-7)
    # the residual enters after the activation and adds its own rounding term
    z2, zc2, S2, e2 = L.conv_terms(o, X, w, b, res=torch.full((1, 1, 1, 1), 3.0, dtype=torch.float64))
    assert float(z2) == 3.0 - 0.125 * s and float(zc2) == float(zc) and float(S2) == float(S)
    assert float(e2) == pytest.approx(float(e) + 2.0 ** -24 * (3.0 - 0.125 * s), rel=1e-12)
    # the weight is rounded to bf16 (0.3 -> 0.30078125), the bias is not (0.3f stays)
    z3, _, S3, _ = L.conv_terms(dict(o, act=L.NONE), X, np.array([0.3, 0.0], np.float32).reshape(1, 2, 1, 1), np.array([0.3], np.float32))
    assert float(z3) == 0.30078125 + float(np.float32(0.3))
    # interval: z = 1 + 2^-8 is a tie; e reaches both neighbours, nothing further.  rho: the distance to got's cell over u S
    one = lambda v: torch.tensor([v], dtype=torch.float64).view(1, 1, 1, 1)
    z, e, S = one(1.0 + 2.0 ** -8), one(2.0 ** -20), one(4.0)
    for got, bad, rho in [(1.0, 0, 0.0), (1.0 + 2.0 ** -7, 0, 0.0), (1.0 + 2.0 ** -6, 1, 2.0 ** -7 / (4 * 2.0 ** -24)),
                          (1.0 - 2.0 ** -8, 1, (2.0 ** -8 + 2.0 ** -9) / (4 * 2.0 ** -24))]:
        st = L.interval_stats(one(got), z, e, S)
        assert st["bad"] == bad and st["rho_max"] == pytest.approx(rho, rel=1e-12), got
    # with a pool both sides take the maximum over the window
    zp = torch.tensor([[0.25, 1.0], [-3.0, 0.5]], dtype=torch.float64).view(1, 1, 2, 2)
    st = L.interval_stats(one(1.0), zp, torch.full_like(zp, 1e-6), torch.ones_like(zp), pool=1)
    assert st["bad"] == 0 and st["exact"] == 1.0 and L.interval_stats(one(0.5), zp, torch.full_like(zp, 1e-6), torch.ones_like(zp), pool=1)["bad"] == 1
    # fp32 output: |got - z| <= e
    assert L.interval_stats(one(1.0 + 2.0 ** -21), one(1.0), e, S, fp32_out=True)["bad"] == 0
    assert L.interval_stats(one(1.0 + 2.0 ** -19), one(1.0), e, S, fp32_out=True)["bad"] == 1
    # bilinear x2 of a 2 x 2 map: c = 6 + 4 (2 + 2 - 2) = 14; the pixel (1, 2) lies at (1/3, 2/3)
    Xu = torch.tensor([[1.0, 2.0], [4.0, -8.0]], dtype=torch.float64).view(1, 1, 2, 2)
    zu, eu, Mu = L.upsample_terms(Xu)
    assert float(zu[0, 0, 1, 2]) == pytest.approx((2 / 3) * ((1 / 3) * 1 + (2 / 3) * 2) + (1 / 3) * ((1 / 3) * 4 + (2 / 3) * -8), rel=1e-14)
    assert float(zu[0, 0, 3, 3]) == -8.0 and float(zu[0, 0, 0, 0]) == 1.0
    assert float(eu[0, 0, 1, 2]) == pytest.approx(14 * 2.0 ** -24 * 8.0 * 1.001, rel=1e-12)


# ---------------------------------------------------------------------------------------------------- the emulation passes
@pytest.mark.parametrize("arch", L.ARCHS)
def test_emulation_passes_everywhere(arch):
    g, x, weights, T = _emu(arch)
    reports = L.check_graph(arch, x, weights, T)
    assert len(reports) == len(g.ops)
    assert not L.describe(reports), L.describe(reports)
    worst = max(r["rho_max"] for r in reports if r["kind"] == "conv")
    print("%s: %d ops, largest rho of the emulation %.1f" % (arch, len(reports), worst))
    if arch in ("slim_yolo_v2", "tiny_yolo_v3"):             # the two-layer check of the fused front end accepts the layer launches' map
        st = L.check_front(arch, x, weights, T[1])
        assert st["bad"] == 0, st


# ---------------------------------------------------------------------------------------------------- mutations
def _mutated(arch, idx, y, also=()):
    """reports (with masks) of op idx, and of the ops in `also`, after its own channels are replaced by y"""
    g, x, weights, T = _emu(arch)
    o = g.ops[idx]
    Tm = list(T)
    Tm[o["o"]] = T[o["o"]].copy()
    L.place(g, idx, Tm, y)
    return [L.check_op(g, i, x, weights, Tm, want_mask=True) for i in (idx,) + tuple(also)], Tm


def _own(g, idx, T):
    o = g.ops[idx]
    off = o.get("choff", 0)
    n = o["cout"] if o["op"] == "conv" and o["cout"] else T[o["o"]].shape[1] - off
    return T[o["o"]][:, off:off + n]


def _assert_caught(arch, idx, y):
    g, x, weights, T = _emu(arch)
    changed = y != _own(g, idx, T)[:, :y.shape[1]]
    assert changed.any(), "the mutation changed nothing"
    (st,), _ = _mutated(arch, idx, y)
    assert st["bad"] > 0 and (st["mask"] & changed).any(), (L.op_name(g, idx), st["bad"], int(changed.sum()))
    assert not (st["mask"] & ~changed).any(), "an element the mutation left alone was reported"
    return st


def _find(g, pred):
    return next(i for i, o in enumerate(g.ops) if pred(o))


def test_mutation_1_tap_removed_in_the_last_column():
    for arch, pred in [("slim_yolo_v2", lambda o: o["i"] == 1), ("yolo_v3", lambda o: o["op"] == "conv" and o["k"] == 3 and o["res"] >= 0)]:
        g, x, weights, T = _emu(arch)
        idx = _find(g, pred)

        def drop(w):
            w[:, :, 1, 0] = 0
            return w
        y = _own(g, idx, T).copy()
        y[..., -1] = L.emulate_op(g, idx, x, weights, T, wmod=drop)[..., -1]
        _assert_caught(arch, idx, y)


def test_mutation_2_bias_of_one_channel_omitted():
    for arch, pred in [("tiny_yolo_v3", lambda o: o["i"] == 2), ("yolo_v2", lambda o: o["op"] == "conv" and o["k"] == 1)]:
        g, x, weights, T = _emu(arch)
        idx = _find(g, pred)

        ch = int(np.abs(weights[g.ops[idx]["layer"]][1]).argmax())

        def nob(b):
            b[ch] = 0
            return b
        y = _own(g, idx, T).copy()
        y[:, ch] = L.emulate_op(g, idx, x, weights, T, bmod=nob)[:, ch]
        st = _assert_caught(arch, idx, y)
        assert all(c[1] == ch for c in st["first"])


def test_mutation_3_the_other_slope():
    for arch, act, other in [("yolo_v2", L.L100, 0.125), ("yolo_v2", L.L125, 0.1), ("slim_yolo_v2", L.L125, 0.1), ("yolo_v3", L.L100, 0.125)]:
        g, x, weights, T = _emu(arch)
        idx = [i for i, o in enumerate(g.ops) if o["op"] == "conv" and o["act"] == act][-1]        # a late layer of that slope
        _assert_caught(arch, idx, L.emulate_op(g, idx, x, weights, T, slope=other))


def test_mutation_4_residual_from_the_pixel_to_the_left():
    for arch in ("yolo_v3", "yolo_v3_spp"):
        g, x, weights, T = _emu(arch)
        idx = [i for i, o in enumerate(g.ops) if o["op"] == "conv" and o["res"] >= 0][3]
        full = L.emulate_op(g, idx, x, weights, T, res_shift=1)
        _assert_caught(arch, idx, full)
        y = _own(g, idx, T).copy()                          # ... and in the last column alone
        y[..., -1] = full[..., -1]
        _assert_caught(arch, idx, y)


def test_mutation_5_two_64_channel_blocks_swapped():
    for arch in ("slim_yolo_v2", "yolo_v3_spp"):
        g, x, weights, T = _emu(arch)
        idx = _find(g, lambda o: o["op"] == "conv" and (o["cout"] or 0) >= 128)
        y = _own(g, idx, T).copy()
        y[:, :64], y[:, 64:128] = _own(g, idx, T)[:, 64:128], _own(g, idx, T)[:, :64]
        _assert_caught(arch, idx, y)


def test_mutation_6_pool_window_shifted_by_one():
    for arch, pred in [("yolo_v2", lambda o: o["op"] == "pool"), ("tiny_yolo_v3", lambda o: o["op"] == "pool" and o.get("s1")),
                       ("slim_yolo_v2", lambda o: o["op"] == "conv" and o["pool"] and o["i"] >= 0)]:
        g, x, weights, T = _emu(arch)
        idx = _find(g, pred)
        _assert_caught(arch, idx, L.emulate_op(g, idx, x, weights, T, pool_shift=1))


def test_mutation_7_truncation_instead_of_rne():
    for arch, pred in [("slim_yolo_v2", lambda o: o["i"] == -1), ("slim_yolo_v2", lambda o: o["i"] == 4),
                       ("yolo_v3", lambda o: o["op"] == "conv" and o["res"] >= 0)]:
        g, x, weights, T = _emu(arch)
        idx = _find(g, pred)
        st = _assert_caught(arch, idx, L.emulate_op(g, idx, x, weights, T, trunc=True))
        print("%s: %.1f %% of the truncated elements reported" % (L.op_name(g, idx), 100.0 * st["bad"] / st["n"]))
        if g.ops[idx]["i"] == -1:                           # K = 28: the interval is a small part of a bf16 step, and about
            assert st["bad"] > 0.3 * st["n"]                # half of all values round up


def test_mutation_8_one_element_one_step_beyond_its_interval():
    for arch, pred in [("tiny_yolo_v3", lambda o: o["i"] == 3), ("yolo_v2", lambda o: o["op"] == "conv" and o["choff"] == 256)]:
        g, x, weights, T = _emu(arch)
        idx = _find(g, pred)
        o = g.ops[idx]
        z, zc, S, e = L.conv_terms(o, L.t64(T[o["i"]])[:, :o["cin"]], *weights[o["layer"]])
        for up in (True, False):
            at = (z.shape[0] - 1, z.shape[1] - 1, z.shape[2] - 1, 0) if up else (0, 3, 1, z.shape[3] - 1)
            edge = L.rb((z + e)[at]) if up else L.rb((z - e)[at])
            y = _own(g, idx, T).copy()
            y[at] = float(L.bf16_next(edge.view(1), up)[0])
            st = _assert_caught(arch, idx, y)
            assert st["bad"] == 1 and st["first"] == [at]


def test_mutation_9_concat_range_at_the_wrong_channel_offset():
    for arch in ("tiny_yolo_v3", "yolo_v3"):
        g, x, weights, T = _emu(arch)
        idx = _find(g, lambda o: o["op"] == "up")
        o = g.ops[idx]
        owner = _find(g, lambda p: p["op"] == "conv" and p["o"] == o["o"])       # the conv that owns [0, choff)
        Tm = list(T)
        Tm[o["o"]] = T[o["o"]].copy()
        up = L.emulate_op(g, idx, x, weights, T)
        Tm[o["o"]][:, o["choff"]:] = 0                        # its own range was never written ...
        Tm[o["o"]][:, o["choff"] - 64:o["choff"] - 64 + up.shape[1]] = up       # ... the data went 64 channels lower
        a = L.check_op(g, idx, x, weights, Tm, want_mask=True)
        b = L.check_op(g, owner, x, weights, Tm, want_mask=True)
        assert a["bad"] > 0 and b["bad"] > 0
        assert b["mask"][:, -64:].any() and not b["mask"][:, :-64].any()        # the owner reports exactly the overwritten channels
        assert "op %d" % owner in L.describe([dict(b, family="RING")]) and "RING" in L.describe([dict(b, family="RING")])
    # a padding channel that is not zero is reported too (DarkNet-53's first map: 32 real channels of 64)
    g, x, weights, T = _emu("yolo_v3")
    Tm = list(T)
    Tm[1] = T[1].copy()
    Tm[1][0, 40, 3, 3] = 2.0 ** -20
    assert L.check_op(g, 1, x, weights, Tm)["pad_bad"] == 1 and L.check_op(g, 1, x, weights, T)["pad_bad"] == 0


def test_mutation_10_upsample_without_align_corners():
    for arch in ("tiny_yolo_v3", "yolo_v3_spp"):
        g, x, weights, T = _emu(arch)
        idx = _find(g, lambda o: o["op"] == "up")
        _assert_caught(arch, idx, L.emulate_op(g, idx, x, weights, T, up_align=False))


def test_fused_front_check_catches_a_wrong_intermediate():
    """the two-layer check: conv1's map truncated instead of rounded in front of conv2 is outside the grown bound"""
    g, x, weights, T = _emu("slim_yolo_v2")
    T0 = L.trunc_bf16(torch.from_numpy(L.emulate_op(g, 0, x, weights, T, trunc=True))).float().numpy()
    Tm = [T0] + list(T[1:])
    y = L.emulate_op(g, 1, x, weights, Tm)
    st = L.check_front("slim_yolo_v2", x, weights, y)
    assert st["bad"] > 0 and 0 < st["ambiguous"] < 0.1
