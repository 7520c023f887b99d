"""Every bf16 tile of the generic implicit-GEMM convolution (csrc/convg.hip) that conv2d_bf16 can select, with its weights packed
by the one B-fragment packer (y355_pack_bfrags, csrc/convg_shared.h), on the smallest shapes at which these can go wrong: a row and a column past the tile, a partial block of output channels, one and
three input chunks (both LDS slabs and the last-chunk path of the 8-wave kernel), 3x3 and 1x1, the thin layout (two taps per
k-step), stride 2 once.  Every case is bf16, so of ConvGInst's variant ladder only the plain instantiation runs here; the
NARROW / PC / STAT branches are run by the int8 Net tests: test_int8_wide_models and test_int8_per_channel (NARROW, PC and the
64-bit epilogue on the tiles of 224-sized DarkNets with max_batch 2: 0, 1, 2, 3, 4, 6, 7, 9, 10, never 5), test_net_calibration
(STAT, and the plain variants on every layer, on tiles 0, 1, 2, 3, 7, 8, 9), test_int8_production_tiles (all of them on the tiles of a
416 x 416 net with max_batch 64: 0, 1, 2, 3, 4, 5, 6, 9, 10, with partial tiles; tests/int8_tile_cases.py restates the selection).

bf16: small-integer operands -- every product and every partial sum is an integer below 2^24, so the fp32 accumulation is
exact in any order and the result must EQUAL the float64 convolution (the method of test_bf16_route_is_exact_on_small_integers);
with a bf16 result and a residual, too, while |y| < 256 (integers that bf16 holds; halves below 128)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# (tag, tile the shape selects (y355_convg_select), cin, cout, ksize, stride, H, W), batch 2
BF16_CASES = [
    ("thin_13x26", 1, 16, 80, 3, 1, 14, 27),            # 32-byte pixels: a k-step holds two taps; 4 waves
    ("c64_13x26_1chunk", 2, 32, 24, 3, 1, 14, 27),      # 8 waves, one chunk: one LDS slab
    ("c64_13x26_3chunks", 2, 96, 80, 3, 1, 14, 27),     # three chunks: both slabs, the last-chunk path
    ("c64_13x26_1x1", 2, 96, 80, 1, 1, 14, 27),
    ("c128_13x26_1chunk", 4, 64, 80, 3, 1, 14, 27),
    ("c128_13x26_3chunks", 4, 192, 80, 1, 1, 14, 27),
    ("c256_13x13_wide_1chunk", 5, 128, 144, 3, 1, 14, 27),    # 256 output channels per workgroup: 144 is a partial block
    ("c256_13x13_wide_3chunks", 5, 384, 144, 1, 1, 14, 27),
    ("c256_13x13_few_1chunk", 6, 128, 24, 1, 1, 14, 27),      # 4 waves, 256-byte chunks
    ("c256_13x13_few_3chunks", 6, 384, 24, 3, 1, 14, 27),
    ("small_1chunk", 7, 32, 80, 3, 1, 9, 17),
    ("small_3chunks", 7, 96, 80, 1, 1, 9, 17),
    ("stride2", 9, 96, 80, 3, 2, 18, 35),               # 9x18 outputs: a row and two columns past the 8x16 tile
]
B = 2


@functools.lru_cache(maxsize=None)
def _bf16_case(tag):
    """operands and float64 references of one case, computed once: (x, w, b, want, x1, w1, res, want_res)"""
    _, _, cin, cout, k, s, H, W = next(c for c in BF16_CASES if c[0] == tag)
    rng = np.random.default_rng(sum(map(ord, tag)))
    x = rng.integers(-4, 5, size=(B, cin, H, W)).astype(np.float32)
    w = rng.integers(-2, 3, size=(cout, cin, k, k)).astype(np.float32)
    b = rng.integers(-8, 9, size=(cout,)).astype(np.float32)

    def ref(xx, ww):
        y = F.conv2d(torch.from_numpy(xx).double(), torch.from_numpy(ww).double(), torch.from_numpy(b).double(), stride=s, padding=k // 2)
        return y.numpy()
    want = ref(x, w)
    # the bf16 result: sparse operands in {-1, 0, 1}, so that conv + bias + residual stays an integer below 256
    x1 = (rng.integers(-1, 2, size=x.shape) * (rng.random(x.shape) < 0.25)).astype(np.float32)
    w1 = (rng.integers(-1, 2, size=w.shape) * (rng.random(w.shape) < 0.25)).astype(np.float32)
    y1 = ref(x1, w1)
    res = rng.integers(-16, 17, size=y1.shape).astype(np.float32)
    for a in (x, w, b, want, x1, w1, res, y1):
        a.setflags(write=False)
    return x, w, b, want, x1, w1, res, y1


@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16_references_are_exact_integers_in_range(case):
    """the precondition of the GPU test, on the CPU: every reference value is a finite integer, |sum| < 2^24 whatever the order
    of accumulation (bounded by sum |x| |w|), and the bf16-result variant stays below 256"""
    tag, _, cin, cout, k, s, H, W = case
    x, w, b, want, x1, w1, res, y1 = _bf16_case(tag)
    assert np.isfinite(want).all() and np.array_equal(want, np.rint(want))
    assert 4 * 2 * cin * k * k + 8 < 2 ** 24                   # worst case of any partial sum
    assert np.abs(want).max() < 2 ** 24
    assert np.isfinite(y1).all() and np.abs(y1 + res).max() < 256          # integers: eight bits
    assert np.abs(np.where(y1 >= 0, y1, y1 * 0.5) + res).max() < 128          # halves: bf16 holds them below 128
    assert np.array_equal(y1, np.rint(y1))


def test_bf16_cases_select_the_tiles_they_name():
    """y355_convg_select's rules restated for conv2d_bf16's layouts (csrc/convg.hip, csrc/ops.hip): every case reaches the tile it is
    there for, and together they reach every bf16 tile the operator can select.  The selector has no Python binding, so this is
    a restatement and not a query: if the C rules change, it has to be changed with them, or the GPU cases stop reaching the
    tiles they name without a failure here"""
    def select(in_pb, cout, H, W, stride):
        if stride == 2:
            return 9
        if in_pb == 32:
            return 1
        if H < 13 or W < 13:
            return 7
        if cout <= 64:
            return 6 if in_pb % 256 == 0 else 2
        if cout <= 128:
            return 4 if in_pb % 128 == 0 else 2
        return 5 if in_pb % 256 == 0 else (4 if in_pb % 128 == 0 else 2)
    for tag, kid, cin, cout, k, s, H, W in BF16_CASES:
        thin = cin <= 16 and k == 3 and s == 1
        in_pb = 2 * (16 if thin else (cin + 31) // 32 * 32)
        assert select(in_pb, cout, H, W, s) == kid, tag
    assert {c[1] for c in BF16_CASES} == {1, 2, 4, 5, 6, 7, 9}


@pytest.mark.gpu
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16_tiles_are_exact_on_small_integers(case):
    from yolo355 import engine as E
    tag, _, cin, cout, k, s, H, W = case
    x, w, b, want, x1, w1, res, y1 = _bf16_case(tag)
    got = E.conv2d_bf16(x, w, b, stride=s, out_fp32=True)
    assert np.array_equal(got, want.astype(np.float32)), (tag, float(np.abs(got - want).max()))
    got = E.conv2d_bf16(x, w, b, stride=s, neg_slope=0.5, out_fp32=True)
    assert np.array_equal(got, np.where(want >= 0, want, want * 0.5).astype(np.float32)), tag
    # bf16 result with the bf16 residual, with and without a slope
    got = E.conv2d_bf16(x1, w1, b, residual=res, stride=s)
    assert np.array_equal(got, (y1 + res).astype(np.float32)), tag
    got = E.conv2d_bf16(x1, w1, b, residual=res, stride=s, neg_slope=0.5)
    assert np.array_equal(got, (np.where(y1 >= 0, y1, y1 * 0.5) + res).astype(np.float32)), tag
