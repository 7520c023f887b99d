"""The detection head and NMS (csrc/head_nms.hip) on adversarial box geometry -- inputs from tests/head_cases.py.

Harness E: Engine.head_nms on crafted int8 maps.  The oracle's greedy NMS (oracle.yolo_oracle.postprocess, tie order
(score desc, anchor index asc)) runs on the GPU's own decoded candidates (Engine.candidates): np.array_equal on boxes,
scores and classes, no tolerance; the decode itself is held to O.head_decode on the dequantised map at the tolerances of
test_nms_edge_list_limits.  Harness H: engine.head_f32 against the fp32 oracle on inputs that satisfy head_cases.h_guards
(asserted before the GPU call): count and classes exact, boxes within 2e-5, scores within 2e-6 (tests/test_ops_wider.py).

Every case asserts on its data that it reaches the path it names (candidate count, suppressing pairs per image -- what
selects the route of resolve_emit_kernel --, chain depth, degenerate counts); test_generators_reach_their_paths makes the
same assertions and the guards on the oracle's decode, without a GPU.
"""
import numpy as np
import pytest

import head_cases as HC


# ------------------------------------------------------------------------------------------------- coverage, on data
def _pairs(box, sc, cl, conf, thr):
    return [HC.suppressing(HC.pair_ious(box[b], sc[b], cl[b], conf), thr) for b in range(box.shape[0])]


def _cover_e1(case, box, sc, cl, tag=""):
    n = [int((sc[b] >= np.float32(case["conf"])).sum()) for b in range(2)]
    assert n == [HC.NMS_CAP, HC.NMS_CAP], n                          # the exact capacity: every anchor a candidate
    npairs = [len(e[0]) for e in _pairs(box, sc, cl, case["conf"], case["thr"])]
    lo, hi = case["band"]
    assert all(lo <= k and (hi is None or k <= hi) for k in npairs), npairs
    print("E1%s C=%d candidates %s suppressing pairs %s route %s" % (tag, case["C"], n, npairs, [HC.route(k) for k in npairs]))
    return npairs


def _cover_e3(case, box, sc, cl, clump):
    out = []
    for b, e in enumerate(_pairs(box, sc, cl, case["conf"], case["thr"])):
        m0 = cl[b][e[0]] == 0
        depth = HC.chain_depth((e[0][m0], e[1][m0]), sc[b])
        cand = sc[b] >= np.float32(case["conf"])
        assert len(np.unique(sc[b][cand & (cl[b] == 0)])) == 1       # the chain's scores are tied: the order is the anchor index
        assert depth >= 200, depth                                   # the suite's other inputs: 17 at most
        if clump:
            assert HC.REG_EDGES + 2000 < len(e[0]) <= HC.LDS_EDGES - 8000, len(e[0])      # the LDS-tail rounds settle the chain
            assert 140 <= int((cand & (cl[b] == 1)).sum()) <= 160
        else:
            assert len(e[0]) < HC.REG_EDGES // 2                     # register rounds, packed per wave after round 3
        out.append((int(cand.sum()), len(e[0]), depth))
    print("E3 clump=%d (candidates, suppressing pairs, chain depth) %s" % (clump, out))
    return out


def _cover_e4(case, box, sc, cl):
    out = []
    for b in range(2):
        cand = sc[b] >= np.float32(case["conf"])
        ar = HC.areas(box[b][cand])
        n0, nlo, nhi = int((ar == 0).sum()), int(((ar > 0) & (ar < 1e-10)).sum()), int(((ar >= 1e-10) & (ar <= 1e-8)).sum())
        assert n0 >= 50 and nlo >= 20 and nhi >= 20, (n0, nlo, nhi)
        assert ar[ar > 0].min() < 1e-11 and int((ar > 1e-4).sum()) >= 100
        z = cand & (HC.areas(box[b]) == 0)
        assert len(np.unique(cl[b][z])) == 1                         # the zero-area boxes share a class ...
        zb = box[b][z]
        assert np.ptp(zb[:, 0]) > 0.5 and np.ptp(zb[:, 1]) > 0.5     # ... and lie all over the image
        out.append((int(cand.sum()), n0, nlo, nhi))
    print("E4 (candidates, zero-area, 0 < area < 1e-10, 1e-10 <= area <= 1e-8) %s" % out)
    return out


def _one_zero_area_survivor(ref):
    """the reference's formula is 0 / 0 on two zero-area boxes: they suppress each other at any distance"""
    assert int((HC.areas(ref[0]) == 0).sum()) == 1


def _cover_e5_wide(box, sc, cl, case):
    assert box.shape[1] == 320
    npairs = [len(e[0]) for e in _pairs(box, sc, cl, case["conf"], case["thr"])]
    assert min(npairs) > 20, npairs
    return npairs


def _cover_h(case, dec, thr, min_pairs=1):
    box, sc, cl = dec[:3]
    n = [int((sc[b] >= np.float32(case["conf"])).sum()) for b in range(2)]
    npairs = [len(e[0]) for e in _pairs(box, sc, cl, case["conf"], thr)]
    assert min(npairs) >= min_pairs, npairs
    return n, npairs


def _cover_h1(case, dec):
    box, sc, cl = dec[:3]
    for b in range(2):
        cand = sc[b] >= np.float32(case["conf"])
        bx = box[b][cand]
        ar = HC.areas(bx)
        assert ar.max() >= 0.5 and 0 < ar.min() < 2.0 ** -16, (ar.max(), ar.min())      # octave 0 down to the clamp at group 15
        w, h = bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]
        asp = w[ar > 0] / h[ar > 0]
        assert asp.max() > 50 and asp.min() < 1 / 50.0, (asp.max(), asp.min())


def _cover_h5(case, dec, want):
    """the degenerate mix on the area octaves: zero-area and near-AREA_MIN boxes share octave group 15 with small ordinary
    ones (its smallest area is 0), the zero-area boxes share a class and lie all over the image, one survives"""
    box, sc, cl = dec[:3]
    out = []
    for b in range(2):
        cand = sc[b] >= np.float32(case["conf"])
        ar = HC.areas(box[b])
        n0, nlo, nhi = int((cand & (ar == 0)).sum()), int((cand & (ar > 0) & (ar < 1e-10)).sum()), int((cand & (ar >= 1e-10) & (ar <= 1e-8)).sum())
        assert n0 >= 50 and nlo >= 20 and nhi >= 20, (n0, nlo, nhi)
        nsmall = int((cand & (ar > 1e-8) & (ar < 2.0 ** -16)).sum())
        assert nsmall >= 10 and int((cand & (ar > 1e-4)).sum()) >= 100
        z = cand & (ar == 0)
        assert len(np.unique(cl[b][z])) == 1
        assert np.ptp(box[b][z][:, 0]) > 0.5 and np.ptp(box[b][z][:, 1]) > 0.5
        zc = int(cl[b][z][0])
        assert int((cand & (cl[b] == zc) & (ar > 1e-4)).sum()) >= 3            # ordinary boxes of the zero-area boxes' class
        for i in np.where(cand & (ar > 0) & (ar <= 1e-8))[0]:                    # each tiny box: alone of its kind in its class,
            same = cand & (cl[b] == cl[b][i]) & (np.arange(len(ar)) != i)       # inside an ordinary box of that class
            assert not (same & (ar <= 1e-8)).any()
            inside = same & (box[b][:, 0] < box[b][i, 0]) & (box[b][:, 1] < box[b][i, 1]) & (box[b][:, 2] > box[b][i, 2]) & (box[b][:, 3] > box[b][i, 3])
            assert inside.any()
        _one_zero_area_survivor(want[b])
        out.append((int(cand.sum()), n0, nlo, nhi, nsmall))
    print("H5 (candidates, zero-area, 0 < area < 1e-10, 1e-10 <= area <= 1e-8, 1e-8 < area < 2^-16) %s" % out)
    return out


def _cover_h4(case, dec):
    n = [int((dec[1][b] >= np.float32(case["conf"])).sum()) for b in range(2)]
    assert n == [case["n_on"]] * 2, n
    assert dec[1].shape[1] == 10647


# ------------------------------------------------------------------------------------------------- CPU: the inputs are what they claim
def test_generators_reach_their_paths():
    """every generator through the oracle alone: coverage assertions of the E cases on the oracle's decode (the GPU tests
    repeat them on the tap), guards and coverage of the H cases"""
    for C in (2, 5):
        for band in ("low", "mid", "high"):
            case = HC.e1_full_capacity(band, C)
            _cover_e1(case, *HC.e_decode(case), tag=" " + band)
    case = HC.e2_dense()
    box, sc, cl = HC.e_decode(case)
    for t in (0.3, 0.5, 0.75):
        v, at, under = HC.boundary_threshold(box[0], sc[0], cl[0], case["conf"], case["C"], t)
        assert abs(float(v) - t) < 0.01 and len(at[1]) == len(under[1]) + 1
    for clump in (0, 1):
        case = HC.e3_chain(clump)
        _cover_e3(case, *HC.e_decode(case), clump)
    case = HC.e4_degenerate()
    box, sc, cl = HC.e_decode(case)
    _cover_e4(case, box, sc, cl)
    for thr in (0.5, 5e-5, 1.0):
        for b in range(2):
            _one_zero_area_survivor(HC.oracle_nms(box[b], sc[b], cl[b], case["conf"], thr, case["C"]))
    for passing in (True, False):
        case = HC.e5_single(passing)
        assert [int(v) for v in (HC.e_decode(case)[1] >= 0.5).sum(axis=1)] == [int(passing)] * 2
    for C in (2, 5):
        case = HC.e5_wide(C)
        print("E5 wide C=%d suppressing pairs %s" % (C, _cover_e5_wide(*HC.e_decode(case), case)))
    case = HC.e5_empty_and_dense()
    n = [int(v) for v in (HC.e_decode(case)[1] >= np.float32(case["conf"])).sum(axis=1)]
    assert n[0] == 0 and n[1] > 600, n
    # ---- H: guards (conditions on the inputs) and coverage
    margins = {}
    for C in (1, 2, 40):
        case = HC.h1_three_levels(C)
        dec = HC.h_decode(case)
        assert dec[0].shape[1] == 1680
        _cover_h1(case, dec)
        for thr in HC.H1_THR:
            g = HC.h_guards(case, thr, dec)
            assert g["ok"], (C, thr, g)
            margins["H1 C=%d thr=%g" % (C, thr)] = (g, _cover_h(case, dec, thr))
    for C in (3, 32, 33):
        case = HC.h2_class_limits(C)
        dec = HC.h_decode(case)
        assert case["preds"][0].shape[2:] == (16, 16) and (C * 16 * 16 > HC.NMS_CAP) == (C >= 17)
        cand = dec[1] >= np.float32(case["conf"])
        assert all(len(np.unique(dec[2][b][cand[b]])) == C for b in range(2))       # every class group is populated
        g = HC.h_guards(case, 0.5, dec)
        assert g["ok"], (C, g)
        margins["H2 C=%d" % C] = (g, _cover_h(case, dec, 0.5, HC.H2_MIN_PAIRS[C]))
    case = HC.h3_non_square()
    dec = HC.h_decode(case)
    assert case["preds"][0].shape[2:] == (40, 8)
    g = HC.h_guards(case, 0.5, dec)
    assert g["ok"], g
    margins["H3"] = (g, _cover_h(case, dec, 0.5))
    case = HC.h4_compaction(4096)
    dec = HC.h_decode(case)
    _cover_h4(case, dec)
    g = HC.h_guards(case, 0.5, dec)
    assert g["ok"], g
    margins["H4"] = (g, _cover_h(case, dec, 0.5))
    over = HC.h4_compaction(4097)
    _cover_h4(over, HC.h_decode(over))
    case = HC.h5_degenerate()
    dec = HC.h_decode(case)
    assert case["C"] > 32                                            # above the class-group limit: area octaves
    for thr in HC.H1_THR:
        g = HC.h_guards(case, thr, dec)
        assert g["ok"], (thr, g)
        _cover_h5(case, dec, HC.h_reference(case, thr, dec))
        margins["H5 thr=%g" % thr] = (g, _cover_h(case, dec, thr, 1500))
    for k, (g, (n, npairs)) in margins.items():
        print("%s guards iou %.3g order %.3g conf %.3g union %.3g cls %.3g; candidates %s suppressing pairs %s"
              % (k, g["iou"], g["order"], g["conf"], g["union"], g["cls"], n, npairs))


# ------------------------------------------------------------------------------------------------- harness E
def _engine(case, **kw):
    from yolo355.engine import Engine
    return Engine(case["size"], case["C"], case["anchors"], conf_thresh=case["conf"], nms_thresh=case["thr"], max_batch=2, **kw)


def _check_decode(case, tap):
    box, sc, cl = HC.e_decode(case)
    assert np.array_equal(tap[2], cl)
    assert np.allclose(tap[0], box, atol=2e-5, rtol=0) and np.allclose(tap[1], sc, atol=2e-6, rtol=1e-5)


def _run_e(eng, case, conf=None, thr=None, max_det=None):
    """head_nms on the case's maps; the oracle's NMS on the tap; exact equality.  Returns (detections, tap, oracle lists)."""
    conf = case["conf"] if conf is None else conf
    thr = case["thr"] if thr is None else thr
    B = case["pq"].shape[0]
    dets = eng.head_nms(case["pq"], case["sa"])
    tap = eng.candidates(B)
    refs = []
    for i in range(B):
        ref = HC.oracle_nms(tap[0][i], tap[1][i], tap[2][i], conf, thr, case["C"])
        refs.append(ref)
        want = [r[:max_det] for r in ref[:3]] if max_det else ref[:3]
        assert len(dets[i][1]) == len(want[1]), (i, thr, len(dets[i][1]), len(want[1]))
        assert np.array_equal(dets[i][0], want[0]) and np.array_equal(dets[i][1], want[1]) and np.array_equal(dets[i][2], want[2]), (i, thr)
    return dets, tap, refs


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("band", ["low", "mid", "high"])
def test_full_capacity(band, C):
    """4096 candidates per image (12-bit edge endpoints, keepn[64], the last hist bin): anchor groups (C = 2: 16 groups x 256
    bins) and class groups (C = 5), with the suppressing pairs in the middle of each route's band"""
    case = HC.e1_full_capacity(band, C)
    eng = _engine(case)
    dets, tap, refs = _run_e(eng, case)
    _check_decode(case, tap)
    _cover_e1(case, *tap, tag=" " + band)
    assert all(0 < len(d[1]) < HC.NMS_CAP for d in dets)
    eng.close()


@pytest.mark.gpu
def test_throughput_mode_pair_walk():
    """Y355_OPT_RING_WORKGROUPS set: one pairs workgroup per image walks all 4096 candidates -- identical outputs.
    The option reaches the head as HeadParams::pairs_wgs = Y355_TPUT_PAIRS_WGS (1) where engine.hip fills head_params
    (`p.pairs_wgs = h->ring_wgs > 0 ? ...`); the engine has no getter for it, so this test covers the one-workgroup walk
    only as long as that mapping stands."""
    from yolo355 import _ffi
    case = HC.e1_full_capacity("mid", 2)
    eng = _engine(case)
    ref, tap, _ = _run_e(eng, case)
    _cover_e1(case, *tap, tag=" mid, one pairs workgroup")
    eng.set_option(_ffi.OPT_RING_WORKGROUPS, 192)
    got, _, _ = _run_e(eng, case)
    for a, b in zip(ref, got):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    eng.close()


@pytest.mark.gpu
def test_thresholds_on_the_iou_values():
    """nms_thresh exactly on a pair's fp32 IoU (`ovr <= thr`: kept) and one ulp below it (suppressed), near 0.3 / 0.5 /
    0.75; the pruned instantiation's lowest threshold 1e-4, the un-pruned one just below it, 1.0 and 0.0"""
    case = HC.e2_dense()
    eng = _engine(case)
    _, tap, _ = _run_e(eng, case)
    _check_decode(case, tap)
    conf, C = case["conf"], case["C"]
    for t in (0.3, 0.5, 0.75):
        v, at, under = HC.boundary_threshold(tap[0][0], tap[1][0], tap[2][0], conf, C, t)
        assert abs(float(v) - t) < 0.01
        assert len(at[1]) == len(under[1]) + 1                       # the boundary decides a box of image 0
        for thr, want in ((v, at), (np.nextafter(v, np.float32(0)), under)):
            eng.set_thresholds(conf, float(thr))
            dets, _, refs = _run_e(eng, case, thr=thr)
            assert len(dets[0][1]) == len(want[1]) and np.array_equal(refs[0][3], want[3])
    seen = {}
    for thr in (np.float32(1e-4), np.nextafter(np.float32(1e-4), np.float32(0)), np.float32(1.0), np.float32(0.0)):
        eng.set_thresholds(conf, float(thr))
        dets, _, _ = _run_e(eng, case, thr=thr)
        seen[float(thr)] = ([len(d[1]) for d in dets], [len(e[0]) for e in _pairs(*tap, conf, thr)])
    print("E2 threshold -> (survivors, suppressing pairs)", seen)
    assert seen[1.0][1] == [0, 0] and min(seen[0.0][1]) > HC.LDS_EDGES        # nothing suppresses / the sorted walk
    assert all(HC.REG_EDGES < k <= HC.LDS_EDGES for k in seen[float(np.float32(1e-4))][1])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("clump", [0, 1])
def test_long_chains(clump):
    """suppression chains of 250 tied boxes, each suppressing its successor only: settled by the packed per-wave rounds
    (clump = 0) and by the rounds with an LDS tail (clump = 1: 11 k more pairs from a clump of a second class)"""
    case = HC.e3_chain(clump)
    eng = _engine(case)
    dets, tap, _ = _run_e(eng, case)
    _check_decode(case, tap)
    stats = _cover_e3(case, *tap, clump)
    for d, (ncand, _, depth) in zip(dets, stats):
        assert abs(len(d[1]) - (ncand - 149 * clump) / 2.0) <= 3       # every other box of a chain survives, one box of the clump
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.5, 5e-5, 1.0])
def test_degenerate_boxes(thr):
    """zero-area boxes (0 / 0 = NaN against each other: one survivor), areas on both sides of AREA_MIN stacked on each other
    and inside ordinary boxes; nms_thresh 0.5, 5e-5 (the un-pruned instantiation) and 1.0 (only NaN pairs suppress)"""
    case = dict(HC.e4_degenerate(), thr=thr)
    eng = _engine(case)
    dets, tap, refs = _run_e(eng, case)
    _check_decode(case, tap)
    _cover_e4(case, *tap)
    for b in range(2):
        _one_zero_area_survivor(refs[b])
    print("E4 thr %g suppressing pairs %s survivors %s" % (thr, [len(e[0]) for e in _pairs(*tap, case["conf"], thr)], [len(d[1]) for d in dets]))
    eng.close()


@pytest.mark.gpu
def test_single_anchor_head():
    """N = 1: the anchor passes, then it does not -- count 0, empty outputs"""
    case = HC.e5_single(True)
    eng = _engine(case)
    dets, tap, _ = _run_e(eng, case)
    _check_decode(case, tap)
    assert [len(d[1]) for d in dets] == [1, 1]
    dets, _, _ = _run_e(eng, HC.e5_single(False))
    assert [len(d[1]) for d in dets] == [0, 0] and all(d[0].shape == (0, 4) for d in dets)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 5])
def test_non_square_grid(C):
    """a 2 x 32 grid of cells and bins, anchor groups and class groups"""
    case = HC.e5_wide(C)
    eng = _engine(case)
    dets, tap, _ = _run_e(eng, case)
    _check_decode(case, tap)
    assert all(10 < len(d[1]) < 320 for d in dets)
    _cover_e5_wide(*tap, case)
    eng.close()


@pytest.mark.gpu
def test_empty_image_beside_a_dense_one():
    case = HC.e5_empty_and_dense()
    eng = _engine(case)
    dets, tap, _ = _run_e(eng, case)
    _check_decode(case, tap)
    n = [int(v) for v in (tap[1] >= np.float32(case["conf"])).sum(axis=1)]
    assert n[0] == 0 and n[1] > 600, n
    assert len(dets[0][1]) == 0 and len(dets[1][1]) > 100
    eng.close()


@pytest.mark.gpu
def test_max_det_cut():
    """max_det = 7: count 7 and the first seven detections of the anchor-ordered list, Engine and head_f32"""
    case = HC.e2_dense()
    eng = _engine(case, max_det=7)
    dets, _, refs = _run_e(eng, case, max_det=7)
    assert all(len(r[1]) > 7 for r in refs) and [len(d[1]) for d in dets] == [7, 7]
    eng.close()
    case = HC.h3_non_square()
    got, want = _run_h(case, 0.5, max_det=7)
    assert all(len(w[1]) > 7 for w in want) and [len(g[1]) for g in got] == [7, 7]


# ------------------------------------------------------------------------------------------------- harness H
def _run_h(case, thr, max_det=None, dec=None):
    """guards first (conditions on the input), then head_f32 against the oracle: count and classes exact, boxes within
    2e-5, scores within 2e-6"""
    from yolo355 import engine as E
    dec = HC.h_decode(case) if dec is None else dec
    g = HC.h_guards(case, thr, dec)
    assert g["ok"], g
    want = HC.h_reference(case, thr, dec)
    nlev, A = len(case["strides"]), case["A"]
    got = E.head_f32(case["preds"], case["strides"], np.asarray(case["anchors"], np.float32).reshape(nlev, A, 2), case["C"], case["size"],
                     1.0, case["conf"], thr, max_det=max_det)
    for b, (g_, w) in enumerate(zip(got, want)):
        w = [r[:max_det] for r in w[:3]] if max_det else w[:3]
        assert len(g_[1]) == len(w[1]), (b, thr, len(g_[1]), len(w[1]))
        assert np.array_equal(g_[2], w[2]), (b, thr)
        assert np.abs(g_[0] - w[0]).max() < 2e-5 and np.abs(g_[1] - w[1]).max() < 2e-6, (b, thr)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 40])
def test_area_groups_three_levels(C):
    """three levels at 128 x 128, areas from octave 0 to below 2^-16, aspect ratios past 50:1, at nms_thresh 0.3 / 0.5 / 0.75;
    C = 40 is above the class-group limit and stays on the area octaves"""
    case = HC.h1_three_levels(C)
    dec = HC.h_decode(case)
    _cover_h1(case, dec)
    for thr in HC.H1_THR:
        _cover_h(case, dec, thr)
        got, want = _run_h(case, thr, dec=dec)
        assert all(len(w[1]) > 50 for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 32, 33])
def test_class_group_limits(C):
    """the class grouping at its limits (3, 32: the bin grid shrinks below 16 x 16) and just past them (33: area groups)"""
    case = HC.h2_class_limits(C)
    dec = HC.h_decode(case)
    cand = dec[1] >= np.float32(case["conf"])
    assert all(len(np.unique(dec[2][b][cand[b]])) == C for b in range(2))
    _cover_h(case, dec, 0.5, HC.H2_MIN_PAIRS[C])
    _run_h(case, 0.5, dec=dec)


@pytest.mark.gpu
def test_non_square_level0():
    """level 0 of 40 x 8 cells: a 16 x 8 bin grid"""
    case = HC.h3_non_square()
    assert case["preds"][0].shape[2:] == (40, 8)
    dec = HC.h_decode(case)
    _cover_h(case, dec, 0.5)
    _run_h(case, 0.5, dec=dec)


@pytest.mark.gpu
def test_compaction_boundary():
    """10 647 anchors: exactly 4096 pass -- the compacted list is full and the head matches the oracle; 4097 -- loud"""
    from yolo355 import engine as E
    from yolo355._ffi import Y355Error
    case = HC.h4_compaction(4096)
    dec = HC.h_decode(case)
    _cover_h4(case, dec)
    _cover_h(case, dec, 0.5)
    _run_h(case, 0.5, dec=dec)
    over = HC.h4_compaction(4097)
    _cover_h4(over, HC.h_decode(over))
    with pytest.raises(Y355Error, match="4096"):
        E.head_f32(over["preds"], over["strides"], np.asarray(over["anchors"], np.float32).reshape(3, 3, 2), over["C"], over["size"], 1.0,
                   over["conf"], 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("thr", HC.H1_THR)
def test_degenerate_boxes_on_area_groups(thr):
    """case E4's mix through head_f32: 60 scattered zero-area boxes of one class (NaN against each other: one survives), 22
    lone boxes on each side of AREA_MIN inside ordinary boxes of their class, small and ordinary boxes -- the degenerate ones
    all in octave group 15.  (nms_thresh 5e-5 cannot satisfy the IoU-margin guard: disjoint pairs are 5e-5 from it.)"""
    case = HC.h5_degenerate()
    dec = HC.h_decode(case)
    _cover_h5(case, dec, HC.h_reference(case, thr, dec))
    _cover_h(case, dec, thr, 1500)
    _run_h(case, thr, dec=dec)
