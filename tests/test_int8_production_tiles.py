"""The int8 form of the five y355_net graphs on the tiles a deployed net takes (416 x 416, max_batch 64): calibration steps and
forwards bit for bit against the integer restatements (tests/net_calib_ref.py), on the cases of tests/int8_tile_cases.py.

The other int8 modules (test_int8_wide_models, test_int8_per_channel, test_net_calibration, test_fp32_models) run on handles with
max_batch 1 or 2 and mostly on maps smaller than 13 x 13, where y355_convg_select picks other tiles: no calibration step had
run the STAT instantiations of tiles 4, 5, 6 and 10 (nor the plain variants of those tiles on every layer, as the write pass does),
no int8 DarkNet convolution on tile 5 had been compared with anything, and no int8 net had run with Y355_NET_OPT_WORKGROUPS.

CPU: the restatement of the selectors reaches, over the case table, everything the five graphs select at 416 x 416 with
max_batch 64; it reproduces the tiles of test_net_calibration's sizes.
GPU, per case (run_case, once; the comparisons happen there and the tests assert their findings):
  calibration   two steps on one handle (freeze, then not, other images): exponents, trackers, maxima bit for bit, and every
                tensor the pass wrote;
  forward       on the calibrated exponents: a tap forward (every tensor, the clamp count, candidates, detections, routes), a
                plain forward and a plain forward with Y355_NET_OPT_WORKGROUPS = 7 (the same bytes, counters, detections, routes);
  wide          v3_448_mb64 only (run_wide: a second handle of the same configuration under the calibrated exponents, one image):
                a stride-32 residual 3x3 layer, a stride-32 3x3 512 -> 1024 and a stride-32 1x1 reloaded with the same integers
                at lower weight exponents until they need the 64-bit epilogue, once uniformly and once by c mod 17; then the
                residual layer a few bits coarser, so that the 32-bit residual epilogue runs on tile 5 as well (as loaded, every
                residual layer of the deeper levels needs 64 bits under these weights).
No comparison is restricted to a subset of tensors or elements, except the unwritten tensor 0 behind a fused front end.
Measured on an MI355X (16 CPUs for the references), the GPU tests of this module alone: 49.8 s wall for 32 tests.  The first test
of a case carries all its runs and references: 11.8 s for v3_448_mb64 and 10.8 s for v3_416_mb2 (DarkNet-53, B = 2: two steps, three
forwards, five reads of every tensor), 6.7 s for v3_448_mb64_pc, 3.4 to 4.2 s for the other DarkNet rows and the wide-epilogue
test, under 1.5 s for tiny and slim; the references and the tensor reads dominate, not GPU work.  Every handle with max_batch 64
was created as such (the fall-back to the equivalent max_batch 48 was not needed).
The head: the synthetic weights put the scores of all anchors (up to 11 466) in one narrow band, so the confidence threshold of a
case is taken from the restatement's scores (_pick_conf), at most 300 candidates per image.
"""
import traceback

import numpy as np
import pytest
import torch

import int8_pc_ref as P
import int8_tile_cases as T
import int8_wide_ref as W
import net_calib_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))

SMALL = ("slim_yolo_v2", "tiny_yolo_v3")
_RUNS = {}


# ---------------------------------------------------------------------------------------------------- CPU
def _union(fn):
    out = set()
    for tag in T.TAGS:
        out |= fn(T.predict_case(tag))
    return out


def test_case_table_reaches_what_a_deployed_net_selects():
    """computed from predict() and the table, not typed in: the (tile, residual) pairs of the statistics pass and the (family,
    tile or ring, residual) triples of the forward that the five graphs select at 416 x 416 with max_batch 64, classes 2 and 20"""
    stat, fwd = _union(T.stat_set), _union(T.forward_set)
    for tag in T.TAGS:
        p = T.predict_case(tag)
        print(tag, "stat", sorted(T.stat_set(p)), "forward", sorted(T.forward_set(p), key=str))
    print("required stat   ", sorted(T.required("stat")))
    print("required forward", sorted(T.required("forward"), key=str))
    print("reached stat    ", sorted(stat))
    print("reached forward ", sorted(fwd, key=str))
    assert T.required("stat") <= stat, sorted(T.required("stat") - stat)
    assert T.required("forward") <= fwd, sorted(T.required("forward") - fwd, key=str)
    # the drop-in's handle (max_batch 2): tile 10 where the deployed net takes tile 5, with and without the residual
    mb2 = set()
    for tag in T.TAGS:
        if T.case(tag)[4] == 2:
            mb2 |= T.stat_set(T.predict_case(tag))
    assert {(10, False), (10, True)} <= mb2, sorted(mb2)
    # what the deployed nets take in the statistics pass, as the issue behind this module states it
    assert {t for t, _ in T.required("stat")} == {0, 1, 2, 3, 4, 5, 6, 9, 10}
    assert {t for t, r in T.required("stat") if r} == {1, 2, 4, 5}


def test_deployed_darknet53_takes_tile_5_and_tile_4_as_counted():
    """DarkNet-53 at 416 x 416, max_batch 64, 20 classes: tile 5 for 29 layers, 12 of them with the residual sum, tile 4 for 26,
    8 of them with the residual (the counts of the issue behind this module: the restatement there and this one agree); these
    8-wave tiles read more than one chunk there, which the STAT pipeline of convg8_kernel treats differently"""
    p = T.predict("yolo_v3", [416, 416], 64, T.predc_of("yolo_v3", 20))
    n = lambda tile, res: sum(1 for e in p if e["stat"] == tile and (e["residual"] or not res))
    assert (n(5, False), n(5, True), n(4, False), n(4, True)) == (29, 12, 26, 8)
    for tile in (4, 5, 10):
        assert max(e["chunks"] for e in p if e["stat"] == tile) > 1, tile


def test_sizes_of_the_calibration_tests_stay_off_the_production_tiles():
    """the claim this module rests on: every GPU calibration test so far (test_net_calibration.SIZE, max_batch 2) reaches no tile
    outside {0, 1, 2, 3, 7, 8, 9}.  If this fails the restatement is wrong (or those tests have changed)"""
    import test_net_calibration as C
    seen = set()
    for arch, size in C.SIZE.items():
        seen |= {e["stat"] for e in T.predict(arch, size, 2, C._predc(arch)) if e["stat"] is not None}
    assert seen <= {0, 1, 2, 3, 7, 8, 9}, sorted(seen)


def test_equivalent_max_batch_is_48():
    """the smallest max_batch for which every layer of the two DarkNet-53 rows takes the tiles it takes at 64"""
    for tag in ("v3_448_mb64", "spp_416_mb64"):
        assert _equivalent_max_batch(tag) <= 48
    assert _equivalent_max_batch("spp_416_mb64") == 48


def _equivalent_max_batch(tag):
    _, arch, size, classes, mb, _, _ = T.case(tag)
    want = [(e["stat"], e["family"], e["tile"]) for e in T.predict_case(tag)]
    return min(m for m in range(1, mb + 1)
               if [(e["stat"], e["family"], e["tile"]) for e in T.predict(arch, size, m, T.predc_of(arch, classes))] == want)


# ---------------------------------------------------------------------------------------------------- GPU
def _bytes(net, t, B, sa):
    """tensor t as the integers the kernels wrote: get_tensor's value times 2^sa[t], sa the exponents get_tensor divides by"""
    return np.rint(net.get_tensor(t, B) * np.float32(2.0 ** sa[t])).astype(np.int16)


def _load(net, i, q):
    net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])


def _ref_layers(ql):
    """the layers as the restatements take them: per-channel ones widened (int8_pc_ref.widen), int64"""
    return [dict(q_w=np.asarray(q["q_w"], np.int64), q_b=np.asarray(q["q_b"], np.int64), e_w=int(q["e_w"]), e_b=int(q["e_b"]))
            for q in P.widen(ql)]


def _decode(arch, ref, x, qref, size, classes):
    """(boxes [B, N, 4], class scores [B, N, C]) of the restatement's prediction maps, by the decoders the existing int8 tests use"""
    from oracle import fp32_oracle as FP
    from oracle import net_int8_oracle as N
    from oracle import yolo_oracle as O
    anchors = T.anchors_of(arch)
    if arch == "tiny_yolo_v3":
        r = N.tiny_detect(x, qref, ref["sa_in"], ref["sa"], size, anchors, classes, conf_thresh=0.99)
        for t in range(len(r["t"])):                                    # oracle/net_int8_oracle.py and net_calib_ref agree
            assert np.array_equal(r["t"][t], ref["t"][t][:, :r["t"][t].shape[1]]), t
        return np.asarray(r["box"]), np.asarray(r["cls_scores"])
    if arch == "slim_yolo_v2":
        pred = ref["t"][-1].astype(np.float32) * np.float32(2.0 ** -ref["sa"][-1])
        box, sc = O.head_decode(pred, size, anchors, classes)
        return np.asarray(box), np.asarray(sc)
    preds = W.preds_float(ref)
    if arch == "yolo_v2":
        box, sc = FP.head_decode_v2(preds[0], size, anchors, classes, 32)
    else:
        box, sc = FP.tiny_head_decode(preds, size, anchors, classes, level_strides=(8, 16, 32))
    return np.asarray(box), np.asarray(sc)


def _pick_conf(sc, most=300):
    """a confidence threshold for heads of up to 11 466 anchors whose synthetic weights put the scores of all of them in one
    narrow band (0.05 .. 0.5 with 2 classes, below 0.05 with 20): the lowest midpoint between two of the REFERENCE's distinct
    best-class scores, at least 4e-5 apart (ten times the score tolerance on either side), that at most `most` anchors of an
    image pass (the head keeps up to 4096 candidates per image) and at least one does"""
    m = sc.max(axis=2)
    v = np.unique(m.astype(np.float64))
    for j in range(len(v) - 1):
        c = 0.5 * (v[j] + v[j + 1])
        if v[j + 1] - v[j] > 4e-5 and c >= 0.01 and int((m > c).sum(axis=1).max()) <= most:
            return float(c)
    raise AssertionError("no threshold separates the reference's scores")


def _dets(box, sc, conf, classes):
    from oracle import yolo_oracle as O
    return [O.postprocess(box[i], sc[i], conf, 0.5, classes) for i in range(box.shape[0])]


def _check_small_against_restatement(net, x, ref, head):
    """test_int8_wide_models._check_against_restatement for the two graphs whose heads int8_wide_ref.detect does not decode:
    the same assertions with the same tolerances"""
    from helpers import dets_match
    B = x.shape[0]
    sa_in, sa_eff = net.get_act_exponents()
    assert sa_eff == ref["sa"]
    out = net.forward(x, tap=True)
    for t in range(net.num_tensors):
        got = np.rint(net.get_tensor(t, B).astype(np.float64) * 2.0 ** sa_eff[t]).astype(np.int64)
        assert np.array_equal(got, ref["t"][t]), "tensor %d differs in %d places" % (t, int((got != ref["t"][t]).sum()))
    assert net.counters() == ref["sat"]
    box, sc, dets = head
    cb, cs, cc = net.candidates(B)
    assert np.allclose(cb, box, atol=2e-5, rtol=0)
    assert np.allclose(cs, sc.max(axis=2), atol=2e-6, rtol=1e-5)
    for i in range(B):
        ok, msg = dets_match(dets[i][:3], out[i], all_scores=sc[i].max(axis=1))
        assert ok, (i, msg)
    return out


def _route_findings(net, ql, pred, narrow, run):
    """family and flags y355_net_layer_route reports against predict() and the loaded layers; returns (findings, reached)"""
    bad, reached = [], set()
    for i, (e, L) in enumerate(zip(pred, ql)):
        r = net.layer_route(i)
        fam = T.FAMILY.get(r & 0xff, "?")
        if fam != e["family"]:
            bad.append("%s: layer %d ran %s, predicted %s (tile %s)" % (run, i, fam, e["family"], e["tile"]))
        else:
            reached.add((fam, e["tile"], bool(r & T.RESIDUAL)))
        if fam in (T.FIRST, T.FRONT):                      # (the first-layer kernels report their own flags)
            continue
        want = (0 if narrow[i] else T.EPI64) | (T.RESIDUAL if e["residual"] else 0) | (T.PER_CHANNEL if T.is_per_channel(L) else 0)
        if (r & ~0xff) != want:
            bad.append("%s: layer %d flags %#x, the loaded layers imply %#x" % (run, i, r & ~0xff, want))
    return bad, reached


def _same_dets(a, b, B):
    return all(all(np.array_equal(u, v) for u, v in zip(a[i], b[i])) for i in range(B))


def _calibration(net, tag, ql, out):
    """two steps on one handle against net_calib_ref.step on the same trackers; returns the trackers' exponents"""
    from test_net_calibration import _same_state
    _, arch, size, classes, mb, B, pc = T.case(tag)
    bad = out["calibration"]
    tr = [R.Tracker() for _ in range(len(R.graph(arch).C) + 1)]
    for k, (freeze, seed) in enumerate([(True, 500), (False, 510)]):
        x = T.images_of(seed, B, size)
        got = net.calibrate(x, freeze=freeze)
        r = R.step(arch, x, ql, tr, freeze, predc=T.predc_of(arch, classes))
        if got != (r["sa_in"], r["sa"]):
            bad.append("step %d: exponents %s, restatement %s" % (k, got, (r["sa_in"], r["sa"])))
        try:
            _same_state(net, tr, r)
        except AssertionError as e:
            bad.append("step %d: tracker state or maxima: %s" % (k, str(e)[:400]))
        # every tensor the pass wrote.  get_tensor divides by the exponents in force AFTER the step (got[1]), so multiplying by
        # them gives the bytes back whatever exponent they were written under; r["t"] holds the bytes the pass wrote -- for a
        # tensor with a late producer (r["late"]) under r["first_sa"], the first producer's exponent, not under r["sa"]
        for t in range(net.num_tensors):
            b = _bytes(net, t, B, got[1])
            if not np.array_equal(b, r["t"][t]):
                bad.append("step %d: tensor %d (written under exponent %d%s) differs in %d places" %
                           (k, t, r["first_sa"][t] if r["first_sa"][t] is not None else r["sa"][t], ", late producer" if t in r["late"] else "",
                            int((b != r["t"][t]).sum())))
        del r
    out["stat"] = T.stat_set(T.predict_case(tag))
    return net.get_act_exponents()


def _forwards(net, tag, ql, exps, out):
    from yolo355 import _ffi
    from test_int8_wide_models import _check_against_restatement
    _, arch, size, classes, mb, B, pc = T.case(tag)
    sa_in, sa = exps
    x = T.images_of(600, B, size)
    qref = _ref_layers(ql)
    ref = R.forward_int(arch, x, qref, sa_in, sa, T.predc_of(arch, classes))
    ref["sa_in"] = sa_in
    narrow = T.narrow_of(arch, ql, sa_in, sa)
    wide = {i for i, n in enumerate(narrow) if not n}
    fused = arch in SMALL and not any(T.is_per_channel(L) for L in ql[:2])
    # ---- tap
    box, sc = _decode(arch, ref, x, qref, size, classes)
    conf = _pick_conf(sc)
    net.set_thresholds(conf, 0.5)
    out["conf"] = (conf, [int(v) for v in (sc.max(axis=2) > conf).sum(axis=1)])
    if arch in SMALL:
        o_tap = _check_small_against_restatement(net, x, ref, (box, sc, _dets(box, sc, conf, classes)))
    else:
        o_tap = _check_against_restatement(net, x, ref, arch, size, T.anchors_of(arch), classes, conf)
    bad, reached = _route_findings(net, ql, T.predict_case(tag, wide), narrow, "tap")
    out["forward"] += bad
    out["routes"] |= reached
    # ---- plain, and plain with the persistent walk on 7 workgroups: the same tensors, counters and detections
    plain = None
    for run, wgs in (("plain", 0), ("wg7", 7)):
        bad = out["forward"] if run == "plain" else out["wg7"]
        net.set_option(_ffi.NET_OPT_WORKGROUPS, wgs)
        try:
            o = net.forward(x)
            skip0 = False
            if fused:                                             # the fused launch does not write conv1's own map
                try:
                    net.get_tensor(0, B)
                    bad.append("%s: tensor 0 was readable behind the fused front end" % run)
                except _ffi.Y355Error as e:
                    skip0 = e.code == _ffi.ENOTREADY
                    if not skip0:
                        raise
            got = [None if (skip0 and t == 0) else _bytes(net, t, B, sa) for t in range(net.num_tensors)]
            for t, b in enumerate(got):
                if b is not None and not np.array_equal(b, ref["t"][t]):
                    bad.append("%s: tensor %d differs from the restatement in %d places" % (run, t, int((b != ref["t"][t]).sum())))
                if plain is not None and (b is None) != (plain[t] is None):
                    bad.append("%s: tensor %d written in one of the two plain forwards only" % (run, t))
                elif plain is not None and b is not None and not np.array_equal(b, plain[t]):
                    bad.append("%s: tensor %d differs from the plain forward's bytes" % (run, t))
            if net.counters() != ref["sat"]:
                bad.append("%s: clamp count %d, restatement %d" % (run, net.counters(), ref["sat"]))
            if not _same_dets(o, o_tap, B):
                bad.append("%s: detections differ from the tap forward's" % run)
            rb, reached = _route_findings(net, ql, T.predict_case(tag, wide, fused_front=fused), narrow, run)
            bad += rb
            out["routes"] |= reached
            if plain is None:
                plain = got
        finally:
            net.set_option(_ffi.NET_OPT_WORKGROUPS, 0)
    return x


def _wide(net, tag, ql, exps, x, out):
    """three stride-32 layers on the 64-bit epilogue at the production tiles: per tensor (all channels lowered equally) and per
    channel (lowered by c mod 17 more), each a tap forward of one image against the restatement on the reloaded layers"""
    _, arch, size, classes, mb, B, pc = T.case(tag)
    sa_in, sa = exps
    bad = out["wide"]
    g = R.graph(arch)
    convs = [o for o in g.ops if o["op"] == "conv"]
    narrow0 = T.narrow_of(arch, ql, sa_in, sa)
    base = T.predict_case(tag, {i for i, n in enumerate(narrow0) if not n})
    s32 = [o for o in convs if g.div[o["i"]] == 32 and not o["s2"]]
    pick = {
        "residual 3x3 (tile 5 + residual)": next(o for o in s32 if o["res"] >= 0 and base[o["layer"]]["tile"] == 5),
        "3x3 512 -> 1024 (ring I4 while narrow)": next(o for o in s32 if base[o["layer"]]["tile"] == "I4"),
        "1x1 (pointwise while narrow)": next(o for o in s32 if base[o["layer"]]["family"] == T.POINTWISE and o["cout"] is not None),
    }
    x1 = x[:1]

    def compare(mode, q2):
        """a tap forward of the loaded layers q2 against the restatement: every tensor, the clamp count, every layer's route"""
        narrow = T.narrow_of(arch, q2, sa_in, sa)
        ref = R.forward_int(arch, x1, _ref_layers(q2), sa_in, sa, T.predc_of(arch, classes))
        net.forward(x1, tap=True)
        for t in range(net.num_tensors):
            b = _bytes(net, t, 1, sa)
            if not np.array_equal(b, ref["t"][t]):
                bad.append("%s: tensor %d differs in %d places" % (mode, t, int((b != ref["t"][t]).sum())))
        if net.counters() != ref["sat"]:
            bad.append("%s: clamp count %d, restatement %d" % (mode, net.counters(), ref["sat"]))
        pred = T.predict_case(tag, {i for i, n in enumerate(narrow) if not n})
        bad.extend(_route_findings(net, q2, pred, narrow, mode)[0])
        return pred

    try:
        for mode in ("per tensor", "per channel"):
            q2 = [dict(L) for L in ql]
            for name, o in pick.items():
                li = o["layer"]
                cout = np.asarray(ql[li]["q_w"]).shape[0]
                spread = (np.arange(cout) % 17) if mode == "per channel" else np.zeros(cout, np.int64)
                for d in range(0, 25):                            # the restatement decides: the smallest lowering that needs 64 bits
                    q2[li]["e_w"] = (int(ql[li]["e_w"]) - d - spread).astype(np.int32)
                    if not T.narrow_of(arch, q2, sa_in, sa, only=li):
                        break
                else:
                    raise AssertionError("%s: no lowering up to 24 bits leaves the 32-bit epilogue" % name)
                # valid for the engine: every accumulator shift at most 24 (Y355_RQ_SHL_MAX_NET of csrc/y355_requant.h), the requantising
                # shift inside [-20, 62] (refresh_layer_i8)
                Fb = max(sa[o["i"]] + int(q2[li]["e_w"].max()), int(ql[li]["e_b"]))
                assert Fb - sa[o["i"]] - int(q2[li]["e_w"].min()) <= 24, name
                assert -20 <= Fb + W.ACT[o["act"]][0] - sa[o["o"]] <= 62, name
                _load(net, li, q2[li])
            pred = compare(mode, q2)
            for name, o in pick.items():
                li, r = o["layer"], net.layer_route(o["layer"])
                if T.FAMILY.get(r & 0xff) == pred[li]["family"]:
                    out["routes_wide"].add((pred[li]["family"], pred[li]["tile"], bool(r & T.RESIDUAL), mode))
                if not r & T.EPI64 or bool(r & T.PER_CHANNEL) != (mode == "per channel"):
                    bad.append("%s, %s: route %#x" % (mode, name, r))
                if pred[li]["family"] not in (T.GENERIC4, T.GENERIC8) or pred[li]["tile"] != pred[li]["stat"]:
                    bad.append("%s, %s: predict() does not fall back to the generic tile: %s" % (mode, name, pred[li]))
        # the other way round.  Under these weights every residual layer of the deeper levels needs 64 bits as it is loaded, so the
        # 32-bit residual epilogue never runs on tile 5: the residual layer once more with the same weights on k fewer bits,
        # q_w >> k at exponent e_w - k (a coarser but valid layer: F falls by k, and with it the shift of the residual term in the
        # negative branch, which is what does not fit 32 bits), for the smallest k at which the restatement says 32 bits hold
        o = pick["residual 3x3 (tile 5 + residual)"]
        li = o["layer"]
        q3 = [dict(L) for L in ql]
        for k in (1, 2, 3, 4, 5, 6):
            q3[li]["q_w"], q3[li]["e_w"] = np.asarray(ql[li]["q_w"]) >> k, int(ql[li]["e_w"]) - k
            if T.narrow_of(arch, q3, sa_in, sa, only=li):
                break
        else:
            raise AssertionError("the residual layer needs 64 bits however small its weights")
        for oo in pick.values():                                  # (the other two layers as they were)
            _load(net, oo["layer"], q3[oo["layer"]])
        pred = compare("narrow residual", q3)
        r = net.layer_route(li)
        if r & T.EPI64 or not r & T.RESIDUAL:
            bad.append("narrow residual: route %#x" % r)
        if T.FAMILY.get(r & 0xff) == pred[li]["family"]:
            out["routes_wide"].add((pred[li]["family"], pred[li]["tile"], bool(r & T.RESIDUAL), "narrow residual"))
    finally:
        for o in pick.values():
            _load(net, o["layer"], ql[o["layer"]])


def run_case(tag):
    """the GPU runs of a case and their comparisons, once: dict(calibration / forward / wg7 / wide: findings (empty = equal), stat
    and routes: what was reached, error: the traceback of a phase that raised -- later phases then did not run)"""
    if tag in _RUNS:
        return _RUNS[tag]
    _, arch, size, classes, mb, B, pc = T.case(tag)
    out = dict(calibration=[], forward=[], wg7=[], wide=[], stat=set(), routes=set(), routes_wide=set(), conf=None, error=None, done=[], max_batch=mb)
    _RUNS[tag] = out
    ql = T.qlayers_of(tag, 21)
    net = None
    try:
        net = _open(tag, ql, out)
        out["exps"] = _calibration(net, tag, ql, out)
        out["done"].append("calibration")
        _forwards(net, tag, ql, out["exps"], out)
        out["done"].append("forward")
    except Exception:
        out["error"] = traceback.format_exc()
    finally:
        if net is not None:
            net.close()
    return out


def _open(tag, ql, out):
    """the case's handle with its layers loaded"""
    from yolo355 import _ffi
    from yolo355.netengine import Net
    _, arch, size, classes, mb, B, pc = T.case(tag)
    try:
        net = Net(arch, size, classes, T.anchors_of(arch), conf_thresh=T.CONF, nms_thresh=0.5, max_batch=mb, dtype="int8")
    except _ffi.Y355Error:
        # the handle does not fit beside the card's other users: the smallest max_batch that selects the same tiles in every layer
        out["max_batch"] = _equivalent_max_batch(tag)
        if out["max_batch"] == mb:
            raise
        net = Net(arch, size, classes, T.anchors_of(arch), conf_thresh=T.CONF, nms_thresh=0.5, max_batch=out["max_batch"], dtype="int8")
    for i, q in enumerate(ql):
        _load(net, i, q)
    return net


def run_wide(tag="v3_448_mb64"):
    """the wide-epilogue runs, once, on a handle of the case's own configuration under the exponents its calibration left (a
    handle of its own, so that no single test carries all the references of the case)"""
    res = run_case(tag)
    if "wide" in res["done"] or "calibration" not in res["done"] or res.get("wide_tried"):
        return res
    res["wide_tried"] = True
    ql = T.qlayers_of(tag, 21)
    net = None
    try:
        net = _open(tag, ql, res)
        net.set_act_exponents(*res["exps"])
        net.set_thresholds(0.99, 0.5)                             # (these runs compare tensors and counters, not the head)
        _, arch, size, classes, mb, B, pc = T.case(tag)
        _wide(net, tag, ql, res["exps"], T.images_of(600, B, size), res)
        res["done"].append("wide")
    except Exception:
        res["error"] = traceback.format_exc()
    finally:
        if net is not None:
            net.close()
    return res


def _assert_phase(tag, phase, keys):
    res = run_case(tag)
    assert phase in res["done"], "%s: the %s phase did not finish:\n%s" % (tag, phase, res["error"])
    for k in keys:
        assert not res[k], "%s, %s:\n%s" % (tag, k, "\n".join(res[k][:40]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", T.TAGS)
def test_two_calibration_steps_equal_the_restatement_in_state_and_tensors(tag):
    _assert_phase(tag, "calibration", ["calibration"])
    res = run_case(tag)
    print(tag, "max_batch", res["max_batch"], "statistics and write pass on (tile, residual):", sorted(res["stat"]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", T.TAGS)
def test_forwards_on_the_calibrated_exponents_are_bit_exact(tag):
    _assert_phase(tag, "forward", ["forward"])
    res = run_case(tag)
    print(tag, "confidence threshold and anchors passing it per image:", res["conf"])
    print(tag, "forward routes (family, tile or ring, residual):", sorted(res["routes"], key=str))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", T.TAGS)
def test_seven_persistent_workgroups_change_nothing(tag):
    _assert_phase(tag, "forward", ["wg7"])


@pytest.mark.gpu
def test_wide_epilogue_at_the_production_tiles():
    run_wide()
    _assert_phase("v3_448_mb64", "wide", ["wide"])
    seen = run_case("v3_448_mb64")["routes_wide"]
    print("64-bit epilogue ran on (family, tile, residual, weights):", sorted(seen, key=str))
    for mode in ("per tensor", "per channel"):
        assert (T.GENERIC8, 5, True, mode) in seen and (T.GENERIC8, 5, False, mode) in seen, sorted(seen, key=str)
    assert (T.GENERIC8, 5, True, "narrow residual") in seen, sorted(seen, key=str)


@pytest.mark.gpu
def test_every_route_of_a_deployed_net_ran_checked():
    """what predict() requires of the table on the CPU, on what the runs reported: the families y355_net_layer_route gave, layer
    by layer equal to predict()'s (a layer whose family differed does not count)"""
    stat, fwd = set(), set()
    for tag in T.TAGS:
        res = run_case(tag)
        if "calibration" in res["done"] and not res["calibration"]:
            stat |= res["stat"]
        fwd |= res["routes"]
    assert T.required("stat") <= stat, sorted(T.required("stat") - stat)
    assert T.required("forward") <= fwd, sorted(T.required("forward") - fwd, key=str)
