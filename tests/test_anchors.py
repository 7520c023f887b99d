"""The anchor fit on the GPU (csrc/anchors.hip through yolo355/anchors.py) against the reference's own results
(tests/golden/anchors.npz) and the host restatement (tests/anchors_ref.py), at the smallest shapes that can still go wrong
(tests/anchors_cases.py).  Discrete outcomes (initial centroids, iteration count, groups, counts) are equal exactly: the golden
records the margins with which the reference decided each of them.  Centroids within 2 n 2^-53 relative and the loss within
14 n^2 2^-53 absolute (anchors_cases.centroid_bound / loss_bound say why)."""
import numpy as np
import pytest
import torch

import anchors_cases as AC
import anchors_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return AC.load_golden()


@pytest.fixture(scope="module")
def A():
    from yolo355 import anchors
    return anchors


def run(A, wh, k, first=None, u=None, init_index=None, iters=AC.ITERS, max_restarts=None, boxes_on_device=False):
    """one fit on a handle of its own -> (list of Restart, best, groups of every restart, the handle's score of the best)"""
    R_ = len(init_index) if init_index is not None else len(first)
    h = A.AnchorFit(len(wh), max_restarts or R_, max(k, 1))
    try:
        h.set_boxes(torch.from_numpy(wh).to(h.device) if boxes_on_device else wh)
        h.fit(k, first=first, u=u, init_index=init_index, iters=iters, convergence=AC.CONVERGENCE)
        runs, best = h.result()
        return runs, best, [h.assignments(r) for r in range(R_)], h.score(runs[best].anchors, with_index=True)
    finally:
        h.close()


def case_start(gold, tag):
    c = AC.case(tag)
    if c["init_index"] is not None:
        return c, dict(init_index=np.array([c["init_index"]], np.int32))
    return c, dict(first=gold[tag + "/first"].astype(np.int32), u=gold[tag + "/u"].reshape(1, -1))


def same_bytes(a, b):
    return all(x.anchors.tobytes() == y.anchors.tobytes() and x.init.tobytes() == y.init.tobytes() and x.loss == y.loss
               and x.iterations == y.iterations and np.array_equal(x.counts, y.counts) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("tag", AC.TAGS)
def test_fit_equals_the_reference(gold, A, tag):
    c, start = case_start(gold, tag)
    n, k = c["n"], c["k"]
    runs, best, groups, (mean_iou, s_counts, s_idx) = run(A, c["wh"], k, iters=c["iters"], **start)
    r = runs[0]
    assert best == 0 and len(runs) == 1
    assert np.array_equal(r.init, gold[tag + "/init"])                                   # boxes, copied bit for bit
    assert r.iterations == int(gold[tag + "/iterations"][0])
    assert np.array_equal(groups[0], gold[tag + "/groups"])
    assert np.array_equal(r.counts, np.bincount(gold[tag + "/groups"], minlength=k))
    want = gold[tag + "/anchors"]
    err = np.abs(r.anchors - want)
    print("%s: max rel centroid err %.3g (bound %.3g), loss err %.3g (bound %.3g)"
          % (tag, (err / np.maximum(want, 1e-300)).max(), AC.centroid_bound(n), abs(r.loss - gold[tag + "/losses"][-1]), AC.loss_bound(n)))
    assert (err <= AC.centroid_bound(n) * want).all(), (r.anchors, want)
    assert abs(r.loss - gold[tag + "/losses"][-1]) <= AC.loss_bound(n)
    # score on the fitted anchors: the groups that the NEXT step would form; the fit has converged (or is the cap case), so with
    # equal groups in the last two steps they are the last groups
    if tag != "n1500_k5_iters3":
        assert np.array_equal(s_counts, r.counts) and np.array_equal(s_idx, groups[0])
    w_mean, w_counts, w_idx = R.score(c["wh"], r.anchors)
    assert np.array_equal(s_idx, w_idx) and np.array_equal(s_counts, w_counts)
    assert abs(mean_iou - w_mean) <= 2.0 * n * AC.EPS * w_mean


def test_two_runs_and_more_restarts_give_the_same_bytes(gold, A):
    c, start = case_start(gold, "n4097_k9")
    a = run(A, c["wh"], c["k"], **start)
    b = run(A, c["wh"], c["k"], **start)
    assert same_bytes(a[0], b[0]) and np.array_equal(a[2][0], b[2][0]) and a[3][0] == b[3][0]
    first, u = A.draws(c["n"], c["k"], c["seed"], restarts=3)
    assert first[0] == start["first"][0] and np.array_equal(u[0], start["u"][0])
    three = run(A, c["wh"], c["k"], first=first, u=u, max_restarts=5)
    assert same_bytes(three[0][:1], a[0]) and np.array_equal(three[2][0], a[2][0])        # restart 0 does not see its neighbours


def test_restarts_that_finish_apart_keep_their_own_results(A):
    wh, k = AC.boxes("b1500"), 5
    first, u = A.draws(len(wh), k, 3, restarts=4)
    runs, best, groups, _ = run(A, wh, k, first=first, u=u)
    want = [R.fit(wh, k, first=int(first[r]), u=u[r], iters=AC.ITERS, convergence=AC.CONVERGENCE) for r in range(4)]
    steps = [w["iterations"] for w in want]
    assert len(set(steps)) > 1 and max(steps) - min(steps) >= 3, steps                   # or the case shows nothing
    for r in range(4):
        solo = run(A, wh, k, first=first[r:r + 1], u=u[r:r + 1])
        assert same_bytes(solo[0], runs[r:r + 1]) and np.array_equal(solo[2][0], groups[r]), r
        assert runs[r].iterations == steps[r] and np.array_equal(groups[r], want[r]["groups"]) and np.array_equal(runs[r].init, want[r]["init"])
        assert abs(runs[r].loss - want[r]["loss"]) <= AC.loss_bound(len(wh))
    losses = [x.loss for x in runs]
    assert best == int(np.argmin(losses))                                                # np.argmin: the first of equal minima
    # equal losses: two restarts with one start
    twins, tbest, _, _ = run(A, wh, k, first=first[[1, 2, 2]], u=u[[1, 2, 2]])
    assert twins[1].loss == twins[2].loss and tbest == (0 if twins[0].loss <= twins[1].loss else 1)


def test_score_on_config_constants(A):
    wh = AC.boxes("b4097")
    h = A.AnchorFit(len(wh), 1, 16)
    try:
        h.set_boxes(wh)
        for anchors in (AC.CONFIG_ANCHORS_PX, np.concatenate([np.zeros((1, 2)), AC.CONFIG_ANCHORS_PX[::-1], AC.CONFIG_ANCHORS_PX[:1]])):
            mean, counts, idx = h.score(anchors, with_index=True)
            w_mean, w_counts, w_idx = R.score(wh, anchors)
            assert np.array_equal(idx, w_idx) and np.array_equal(counts, w_counts) and counts.sum() == len(wh)
            assert abs(mean - w_mean) <= 2.0 * len(wh) * AC.EPS * w_mean
            assert h.score(anchors)[0] == mean
        assert counts[0] == 0 and counts[-1] == 0                                        # (0, 0) never wins, a repeated anchor loses the tie
    finally:
        h.close()


def test_fit_anchors_and_the_handle_agree(gold, A):
    c, start = case_start(gold, "n257_k3")
    runs, best, groups, (mean_iou, _, _) = run(A, c["wh"], c["k"], first=A.draws(c["n"], c["k"], c["seed"], 3)[0], u=A.draws(c["n"], c["k"], c["seed"], 3)[1])
    res = A.fit_anchors(c["wh"], c["k"], seed=c["seed"], restarts=3)
    assert same_bytes(res.all, runs) and res.best == best and res.mean_iou == mean_iou
    assert res.anchors.tobytes() == runs[best].anchors.tobytes() and res.loss == runs[best].loss and res.iterations == runs[best].iterations
    assert np.array_equal(res.counts, runs[best].counts) and np.array_equal(res.groups, groups[best])
    assert np.array_equal(res.all[0].init, gold["n257_k3/init"])                         # restart 0 is the reference's run for `seed`
    d = AC.case("four_dup_k6")
    res = A.fit_anchors(d["wh"], d["k"], plus=False, init_index=[d["init_index"]])
    assert np.array_equal(res.anchors, gold["four_dup_k6/anchors"]) and np.array_equal(res.groups, gold["four_dup_k6/groups"])
    res = A.fit_anchors(d["wh"], 4, plus=False, seed=5, restarts=2)                       # the reference's random.sample
    assert np.array_equal(res.all[1].init, d["wh"][A.sample_indices(64, 4, 5, 2)[1]])


def test_device_and_host_boxes_agree_and_bad_arguments_are_named(gold, A):
    c, start = case_start(gold, "n1500_k5")
    a = run(A, c["wh"], c["k"], **start)
    b = run(A, c["wh"], c["k"], boxes_on_device=True, **start)
    assert same_bytes(a[0], b[0]) and np.array_equal(a[2][0], b[2][0])
    from yolo355._ffi import Y355Error
    h = A.AnchorFit(16, 2, 4)
    try:
        with pytest.raises(Y355Error, match="no boxes set"):
            h.fit(2, first=[0], u=[[0.5]])
        bad = np.full((4, 2), 3.0)
        bad[1, 1] = np.nan
        with pytest.raises(Y355Error, match="box 1: h"):
            h.set_boxes(bad)
        bad[1, 1] = 0.0
        with pytest.raises(Y355Error, match="finite and > 0"):
            h.set_boxes(torch.from_numpy(bad).to(h.device))
        assert h._lib.y355_anchors_num_boxes(h._h) == 0
        with pytest.raises(Y355Error, match="max_boxes"):
            h.set_boxes(np.ones((17, 2)))
        h.set_boxes(np.arange(2, 18, dtype=np.float64).reshape(8, 2))
        for kw, text in ((dict(k=5, first=[0], u=[[0.5] * 4]), "k must be"), (dict(k=2, first=[0, 1, 2], u=[[0.5]] * 3), "restarts must be"),
                         (dict(k=2, first=[8], u=[[0.5]]), r"first\[0\]"), (dict(k=2, first=[0], u=[[1.0]]), r"u\[0\]\[0\]"),
                         (dict(k=2, init_index=[[0, 9]]), r"init_index\[0\]\[1\]"), (dict(k=2, first=[0], u=[[0.5]], iters=0), "max_iters"),
                         (dict(k=2, first=[0], u=[[0.5]], convergence=float("nan")), "convergence")):
            with pytest.raises(Y355Error, match=text):
                h.fit(**kw)
        with pytest.raises(Y355Error, match="no fit made"):
            h.result()
        import ctypes
        i32 = (ctypes.c_int32 * 2)(0, 1)
        u = (ctypes.c_double * 1)(0.5)
        assert h._lib.y355_anchors_fit(h._h, 2, 1, 10, 1e-6, i32, u, i32, None) == -1 and "exactly one start" in h._lib.y355_anchors_last_error().decode()
        assert h._lib.y355_anchors_fit(h._h, 2, 1, 10, 1e-6, None, None, None, None) == -1
        with pytest.raises(Y355Error, match="anchors must be"):
            h.score([[1.0, -2.0]])
        h.fit(2, first=[3], u=[[0.25]])
        with pytest.raises(Y355Error, match="restart must be"):
            h.assignments(1)
        assert h.result()[0][0].iterations >= 2
    finally:
        h.close()


def test_the_command_line_tool(A, tmp_path):
    import json
    from yolo355.tools import fit_anchors as cli
    wh = AC.boxes("b257")
    coco = {"images": [{"id": 3, "width": 500, "height": 375}],
            "annotations": [{"image_id": 3, "bbox": [1.0, 2.0, float(w), float(h)], "area": float(w * h)} for w, h in wh]}
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(coco))
    out = cli.main(["-d", "coco", "--annotations", str(path), "-na", "6", "-size", "320", "--restarts", "3", "--seed", "2", "--stride", "16", "--json"])
    boxes = A.coco_boxes(str(path), 320)
    res = A.fit_anchors(boxes, 6, seed=2, restarts=3)
    assert out["boxes"] == len(boxes) == 257 and out["best_restart"] == res.best and out["mean_iou"] == res.mean_iou
    assert np.array_equal(out["anchors_px"], res.anchors) and out["counts"] == res.counts.tolist() and out["loss"] == res.loss
    assert np.array_equal(out["anchors_grid_units"], res.anchors / 16.0) and np.array_equal(out["anchors_px_by_area"], A.sort_by_area(res.anchors))
    cli.main(["-d", "coco", "--annotations", str(path), "-na", "6", "-size", "320", "--restarts", "2", "--levels", "2"])      # the text form
