"""The y355_net families while several handles share the GPU: bench.py's measure_net regime (three Net handles on three HIP
streams, steps alternating without a synchronisation in between), which no other test checks a byte of.  The cases, and what
the table must reach, are in tests/net_shared_cases.py.

Per case (open_set, once; the handles stay open for the case's variants and are closed when another case needs the memory):
  anchor   with the device idle, handle 0 runs a plain forward (flags 0: the production route, fused front end) of the periodic
           full batch into zero-filled buffers: `ref` = the four output tensors, the prediction maps, the int8 clamp count.
           ref is periodic with period P; it equals, byte for byte, a forward of the P base images alone (batch independence);
           int8: the prediction maps of the P base images equal net_calib_ref.forward_int on the same layers and exponents in
           every element and the clamp count is the restatement's (B / P times it for the full batch; y355_net_counters is the
           count of the LAST forward, include/yolo355.h); bf16: the link to float64 is test_bf16_layers on the same model and
           first image.  Every other handle, alone, reproduces ref byte for byte.
  shared   rounds of 2 x handles forwards, forward i on stream i mod handles into its own zero-filled buffers, nothing but the
           timing events between them, one synchronisation, every buffer set torch.equal to ref; after the last round every
           handle's prediction maps and clamp count against ref.  A timing event before and after each forward, read against one
           common first event, shows whether forwards of two handles were in flight at the same time: the test FAILS if that
           happened in no round (a condition on the test, not a tolerance on the kernels) and prints the share of rounds.
Variants on the same handles and the same ref: Y355_NET_OPT_WORKGROUPS 128 and 192 (half the rounds each); two calibration
steps on handle 0 beside the other handles' forwards (state, exponents and maxima bit for bit against net_calib_ref.step, the
forwards still equal to ref, handle 0 back on ref afterwards); the frames route (forward_frames_device, one 480 x 640 uint8
batch; its stand-alone result equals forward on normalize_frames(resize_linear_u8(frames)) first); and three UNLIKE handles --
an int8 YOLOv3tiny Net, a bf16 SlimYOLOv2 Net and the int8 SlimYOLOv2 Engine -- whose kernels have different LDS and register
footprints, each against its own stand-alone result.
The confidence threshold of a case is taken from handle 0's own candidates (_pick_conf: at most 200 anchors of an image pass,
more where an int8 head puts more than that on one score, and at least one does), so that every output buffer holds
detections and no forward drops candidates; a condition on the test's inputs, the comparisons are all byte for byte.
No captured graphs, one process, at most three streams with work in flight.

MEASURED: one run on an MI355X (profiles/net_shared_gpu.md has the table per case and variant): 21 shared runs, 480 rounds, no
mismatch.  Rounds in which forwards of two handles were in flight together: 100 % in every run (two or more handles in flight
during 94 to 99 % of the busy time; 54 % for the unlike neighbours, whose forwards differ in length) except v2_i8's calibration
variant, 2 of 4 rounds, the most it can show: its single forwarding handle has handle 0's calibration beside it only in the two
rounds that take a step.  Families that ran shared: FRONT, THIN, RING (I0 .. I5 and the bf16 rings), POINTWISE, GENERIC4, GENERIC8;
int8 layer by layer equal to predict() under the calibrated exponents, every (family, tile) of required("forward") with FRONT in
FIRST's place; the fewest work items of a RING / GENERIC8 launch times B: 256 to 512.  Every handle was created at its row's
max_batch (no fall-back to 48).  Wall: 20.8 s for the 21 GPU tests of this module, the longest test 3.39 s (v2_i8 calibration: three
CPU restatement steps), the GPU rounds of a test 0.02 to 0.45 s; in the same run of the whole suite test_int8_production_tiles took
39.3 s, its longest test 8.82 s (v3_448_mb64; 49.8 s and 11.8 s in that module's docstring, from an earlier machine), so no round
count was reduced.  Not measured: CU co-residency itself (no profiler run); the evidence is the timing events and the counts.
"""
import copy
import time

import numpy as np
import pytest
import torch

import int8_tile_cases as T
import net_calib_ref as R
import net_shared_cases as S

_SETS = {}                      # tag -> HandleSet (open handles)
_RESTATE = {}                   # tag -> net_calib_ref.forward_int of the P base images, once per case
_ROUTES = {}                    # bf16 tag -> dict(plain = families of the plain forward, tap = of the tap forward)
_REACHED = {}                   # int8 tag -> {(family, tile or ring, residual)} the plain forward reported, equal to predict()'s


# ---------------------------------------------------------------------------------------------------- CPU
def test_every_int8_row_fills_the_device_at_its_batch():
    """the smallest work-item count among a row's RING and GENERIC8 layers, times the row's B, is at least the device's 256
    compute units -- recomputed from G_TILES / RINGS and predict(), tap route and the plain route with the fused front end"""
    for tag in S.INT8_TAGS:
        B = S.case(tag)[4]
        for fused in ((False, True) if S.case(tag)[1] in S.SMALL else (False,)):
            items = S.work_items(tag, fused_front=fused)
            assert items, tag
            n, fam, tile, layer = min(items, key=lambda v: v[0])
            print(tag, "B", B, "fused front" if fused else "tap", "fewest items per image:", n, fam, tile, "layer", layer, "->", n * B)
            assert n * B >= S.CUS, (tag, n, B)
    # the figures the batch sizes rest on: 4 items per image for tile 5 and ring I4 on a 13 x 13 map, 2 for ring I5
    per = {(f, t): n for tag in ("v2_i8",) for n, f, t, _ in S.work_items(tag)}
    assert per[(T.GENERIC8, 5)] == 4
    tiny416 = T.predict("tiny_yolo_v3", [416, 416], 128, T.predc_of("tiny_yolo_v3", 2))
    assert {e["tile"] for e in tiny416 if e["family"] == T.RING} >= {"I4", "I5"}


def test_int8_rows_reach_every_ring_and_every_deployed_forward_tile():
    """the table does not drift off the deployed tiles: together the int8 rows reach the rings I0 .. I5 and every
    (family, tile) of int8_tile_cases.required("forward"), whatever the residual flag of the layer that takes it"""
    reached = set()
    for tag in S.INT8_TAGS:
        reached |= T.forward_set(S.predict_row(tag))
    rings = {t for f, t, _ in reached if f == T.RING}
    assert rings == {r[0] for r in T.RINGS} == {"I0", "I1", "I2", "I3", "I4", "I5"}, sorted(rings)
    want = {(f, t) for f, t, _ in T.required("forward")}
    got = {(f, t) for f, t, _ in reached}
    print("required", sorted(want, key=str))
    print("reached ", sorted(got, key=str))
    assert want <= got, sorted(want - got, key=str)
    # and the same on the triples without a residual: every one of them runs beside another handle as it is deployed
    assert {v for v in T.required("forward") if not v[2]} <= reached


def test_table_is_the_regime_of_the_benchmark():
    for tag, arch, dtype, size, B, handles, P, rounds, row in S.CASES:
        assert 2 <= handles <= 3 and B % P == 0 and S.DARKNET_FALLBACK % P == 0, tag
        assert (row is not None) == (dtype == "int8"), tag
        assert B == (128 if arch == "tiny_yolo_v3" else 64), tag
        assert handles == (3 if arch in S.SMALL else 2) and rounds == (40 if arch in S.SMALL else 12), tag
        assert P == (1 if arch in ("yolo_v3", "yolo_v3_spp") else 2), tag
        if row is not None:
            assert T.case(row)[1] == arch and T.case(row)[2] == size, tag
    for tags in (S.THROUGHPUT, S.CALIBRATION, S.FRAMES):
        assert set(tags) <= set(S.TAGS)


def test_overlap_and_period_helpers():
    assert S.overlapped([(0, 0.0, 2.0), (1, 1.0, 3.0)])
    assert not S.overlapped([(0, 0.0, 2.0), (0, 1.0, 3.0)])                  # one handle's own forwards do not count
    assert not S.overlapped([(0, 0.0, 1.0), (1, 1.0, 2.0), (2, 2.0, 3.0)])   # one after the other proves nothing
    assert S.overlap_time([(0, 0.0, 2.0), (1, 1.0, 3.0), (0, 4.0, 5.0)]) == (1.0, 4.0)
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    x = S.periodic(a, 6)
    assert x.shape == (6, 3, 4) and S.is_periodic(x, 2) and S.is_periodic(S.periodic(torch.from_numpy(a), 6), 2)
    x[5, 2, 3] = np.float32(-0.0) if x[5, 2, 3] == 0 else x[5, 2, 3] + 1
    assert not S.is_periodic(x, 2) and S.differing(x, S.periodic(a, 6)) == 1 and not S.same_bytes(x, S.periodic(a, 6))
    n = np.array([np.nan, 0.0], np.float32)
    assert S.same_bytes(n, n.copy()) and S.differing(n, -n) == 2


# ---------------------------------------------------------------------------------------------------- GPU
class Actor:
    """one handle of a shared round: its stream, launch(buf) (asynchronous, issued under the stream), the stand-alone result
    it must reproduce -- ref = dict(out = the four output tensors, pred = prediction maps, ctr = clamp count or None) --
    pred() / ctr() of its last forward, and bufs(): a zero-filled output buffer set"""

    def __init__(self, name, stream, launch, ref, pred, ctr, bufs):
        self.name, self.stream, self.launch, self.ref, self.pred, self.ctr, self.bufs = name, stream, launch, ref, pred, ctr, bufs


def _event():
    return torch.cuda.Event(enable_timing=True)


def shared_rounds(actors, rounds, label, side=None, final=True):
    """`rounds` rounds of 2 x len(actors) forwards, forward i by actor i mod n on its stream into its own zero-filled buffers;
    one synchronisation; every buffer set against the actor's ref.  side(it): further work issued behind the forwards of round
    `it`, returns its [(actor id, start event, end event)].  Returns the report (share of rounds with observed overlap)."""
    n = len(actors)
    bufs = [actors[i % n].bufs() for i in range(2 * n)]
    torch.cuda.synchronize()
    first = _event()
    first.record(actors[0].stream)
    hit, both, busy = 0, 0.0, 0.0
    t_start = time.perf_counter()
    for it in range(rounds):
        for b in bufs:
            for t in b:
                t.zero_()
        torch.cuda.synchronize()
        evs = []
        for i, b in enumerate(bufs):
            a = actors[i % n]
            with torch.cuda.stream(a.stream):
                e0, e1 = _event(), _event()
                e0.record()
                a.launch(b)
                e1.record()
            evs.append((i % n, e0, e1))
        if side is not None:
            evs += side(it)
        torch.cuda.synchronize()
        spans = [(k, first.elapsed_time(e0), first.elapsed_time(e1)) for k, e0, e1 in evs]
        hit += 1 if S.overlapped(spans) else 0
        o, t = S.overlap_time(spans)
        both, busy = both + o, busy + t
        for i, b in enumerate(bufs):
            a = actors[i % n]
            for k, (u, v) in enumerate(zip(a.ref["out"], b)):
                if not torch.equal(u, v):
                    diff = sum(S.differing(x, y) for x, y in zip(a.pred(), a.ref["pred"]))
                    raise AssertionError("%s: round %d, handle %d (%s), buffer %d, output tensor %d: the shared result differs from the "
                                         "stand-alone one (%d prediction values of the handle's last forward differ)" %
                                         (label, it, i % n, a.name, i, k, diff))
    wall = time.perf_counter() - t_start
    if final:
        check_final(actors, label)
    rep = dict(label=label, handles=n, rounds=rounds, overlapped=hit, share=hit / float(rounds), in_flight_together=both / busy if busy else 0.0,
               wall=wall)
    print("net_shared %-34s handles %d  rounds %3d  rounds with overlap %3d (%.0f %%)  two handles in flight %.0f %% of the busy time  %.2f s" %
          (label, n, rounds, hit, 100.0 * rep["share"], 100.0 * rep["in_flight_together"], wall))
    assert hit > 0, "%s: in none of the %d rounds were forwards of two handles in flight together: the run proves nothing" % (label, rounds)
    return rep


def check_final(actors, label):
    """after the last round: every handle's prediction maps and clamp count are those of ref"""
    for k, a in enumerate(actors):
        for j, (x, y) in enumerate(zip(a.pred(), a.ref["pred"])):
            assert S.same_bytes(x, y), "%s: handle %d (%s): prediction map %d differs from ref in %d values after the last round" % (
                label, k, a.name, j, S.differing(x, y))
        if a.ref["ctr"] is not None:
            assert a.ctr() == a.ref["ctr"], "%s: handle %d (%s): clamp count %d after the last round, ref %d" % (label, k, a.name, a.ctr(), a.ref["ctr"])


def _pick_conf(scores, caps=(200, 1000, 3500)):
    """a threshold between two of the handle's own candidate scores [P, N] that at most `cap` anchors of every image pass and
    at least one anchor does, for the smallest cap of `caps` that allows one (the head keeps up to 4096 candidates per image;
    an int8 head has few distinct scores with many anchors on each)"""
    for cap in caps:
        c = 0.0
        for s in scores:
            v, n = np.unique(s.astype(np.float64), return_counts=True)
            v, above = v[::-1], np.cumsum(n[::-1])
            k = int(np.searchsorted(above, cap, side="right"))           # the k highest distinct scores: at most cap anchors
            if not 1 <= k < len(v):
                c = None
                break
            c = max(c, 0.5 * (v[k - 1] + v[k]))
        if c is not None and 0.0 < c < 1.0 and 0 < int((scores > c).sum(axis=1).max()) <= cap:
            return float(c)
    raise AssertionError("no threshold lets between 1 and %d anchors of every image pass" % caps[-1])


class HandleSet:
    def __init__(self, tag):
        from yolo355.netengine import PRED_TAIL
        self.tag = tag
        _, self.arch, self.dtype, self.size, self.B, self.n, self.P, self.rounds, self.row = S.case(tag)
        self.int8 = self.dtype == "int8"
        self.dev = torch.device("cuda", 0)
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(self.n)]
        self.nets = []
        self.findings = []                                     # what the anchor found unequal (empty: ref stands)
        self.wall = {}
        t0 = time.perf_counter()
        self._create()
        self.pred_idx = [self.nets[0].num_tensors - k for k in PRED_TAIL[self.arch]]
        self._anchor()
        self.wall["open + anchor"] = time.perf_counter() - t0

    # ---- handles
    def _model(self):
        if self.int8:
            self.classes = S.classes_of(self.tag)
            self.anchors = T.anchors_of(self.arch)
            self.ql = T.qlayers_of(self.row, 21)
            self.base = T.images_of(600, self.P, self.size)
        else:
            import bf16_layer_ref as L
            m = L.model_of(self.arch)
            self.classes, self.anchors, self.weights = m["classes"], m["anchors"], m["weights"]
            self.base = L.images_of(self.arch, self.size, self.P)

    def _make(self, B):
        from yolo355.netengine import Net
        nets = []
        try:
            for st in self.streams:
                with torch.cuda.stream(st):
                    net = Net(self.arch, self.size, self.classes, self.anchors, conf_thresh=T.CONF, nms_thresh=0.5, max_batch=B,
                              device=self.dev, dtype=self.dtype)
                    nets.append(net)
                    if self.int8:
                        for i, q in enumerate(self.ql):
                            net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
                    else:
                        for i, (w, b) in enumerate(self.weights):
                            net.load_layer(i, w, b)
        except Exception:
            for net in nets:
                net.close()
            raise
        return nets

    def _create(self):
        """every handle under its own stream, as bench.py makes them.  A DarkNet row whose handles do not fit beside the
        card's other users at max_batch 64 runs at the equivalent max_batch 48 with B = 48 (the same tiles in every layer:
        test_int8_production_tiles._equivalent_max_batch); never below, the tiles change"""
        from yolo355 import _ffi
        self._model()
        try:
            self.nets = self._make(self.B)
        except (_ffi.Y355Error, torch.cuda.OutOfMemoryError):
            if self.arch in S.SMALL:
                raise
            torch.cuda.empty_cache()
            self.B = S.DARKNET_FALLBACK
            self.nets = self._make(self.B)
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        for net in self.nets:
            net.close()
        self.nets = []
        self.x = self.ref = None

    # ---- single runs
    def bufs(self):
        return tuple(torch.zeros_like(t) for t in self.nets[0]._buffers(self.B))

    def pred(self, k, B=None):
        return [self.nets[k].get_tensor(t, self.B if B is None else B) for t in self.pred_idx]

    def alone(self, k, x, launch=None):
        """one forward of handle k on an idle device: dict(out, pred, ctr)"""
        net, B = self.nets[k], int(x.shape[0])
        torch.cuda.synchronize()
        out = self.bufs()
        with torch.cuda.stream(self.streams[k]):
            (launch or (lambda buf: net.forward_device(x, 0, buf)))(out)
        torch.cuda.synchronize()
        if net.overflow():
            self.findings.append("handle %d: a forward dropped candidates (the threshold lets too many pass)" % k)
        return dict(out=list(out), pred=self.pred(k, B), ctr=net.counters() if self.int8 else None)

    def same(self, got, want, what, rows=None):
        """findings of two single runs; rows: compare the first `rows` images only (the others of `got` must be untouched)"""
        bad = []
        for j, (u, v) in enumerate(zip(got["out"], want["out"])):
            if rows is None:
                ok = torch.equal(u, v)
            else:
                ok = torch.equal(u[:rows], v[:rows]) and not bool(u[rows:].any())
            if not ok:
                bad.append("%s: output tensor %d differs" % (what, j))
        for j, (x, y) in enumerate(zip(got["pred"], want["pred"])):
            y = y if rows is None else y[:rows]
            if not S.same_bytes(x, y):
                bad.append("%s: prediction map %d differs in %d values" % (what, j, S.differing(x, y)))
        if rows is None and got["ctr"] != want["ctr"]:
            bad.append("%s: clamp count %s, ref %s" % (what, got["ctr"], want["ctr"]))
        return bad

    def families(self, k=0):
        from bf16_layer_ref import FAMILY as BF
        table = T.FAMILY if self.int8 else BF
        return [table.get(self.nets[k].layer_route(i) & 0xff, "?") for i in range(self.nets[k].num_layers)]

    # ---- the anchor
    def _anchor(self):
        from yolo355 import _ffi
        import test_int8_production_tiles as PT
        net0, P, B = self.nets[0], self.P, self.B
        xb = torch.from_numpy(self.base).to(self.dev)
        self.x = S.periodic(xb, B).contiguous()
        if self.int8:
            with torch.cuda.stream(self.streams[0]):
                self.exps = net0.calibrate(xb, freeze=True)
            self.saved_trackers = net0.trackers
            for net in self.nets[1:]:
                net.set_act_exponents(*self.exps)
        # the threshold, from a tap forward of the base images (which also is the only forward that takes the FIRST family)
        with torch.cuda.stream(self.streams[0]):
            net0.forward_device(xb, _ffi.F_TAP)
        torch.cuda.synchronize()
        self.tap_families = self.families()
        self.conf = _pick_conf(net0.candidates(P)[1])
        net0.overflow()                                        # (clears the flag: the tap forward ran on the constructor's threshold)
        for net in self.nets:
            net.set_thresholds(self.conf, 0.5)
        # ref, its period, batch independence
        self.ref = self.alone(0, self.x)
        self.plain_families = self.families()
        self.detections = int(self.ref["out"][3].sum())
        if self.detections <= 0:
            self.findings.append("ref holds no detection")
        for j, t in enumerate(self.ref["out"]):
            if not S.is_periodic(t, P):
                self.findings.append("ref: output tensor %d is not periodic with period %d" % (j, P))
        for j, t in enumerate(self.ref["pred"]):
            if not S.is_periodic(t, P):
                self.findings.append("ref: prediction map %d is not periodic with period %d" % (j, P))
        sub = self.alone(0, xb)
        self.findings += self.same(sub, self.ref, "the %d base images alone" % P, rows=P)
        if self.int8:
            # the restatement, once per case: every element of the prediction maps, the clamp count
            if self.tag not in _RESTATE:
                sa_in, sa = self.exps
                _RESTATE[self.tag] = R.forward_int(self.arch, self.base, PT._ref_layers(self.ql), sa_in, sa, T.predc_of(self.arch, self.classes))
            r = _RESTATE[self.tag]
            for t in self.pred_idx:
                got = PT._bytes(net0, t, P, self.exps[1])
                if not np.array_equal(got, r["t"][t]):
                    self.findings.append("tensor %d (a prediction map) differs from the restatement in %d places" % (t, int((got != r["t"][t]).sum())))
            if sub["ctr"] != r["sat"]:
                self.findings.append("clamp count of the %d base images %d, restatement %d" % (P, sub["ctr"], r["sat"]))
            if self.ref["ctr"] != (B // P) * r["sat"]:
                self.findings.append("clamp count of the full batch %d, %d x the restatement's %d expected" % (self.ref["ctr"], B // P, r["sat"]))
        for k in range(1, self.n):
            self.findings += self.same(self.alone(k, self.x), self.ref, "handle %d alone" % k)
        if self.int8:
            # what ran: the family every layer of the plain forward reports against predict() under the calibrated exponents (a
            # layer whose epilogue needs 64 bits leaves its ring), and the fewest work items of a RING / GENERIC8 launch
            narrow = T.narrow_of(self.arch, self.ql, *self.exps)
            wide = {i for i, ok in enumerate(narrow) if not ok}
            fused = self.arch in S.SMALL
            bad, reached = PT._route_findings(net0, self.ql, S.predict_row(self.tag, wide, fused, B), narrow, "plain forward")
            self.findings += bad
            _REACHED[self.tag] = reached
            self.fewest = min(S.work_items(self.tag, wide, fused, B), key=lambda v: v[0])
            print("net_shared %s: %d layers on the 64-bit epilogue; fewest work items of a RING / GENERIC8 launch: %d x B = %d (%s %s, layer %d)" % (
                self.tag, len(wide), self.fewest[0], self.fewest[0] * B, self.fewest[1], self.fewest[2], self.fewest[3]))
        if not self.int8:
            _ROUTES[self.tag] = dict(plain=set(self.plain_families), tap=set(self.tap_families))

    # ---- shared rounds
    def actors(self, which=None, launch=None, ref=None):
        """launch(net, buf): the forward an actor issues (default: forward_device of the full batch)"""
        out = []
        for k in (range(self.n) if which is None else which):
            net = self.nets[k]
            fn = (lambda buf, net=net: net.forward_device(self.x, 0, buf)) if launch is None else (lambda buf, net=net: launch(net, buf))
            out.append(Actor("%s %s" % (self.tag, k), self.streams[k], fn, ref or self.ref, lambda k=k: self.pred(k),
                             (lambda net=net: net.counters()) if self.int8 else None, self.bufs))
        return out

    def describe(self):
        return "%s: %s %s %dx%d, %d handles, B = max_batch = %d, P = %d, conf %.6g (%d detections in ref), families plain %s tap %s" % (
            self.tag, self.arch, self.dtype, self.size[0], self.size[1], self.n, self.B, self.P, self.conf, self.detections,
            sorted(set(self.plain_families)), sorted(set(self.tap_families)))


def open_set(tag, keep=()):
    """the open handles of a case; the handles of every case not in `keep` are closed first (DarkNet handles at max_batch 64
    hold gigabytes each)"""
    if tag not in _SETS:
        for other in [t for t in _SETS if t not in keep]:
            _SETS.pop(other).close()
        torch.cuda.empty_cache()
        _SETS[tag] = HandleSet(tag)
        print("net_shared", _SETS[tag].describe(), "opened and anchored in %.2f s" % _SETS[tag].wall["open + anchor"])
    return _SETS[tag]


def _anchor_and_share(tag):
    """the stand-alone anchor found nothing unequal (HandleSet._anchor), then the shared rounds of the plain forward"""
    s = open_set(tag, keep=("tiny_i8", "slim_bf16") if S.case(tag)[1] in S.SMALL else ())
    assert not s.findings, "%s: the stand-alone anchor:\n%s" % (tag, "\n".join(s.findings[:40]))
    shared_rounds(s.actors(), s.rounds, "%s shared" % tag)


def _throughput(tag):
    """Y355_NET_OPT_WORKGROUPS on every handle, 128 and then 192 workgroups: the same ref, the same assertions, half the rounds"""
    from yolo355 import _ffi
    s = open_set(tag, keep=("tiny_i8", "slim_bf16"))
    try:
        for wgs in S.THROUGHPUT_WGS:
            for net in s.nets:
                net.set_option(_ffi.NET_OPT_WORKGROUPS, wgs)
            shared_rounds(s.actors(), s.rounds // 2, "%s workgroups %d" % (tag, wgs))
    finally:
        for net in s.nets:
            net.set_option(_ffi.NET_OPT_WORKGROUPS, 0)


def _calibration(tag, rounds=4):
    """handle 0 takes two calibration steps (freeze = False, 2 images) while the other handles run shared forward rounds: the
    steps equal net_calib_ref.step bit for bit (exponents, tracker state, maxima: test_net_calibration._same_state), the
    forwards still equal ref, and handle 0, given its exponents and trackers back, reproduces ref"""
    from test_net_calibration import _same_state
    s = open_set(tag, keep=("tiny_i8", "slim_bf16"))
    net0 = s.nets[0]
    predc = T.predc_of(s.arch, s.classes)
    tr = [R.Tracker() for _ in range(len(R.graph(s.arch).C) + 1)]
    r = R.step(s.arch, s.base, s.ql, tr, True, predc=predc)
    assert (r["sa_in"], r["sa"]) == tuple(s.exps), "the anchor's own calibration step differs from the restatement"
    xs, want = [], []
    for seed in (510, 520):
        x = T.images_of(seed, 2, s.size)
        r = R.step(s.arch, x, s.ql, tr, False, predc=predc)
        r.pop("t")
        xs.append(torch.from_numpy(x).to(s.dev))
        want.append((copy.deepcopy(tr), r))
    steps = {1: 0, 2: 1}                                         # round -> step
    bad = []

    def side(it):
        if it not in steps:
            return []
        k = steps[it]
        with torch.cuda.stream(s.streams[0]):
            e0, e1 = _event(), _event()
            e0.record()
            got = net0.calibrate(xs[k], freeze=False)
            e1.record()
        trk, rk = want[k]
        if got != (rk["sa_in"], rk["sa"]):
            bad.append("step %d: exponents %s, restatement %s" % (k, got, (rk["sa_in"], rk["sa"])))
        try:
            _same_state(net0, trk, rk)
        except AssertionError as e:
            bad.append("step %d: tracker state or maxima: %s" % (k, str(e)[:400]))
        return [(-1, e0, e1)]

    try:
        shared_rounds(s.actors(range(1, s.n)), rounds, "%s calibration beside forwards" % tag, side=side)
        assert not bad, "\n".join(bad)
    finally:
        net0.trackers = s.saved_trackers
        net0.set_act_exponents(*s.exps)
    back = s.same(s.alone(0, s.x), s.ref, "handle 0 on its exponents again")
    assert not back, "\n".join(back)


def _frames(tag):
    """the shared rounds through forward_frames_device on one periodic uint8 batch of 480 x 640 frames, every handle on its own
    resize stage; ref is handle 0's stand-alone frames result, which first must equal forward on
    normalize_frames(resize_linear_u8(frames)) (the comparison of test_net_frames._check_pair: outputs, maps, clamp count)"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import _ffi, synth
    s = open_set(tag, keep=("tiny_i8", "slim_bf16"))
    fb = synth.make_frames_u8(31, s.P, S.FRAME_SIZE[0], S.FRAME_SIZE[1], "blocks")
    frames = S.periodic(torch.from_numpy(fb).to(s.dev), s.B).contiguous()
    xb = torch.from_numpy(synth.normalize_frames(resize_linear_u8(fb, s.size[0], s.size[1]))).to(s.dev)
    x = S.periodic(xb, s.B).contiguous()
    net0 = s.nets[0]
    n_found = len(s.findings)
    try:
        with torch.cuda.stream(s.streams[0]):
            net0.forward_device(xb, _ffi.F_TAP)
        torch.cuda.synchronize()
        conf = _pick_conf(net0.candidates(s.P)[1])
        net0.overflow()                                        # (clears the flag: the tap forward ran on the other images' threshold)
        for net in s.nets:
            net.set_thresholds(conf, 0.5)
        run = lambda net, buf: net.forward_frames_device(frames, 0, buf)
        ref = s.alone(0, frames, lambda buf: run(net0, buf))
        assert int(ref["out"][3].sum()) > 0
        bad = s.same(s.alone(0, x), ref, "forward on the normalised resized frames")
        for k in range(1, s.n):
            bad += s.same(s.alone(k, frames, lambda buf, k=k: run(s.nets[k], buf)), ref, "handle %d alone on the frames" % k)
        assert not bad and len(s.findings) == n_found, "\n".join(bad + s.findings[n_found:])
        shared_rounds(s.actors(launch=run, ref=ref), s.rounds, "%s frames route" % tag)
    finally:
        del s.findings[n_found:]
        for net in s.nets:
            net.set_thresholds(s.conf, 0.5)


def _unlike(tag=None):
    """three different handles on three streams, 40 rounds: the int8 YOLOv3tiny Net (B = 128), the bf16 SlimYOLOv2 Net (B = 64)
    and the int8 SlimYOLOv2 Engine (B = 64, 416 x 416, as test_gpu_parity.test_two_engines_concurrent sets it up), each against
    its own stand-alone result: kernels with different LDS and register footprints share compute units, which three copies
    of one net never show"""
    from oracle import yolo_oracle as O
    from yolo355 import prep, synth
    from yolo355.engine import Engine
    a = open_set("tiny_i8", keep=("tiny_i8", "slim_bf16"))
    b = open_set("slim_bf16", keep=("tiny_i8", "slim_bf16"))
    assert not a.findings and not b.findings, "\n".join(a.findings + b.findings)
    B = 64
    st = torch.cuda.Stream(device=a.dev)
    with torch.cuda.stream(st):
        eng = Engine([416, 416], 2, synth.ANCHOR_SIZE_MASK, max_batch=B, device=a.dev)
        eng.load_quantized(O.quantize_layers(synth.make_weights(seed=2, num_classes=2)))
        eng.set_act_exponents(eng.calibrate(synth.make_images(1, 1, 416, 416), [prep.RangeTracker() for _ in range(11)]))
    try:
        x = S.periodic(torch.from_numpy(synth.make_images(1000, 2, 416, 416)).to(a.dev), B).contiguous()
        bufs = lambda: tuple(torch.zeros_like(t) for t in eng._buffers(B))
        torch.cuda.synchronize()
        out = bufs()
        with torch.cuda.stream(st):
            eng.forward_device(x, 0, out)
        torch.cuda.synchronize()
        ref = dict(out=list(out), pred=[eng.get_feature(9, B).copy()], ctr=None)
        assert int(out[3].sum()) > 0
        actors = a.actors([0]) + b.actors([0]) + [Actor("engine", st, lambda buf: eng.forward_device(x, 0, buf), ref,
                                                       lambda: [eng.get_feature(9, B)], None, bufs)]
        shared_rounds(actors, 40, "unlike neighbours")
    finally:
        torch.cuda.synchronize()
        eng.close()


# the order keeps a case's variants behind it (its handles are open) and the two small sets open for the unlike neighbours
PLAN = [("tiny_i8", "shared"), ("tiny_i8", "workgroups"), ("tiny_i8", "calibration"), ("tiny_i8", "frames"),
        ("slim_bf16", "shared"), ("slim_bf16", "workgroups"), ("slim_bf16", "frames"), ("tiny_slim_engine", "unlike"),
        ("slim_i8", "shared"), ("slim_i8_c2", "shared"), ("tiny_bf16", "shared"),
        ("v2_i8", "shared"), ("v2_i8", "calibration"), ("v2_bf16", "shared"),
        ("v3_i8", "shared"), ("v3_i8", "workgroups"), ("v3_bf16", "shared"), ("spp_i8", "shared")]
_RUN = {"shared": _anchor_and_share, "workgroups": _throughput, "calibration": _calibration, "frames": _frames, "unlike": _unlike}


def test_plan_holds_every_case_and_variant():
    assert [t for t, v in PLAN if v == "shared"] == S.TAGS
    for variant, tags in (("workgroups", S.THROUGHPUT), ("calibration", S.CALIBRATION), ("frames", S.FRAMES)):
        assert sorted(t for t, v in PLAN if v == variant) == sorted(tags), variant
    assert sum(1 for _, v in PLAN if v == "unlike") == 1


@pytest.mark.gpu
@pytest.mark.parametrize("tag,variant", PLAN, ids=["%s-%s" % p for p in PLAN])
def test_handles_sharing_the_gpu_reproduce_their_stand_alone_results(tag, variant):
    """the docstrings of _anchor_and_share, _throughput, _calibration, _frames and _unlike say what each variant asserts.  The
    DarkNet rows: 2 handles x 2 buffers x 12 rounds of B = 64 (48 where the handles did not fit: HandleSet._create; the line a
    set prints when it opens says which)"""
    _RUN[variant](tag)


@pytest.mark.gpu
def test_bf16_rows_reach_every_conv_family():
    """through y355_net_layer_route: the plain forwards that ran shared reach every family of bf16_layer_ref.CONV_FAMILIES but
    FIRST, which no plain forward of these graphs takes (the fused front end replaces it in slim and tiny, the DarkNet graphs
    start with the input op and a generic convolution); FIRST is what the stand-alone tap forward of slim and tiny reports"""
    import bf16_layer_ref as L
    for tag in S.BF16_TAGS:
        if tag not in _ROUTES:
            open_set(tag)
    plain = set().union(*[_ROUTES[t]["plain"] for t in S.BF16_TAGS])
    tap = set().union(*[_ROUTES[t]["tap"] for t in S.BF16_TAGS])
    print("net_shared bf16 families: plain (shared)", sorted(plain), "tap (stand-alone)", sorted(tap))
    assert set(L.CONV_FAMILIES) - {"FIRST"} <= plain, sorted(set(L.CONV_FAMILIES) - plain)
    assert "FIRST" in tap and "FIRST" not in plain


@pytest.mark.gpu
def test_int8_rows_ran_every_ring_shared():
    """what the CPU test requires of predict() on narrow epilogues, on what the plain forwards reported under the calibrated
    exponents (layer by layer equal to predict()'s, or the anchor has a finding): every ring I0 .. I5 ran beside another handle"""
    for tag in S.INT8_TAGS:
        if tag not in _REACHED:
            open_set(tag)
    reached = set().union(*[_REACHED[t] for t in S.INT8_TAGS])
    print("net_shared int8 routes that ran shared (family, tile or ring, residual):", sorted(reached, key=str))
    rings = {t for f, t, _ in reached if f == T.RING}
    assert rings == {r[0] for r in T.RINGS}, sorted(rings)
    assert {(f, t) for f, t, _ in reached if f == T.GENERIC8} >= {(T.GENERIC8, k) for k in (4, 5)}


@pytest.mark.gpu
def test_close_the_handles():
    """(the last test of the module: nothing stays allocated for the modules that run after it)"""
    for tag in list(_SETS):
        _SETS.pop(tag).close()
    torch.cuda.empty_cache()
