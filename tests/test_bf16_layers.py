"""GPU: every op of the bf16 form of the five y355_net graphs, per element, against the layer-local float64 reference of
tests/bf16_layer_ref.py (its docstring holds the rounding contract and the derivation of the bounds).

Per case (bf16_layer_ref.CASES: slim 320x416 B1 / 96x160 B2, tiny 416 B1 / 224x320 B2, yolo_v2 416 B1 / 224x320 B2, yolo_v3
224x320 B2 / 416 B1, yolo_v3_spp 416 B1; weights of the existing generators, noise images.  yolo_v3 at 416 is there because at
224 x 320 sixteen of DarkNet-53's stride-32 layers run the four-wave kernel where a 416 x 416 net runs the eight-wave one):
  tap       a tap forward, the checker over every op;
  plain     a forward without the tap, the checker over every op from the third on (the same kernels; for slim and tiny behind the
            fused front end, whose output -- tensor 1 -- is checked from the network input through both layers, and whose tensor 0 must
            answer Y355_ENOTREADY);
  ring      slim only: a tap forward with Y355_NET_OPT_THIN_RESIDENT = 0 (the thin layers on the ring kernels);
  wg7       the first case of every graph: a plain forward with Y355_NET_OPT_WORKGROUPS = 7 (the persistent walk with fewer
            workgroups than work items).
Coverage: the route family y355_net_layer_route reports for every layer of a 416 x 416 net must have been reached by a checked run
of that graph in that layer, and all six families must have been checked.  The tile id inside a family is not visible through
the ABI: which instantiation of a family ran is known only from the sizes chosen (maps of 13 x 13 and more take the production
tiles).

Two bounds.  Tier 1: no element outside its interval -- the derived bound, no measured number in it.  Tier 2: rho, the distance of
the float64 value to the rounding cell of the engine's value in units of 2^-24 S, at most FACTOR = 4 times the largest value
measured for the route family (the factor because rho depends on the data and on the accumulation order of a tile).  Measured
on an MI355X against the float64 reference, never against another route (profiles/bf16_layer_check.md has every case, run and
family, the 99.9th percentiles and the shares of exactly rounded elements): largest rho FIRST 0.77, FRONT 0.00, RING 1.96,
THIN 0.46, GENERIC4 1.91, GENERIC8 1.99; 99.9th percentiles at most 1.4; 99 % and more of the bf16 elements are the exactly
rounded float64 value.  The bound's 2 K is 56 (first layer) to 23042 (K = 1280 x 9 + 1): no family comes anywhere near it, the
kernels' sums behave like a handful of roundings of S.  The largest values belong to the fp32 prediction maps, whose rho counts
the final fp32 rounding of the value itself.  FRONT measures 0: the growth term conv(u1, |W2b|) of the two-layer check is
subtracted before rho is taken and covers every element that is not the exactly rounded value, so tier 2 asks of the fused front
end that no element needs more than that term.
"""
import numpy as np
import pytest
import torch

import bf16_layer_ref as L

torch.set_num_threads(min(16, torch.get_num_threads()))

FACTOR = 4.0
# largest rho per route family over all cases and runs (profiles/bf16_layer_check.md), rounded up to two decimals
RHO_MEASURED = {"FIRST": 0.77, "FRONT": 0.0, "RING": 1.96, "THIN": 0.46, "GENERIC4": 1.91, "GENERIC8": 1.99}
IDS = [c[0] for c in L.CASES]
_RUNS = {}
_CACHE = {}


def _net(arch, size, B):
    from yolo355.netengine import Net
    m = L.model_of(arch)
    net = Net(arch, size, m["classes"], m["anchors"], 0.05, 0.5, max_batch=B, device="cuda:0", dtype="bf16")
    for i, (w, b) in enumerate(m["weights"]):
        net.load_layer(i, w, b)
    return net


def _forward(net, x, tap):
    from yolo355 import _ffi
    net.forward_device(net._dev_input(x), _ffi.F_TAP if tap else 0)
    net.sync()
    return [net.layer_route(i) for i in range(net.num_layers)]


def _tensors(net, B, skip0=False):
    return [None if (skip0 and t == 0) else net.get_tensor(t, B) for t in range(net.num_tensors)]


def run_case(tag):
    """the checked runs of a case, once: dict(reports [(run, report)], routes {run: [family per layer]})"""
    if tag in _RUNS:
        return _RUNS[tag]
    from yolo355 import _ffi
    _, arch, size, B = next(c for c in L.CASES if c[0] == tag)
    m = L.model_of(arch)
    W = m["weights"]
    x = L.images_of(arch, size, B)
    front = arch in ("slim_yolo_v2", "tiny_yolo_v3")
    g = L.GRAPHS[arch]()
    later = set(range(2, len(g.ops)))
    net = _net(arch, size, B)
    out = dict(reports=[], routes={})

    def checked(run, tap):
        routes = _forward(net, x, tap)
        out["routes"][run] = [L.FAMILY.get(r & 0xff, "?") for r in routes]
        if not tap and front:                             # the fused launch does not write conv1's own map
            with pytest.raises(_ffi.Y355Error) as ei:
                net.get_tensor(0, B)
            assert ei.value.code == _ffi.ENOTREADY
        T = _tensors(net, B, skip0=not tap and front)
        reps = L.check_graph(arch, x, W, T, routes, None if tap else later, _CACHE)
        if not tap and front:
            assert out["routes"][run][:2] == ["FRONT", "FRONT"]
            reps.insert(0, L.check_front(arch, x, W, T[1]))
        out["reports"] += [(run, r) for r in reps]

    try:
        checked("tap", True)
        checked("plain", False)
        if arch == "slim_yolo_v2":
            net.set_option(_ffi.NET_OPT_THIN_RESIDENT, 0)
            checked("ring", True)
            net.set_option(_ffi.NET_OPT_THIN_RESIDENT, 1)
        if tag == next(c[0] for c in L.CASES if c[1] == arch):
            net.set_option(_ffi.NET_OPT_WORKGROUPS, 7)
            checked("wg7", False)
    finally:
        net.close()
    _RUNS[tag] = out
    return out


def family_figures(reports):
    """{(run, family): (largest rho, largest 99.9th percentile, share of exactly rounded elements, elements)}"""
    fig = {}
    for run, r in reports:
        k = (run, r["family"])
        a = fig.get(k, (0.0, 0.0, 0.0, 0))
        fig[k] = (max(a[0], r["rho_max"]), max(a[1], r["rho_999"]), a[2] + r["exact"] * r["n"], a[3] + r["n"])
    return {k: (a[0], a[1], a[2] / a[3], a[3]) for k, a in fig.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", IDS)
def test_every_element_inside_its_interval(tag):
    """tier 1: the derived bound of every op, tap and plain forwards and the options of the module docstring"""
    res = run_case(tag)
    for (run, fam), (rmax, r999, exact, n) in sorted(family_figures(res["reports"]).items()):
        print("%s %-5s %-9s rho max %8.2f  99.9 %% %7.2f  exactly rounded %.4f of %d" % (tag, run, fam, rmax, r999, exact, n))
    for run in res["routes"]:
        bad = [r for rr, r in res["reports"] if rr == run]
        assert not L.describe(bad), "%s, %s forward:\n%s" % (tag, run, L.describe(bad))
    assert {"tap", "plain"} <= set(res["routes"])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", IDS)
def test_rho_within_four_times_the_measured(tag):
    """tier 2: rho of every convolution at most FACTOR times the largest value measured for its route family"""
    res = run_case(tag)
    over = []
    for run, r in res["reports"]:
        if r["kind"] != "conv":
            continue
        assert r["family"] in RHO_MEASURED, (r["name"], r["family"])
        if r["rho_max"] > FACTOR * RHO_MEASURED[r["family"]]:
            over.append("%s forward, %s on %s: rho %.2f > %g x %.2f" % (run, r["name"], r["family"], r["rho_max"], FACTOR, RHO_MEASURED[r["family"]]))
    assert not over, "%s:\n%s" % (tag, "\n".join(over))


def routes_at_416(arch):
    net = _net(arch, [416, 416], 1)
    try:
        routes = _forward(net, L.images_of(arch, [416, 416], 1), False)
    finally:
        net.close()
    return [L.FAMILY.get(r & 0xff, "?") for r in routes]


@pytest.mark.gpu
@pytest.mark.parametrize("arch", L.ARCHS)
def test_routes_of_a_416_net_were_checked(arch):
    """layer by layer, the family a 416 x 416 net runs is among those the checked runs of the graph reached in that layer"""
    want = routes_at_416(arch)
    reached = [set() for _ in want]
    for tag in [c[0] for c in L.CASES if c[1] == arch]:
        for fams in run_case(tag)["routes"].values():
            for i, f in enumerate(fams):
                reached[i].add(f)
    print(arch, "416 x 416:", " ".join(want))
    print(arch, "checked:  ", " ".join("/".join(sorted(s)) for s in reached))
    missing = [(i, f) for i, f in enumerate(want) if f not in reached[i]]
    assert not missing, "%s: (layer, family) of the 416 x 416 net that no checked run reached: %s" % (arch, missing)


@pytest.mark.gpu
def test_every_route_family_was_checked():
    seen = set()
    for tag in IDS:
        seen |= {r["family"] for _, r in run_case(tag)["reports"] if r["kind"] == "conv"}
    assert set(L.CONV_FAMILIES) <= seen, sorted(set(L.CONV_FAMILIES) - seen)
