"""Lists of camera frames of mixed sizes as the input of the y355_net families (y355_net_forward_frames /
y355_net_resize_frames / y355_net_calibrate_frames, Net.*_frame_list, _NetModel.*_frame_list): each frame has its own pointer,
size and row pitch, one ragged resize stage brings all of them to the network size.  Element i of a list call must equal
the single-frame call on frame i bit for bit: detections, every tap tensor, candidates, int8 clamp counts."""
import ctypes as C

import numpy as np
import pytest

from test_net_frames import ARCH_IDS, SIZE, _model, _same_dets

MAXB = 4
NEW = ("y355_net_forward_frames", "y355_net_resize_frames", "y355_net_calibrate_frames")


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_ffi_declare_the_frame_list_entry_points():
    from yolo355 import _ffi
    declared = _ffi.declared_symbols()
    for n in NEW:
        assert n in declared and n in _ffi._SIGS, n
    text = open(_ffi.HEADER_PATH).read()
    assert "typedef struct y355_frame {" in text and "} y355_frame;" in text
    f = _ffi.Frame
    assert [n for n, _ in f._fields_] == ["data_dev", "height", "width", "row_bytes"]
    assert (f.data_dev.offset, f.height.offset, f.width.offset, f.row_bytes.offset, C.sizeof(f)) == (0, 8, 12, 16, 24)


def test_frame_list_entry_points_reject_null_arguments_without_hip():
    """a NULL handle or a NULL array is Y355_EINVAL with a message; no HIP call is made (there is no GPU here)"""
    from yolo355 import _ffi
    lib = _ffi.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    arr = (_ffi.Frame * 1)()
    arr[0].data_dev, arr[0].height, arr[0].width = p.value, 4, 4
    sa = (C.c_int32 * 4)()
    calls = [lambda h, f: lib.y355_net_forward_frames(h, f, 1, 0, p, p, p, p),
             lambda h, f: lib.y355_net_resize_frames(h, f, 1, p),
             lambda h, f: lib.y355_net_calibrate_frames(h, f, 1, 0, 0.1, sa, sa, buf, 4)]
    for call in calls:
        assert call(None, arr) == _ffi.EINVAL
        assert lib.y355_last_error().decode()
    assert lib.y355_net_forward_frames(None, None, 1, 0, p, p, p, p) == _ffi.EINVAL
    assert lib.y355_net_resize_frames(None, None, 1, p) == _ffi.EINVAL
    assert lib.y355_net_calibrate_frames(None, None, 1, 0, 0.1, sa, sa, buf, 4) == _ffi.EINVAL


def _bad_lists():
    import torch
    return {"empty": [], "4d": np.zeros((1, 8, 8, 3), np.uint8), "float": [np.zeros((8, 8, 3), np.float32)],
            "channels": [torch.zeros((8, 8, 4), dtype=torch.uint8)], "nested": [[0, 1, 2]],
            "zero_height": [np.zeros((8, 8, 3), np.uint8), np.zeros((0, 8, 3), np.uint8)]}


@pytest.mark.parametrize("bad", ["empty", "4d", "float", "channels", "nested", "zero_height"])
@pytest.mark.parametrize("method", ["forward_frame_list", "calibrate_frame_list"])
def test_frame_list_methods_validate_before_any_engine(method, bad):
    from yolo355.netengine import Net
    m = _model("tiny_yolo_v3")
    with pytest.raises(ValueError):
        getattr(m, method)(_bad_lists()[bad])
    assert not m.__dict__.get("_nets")
    with pytest.raises(ValueError):
        Net.pack_frames(_bad_lists()[bad])


def test_forward_frame_list_quantized_needs_frozen_exponents():
    m = _model("yolo_v2")
    with pytest.raises(RuntimeError, match=r"forward_batch\(x, quantization=True\)"):
        m.forward_frame_list([np.zeros((8, 8, 3), np.uint8)], quantization=True)
    assert not m.__dict__.get("_nets")


def test_pack_frames_lays_odd_sizes_back_to_back():
    import torch
    from yolo355.netengine import Net
    frames = [_noise(1, 1, 1), torch.from_numpy(_noise(2, 3, 5)), _noise(3, 7, 1)[::-1], _noise(4, 2, 2)]
    buf, offsets, sizes = Net.pack_frames(tuple(frames))
    assert sizes == [(1, 1), (3, 5), (7, 1), (2, 2)]
    assert offsets == [0, 3, 48, 69] and buf.dtype == np.uint8 and buf.shape == (81,)
    assert [o % 4 for o in offsets] == [0, 3, 0, 1]                     # misaligned starts
    for f, o, (h, w) in zip(frames, offsets, sizes):
        assert np.array_equal(buf[o:o + h * w * 3].reshape(h, w, 3), np.asarray(f))


# ---------------------------------------------------------------------------------------------------- GPU
_CACHE = {}


def _setup(arch):
    """(model, bf16 net, int8 net), both nets with room for MAXB frames and the int8 exponents frozen"""
    if arch not in _CACHE:
        import torch
        from yolo355 import synth
        m = _model(arch, "cuda:0")
        frames = synth.make_frames_u8(21, MAXB, SIZE[0], SIZE[1], "blocks")
        m.forward_batch(torch.from_numpy(synth.normalize_frames(frames)), quantization=True)
        _CACHE[arch] = (m, m._get_net(MAXB), m._get_net(MAXB, int8=True))
    return _CACHE[arch]


def _ref_input(frames):
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    return synth.normalize_frames(resize_linear_u8(frames, SIZE[0], SIZE[1]))


def _scramble(net):
    """test_net_frames._scramble for every batch slot, the list route's resize buffer included: a list forward of other
    frames fills rs_frames and the per-frame tables, a tap forward of another input every tensor"""
    import torch
    from yolo355 import _ffi, synth
    n = net.max_batch
    net.forward_frame_list_device([_noise(900 + i, 90 + 7 * i, 130 - 11 * i) for i in range(n)], _ffi.F_TAP)
    other = synth.make_frames_u8(99, n, 120, 160, "noise")
    net.forward_frames_device(torch.from_numpy(other).cuda(), _ffi.F_TAP)
    net.forward_device(torch.from_numpy(_ref_input(other)).cuda(), _ffi.F_TAP)
    net.overflow()


def _three_frames(seed=0):
    """one frame at the network size, one smaller with odd sizes, one larger"""
    from yolo355 import synth
    return [synth.make_frames_u8(31 + seed, 1, SIZE[0], SIZE[1], "blocks")[0], synth.make_frames_u8(32 + seed, 1, 149, 211, "blocks")[0],
            synth.make_frames_u8(33 + seed, 1, 480, 640, "blocks")[0]]


def _singles(net, frames, tap, int8, fused_front):
    """what the list call must reproduce: forward_frames(frame[None]) per frame -> (dets, tensors, candidates, clamps)"""
    dets, tens, cands, clamps = [], [], [], 0
    for f in frames:
        _scramble(net)
        dets.append(net.forward_frames(f[None], tap=tap)[0])
        tens.append([None if (t == 0 and fused_front and not tap) else net.get_tensor(t, 1) for t in range(net.num_tensors)])
        if tap:
            cands.append(net.candidates(1))
        if int8:
            clamps += net.counters()
    return dets, tens, cands, clamps


def _check_list(net, frames, tap, int8, fused_front, given=None):
    """the list call, run first on a scrambled net, against the single-frame calls; given: the list to pass instead"""
    n = len(frames)
    _scramble(net)
    got = net.forward_frame_list(frames if given is None else given, tap=tap)
    gt = [None if (t == 0 and fused_front and not tap) else net.get_tensor(t, n) for t in range(net.num_tensors)]
    gcand = net.candidates(n) if tap else None
    gc = net.counters() if int8 else 0
    dets, tens, cands, clamps = _singles(net, frames, tap, int8, fused_front)
    _same_dets(dets, got)
    for i in range(n):
        for t in range(net.num_tensors):
            if gt[t] is not None:
                assert np.array_equal(gt[t][i], tens[i][t][0]), "frame %d tensor %d differs" % (i, t)
        if tap:
            for a, b in zip(gcand, cands[i]):
                assert np.array_equal(a[i], b[0]), "frame %d candidates differ" % i
    assert gc == clamps
    return got, gc


def _frame_array(ptrs_sizes):
    from yolo355 import _ffi
    arr = (_ffi.Frame * len(ptrs_sizes))()
    for i, (ptr, h, w, rb) in enumerate(ptrs_sizes):
        arr[i].data_dev, arr[i].height, arr[i].width, arr[i].row_bytes = ptr, h, w, rb
    return arr


@pytest.mark.gpu
def test_ragged_stage_equals_the_oracle_on_a_mixed_list():
    """(1,1), (1,7), (7,1), (37,53), the network size, (480,640), (2,16384), (500,375) packed without padding"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    from yolo355.netengine import Net
    sizes = [(1, 1), (1, 7), (7, 1), (37, 53), tuple(SIZE), (480, 640), (2, 16384), (500, 375)]
    frames = [_noise(40 + i, h, w) for i, (h, w) in enumerate(sizes)]
    _, offsets, _ = Net.pack_frames(frames)
    assert len({o % 4 for o in offsets}) > 2                            # several misaligned starts
    net = Net("slim_yolo_v2", SIZE, 3, synth.ANCHOR_SIZE, max_batch=8, device="cuda:0")
    net.resize_frame_list([_noise(60 + i, 50 + i, 70 - i) for i in range(8)])       # other tables first
    got = net.resize_frame_list(frames).cpu().numpy()
    for i, f in enumerate(frames):
        want = resize_linear_u8(f, SIZE[0], SIZE[1])
        assert np.array_equal(got[i], want), (sizes[i], int((got[i] != want).sum()))
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dst", [SIZE, [64, 96]], ids=["224x320", "64x96"])
def test_device_built_tables_over_a_sweep_of_ratios(dst):
    """one-row frames (1, w) and one-column frames (h, 1) over ~80 sizes from 1 to 2000: every table ratio of either axis"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    from yolo355.netengine import Net
    ns = sorted(set(list(range(1, 12)) + [int(round(v)) for v in np.geomspace(12, 2000, 62)]
                    + [dst[0] - 1, dst[0], dst[0] + 1, dst[1] - 1, dst[1], dst[1] + 1, 2 * dst[0], 2 * dst[1]]))
    assert 75 <= len(ns) <= 85 and ns[0] == 1 and ns[-1] == 2000
    net = Net("slim_yolo_v2", dst, 3, synth.ANCHOR_SIZE, max_batch=8, device="cuda:0")
    for axis in (0, 1):
        for k in range(0, len(ns), 8):
            frames = [_noise(n, 1, n) if axis else _noise(n, n, 1) for n in ns[k:k + 8]]
            got = net.resize_frame_list(frames).cpu().numpy()
            for i, f in enumerate(frames):
                want = resize_linear_u8(f, dst[0], dst[1])
                assert np.array_equal(got[i], want), (f.shape, int((got[i] != want).sum()))
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCH_IDS)
@pytest.mark.parametrize("dtype", ["bf16", "int8"])
def test_list_forward_is_bit_exact(arch, dtype):
    """every arch x {bf16, int8} x {plain, tap}: three frames of three sizes against three single-frame calls"""
    m, fnet, qnet = _setup(arch)
    net = qnet if dtype == "int8" else fnet
    frames = _three_frames()
    ndet = 0
    for tap in (False, True):
        dets, _ = _check_list(net, frames, tap, dtype == "int8", arch in ("slim_yolo_v2", "tiny_yolo_v3"))
        ndet += sum(len(d[1]) for d in dets)
    assert ndet > 0


@pytest.mark.gpu
def test_int8_input_clamps_add_up():
    """sa_in raised until the input quantisation clamps: the list's count (> 0) is the sum of the single calls'"""
    m, fnet, qnet = _setup("tiny_yolo_v3")
    sa_in, sa = m.act_exponents
    try:
        qnet.set_act_exponents(sa_in + 3, sa)
        for tap in (False, True):
            _, c = _check_list(qnet, _three_frames(), tap, True, True)
            assert c > 0
    finally:
        qnet.set_act_exponents(sa_in, sa)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2"])
def test_pitched_views_and_mixed_lists(arch):
    """a CUDA crop view of a larger frame passes its pitch and gives the results of its contiguous copy; a list mixing
    numpy frames with separately allocated CUDA frames gives the results of the all-numpy list"""
    import torch
    m, fnet, qnet = _setup(arch)
    big = torch.from_numpy(_noise(70, 60, 70)).cuda()
    view = big[10:47, 5:58]
    assert not view.is_contiguous() and view.stride() == (210, 3, 1)
    crop = view.contiguous().cpu().numpy()
    a, b, c = _three_frames(3)
    frames = [a, crop, b, c]
    given = [a, view, torch.from_numpy(b).cuda(), torch.from_numpy(c)]          # numpy, pitched CUDA, CUDA, CPU torch
    fused_front = arch == "tiny_yolo_v3"
    for net in (fnet, qnet):
        got = net.resize_frame_list(given).cpu().numpy()
        assert np.array_equal(got, net.resize_frame_list(frames).cpu().numpy())
        _check_list(net, frames, True, net is qnet, fused_front, given=given)
    _scramble(fnet)
    _same_dets(fnet.forward_frame_list(frames), fnet.forward_frame_list(given))


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["slim_yolo_v2", "yolo_v3"])
def test_alternating_sizes_keep_no_stale_state(arch):
    """two lists of different sizes alternated for four rounds with nothing but launches in between (results collected at the
    end): every round equals the first; one same-size forward_frames call in the middle is what it was before"""
    import torch
    from yolo355 import synth
    m, fnet, qnet = _setup(arch)
    net = qnet
    md = net.max_det

    def bufs():
        return (torch.empty((MAXB, md, 4), dtype=torch.float32, device="cuda:0"), torch.empty((MAXB, md), dtype=torch.float32, device="cuda:0"),
                torch.empty((MAXB, md), dtype=torch.int32, device="cuda:0"), torch.zeros((MAXB,), dtype=torch.int32, device="cuda:0"))
    la = _three_frames(5)
    lb = [synth.make_frames_u8(80 + i, 1, h, w, "blocks")[0] for i, (h, w) in enumerate([(375, 500), (333, 77), (224, 321), (97, 640)])]
    same = torch.from_numpy(synth.make_frames_u8(85, 2, 240, 352, "blocks")).cuda()
    outs = [bufs() for _ in range(10)]
    net.forward_frames_device(same, 0, outs[8])
    for r in range(4):
        net.forward_frame_list_device(la, 0, outs[2 * r])
        if r == 2:
            net.forward_frames_device(same, 0, outs[9])
        net.forward_frame_list_device(lb, 0, outs[2 * r + 1])
    torch.cuda.synchronize()
    assert not net.overflow()
    res = [net._collect(2 if k >= 8 else (3 if k % 2 == 0 else 4), o) for k, o in enumerate(outs)]
    assert sum(len(d[1]) for d in res[0] + res[1]) > 0
    for r in range(1, 4):
        _same_dets(res[0], res[2 * r])
        _same_dets(res[1], res[2 * r + 1])
    _same_dets(res[8], res[9])
    _same_dets(res[0], [net.forward_frames(f[None])[0] for f in la])
    _same_dets(res[1], [net.forward_frames(f[None])[0] for f in lb])


@pytest.mark.gpu
def test_own_sizes_rescale_equals_the_host_rescale():
    m, fnet, qnet = _setup("yolo_v2")
    frames = _three_frames(7)
    plain = fnet.forward_frame_list(frames)
    assert sum(len(d[1]) for d in plain) > 0
    wh = [(f.shape[1], f.shape[0]) for f in frames]
    host = []
    for (b, s, c), (w, h) in zip(plain, wh):
        b = b.copy()
        b *= np.array([[w, h, w, h]])
        host.append((b, s, c))
    own = fnet.forward_frame_list(frames, sizes_wh="own")
    _same_dets(host, own)
    _same_dets(own, fnet.forward_frame_list(frames, sizes_wh=np.asarray(wh, np.float32)))
    with pytest.raises(ValueError):
        fnet.forward_frame_list(frames, sizes_wh="theirs")
    with pytest.raises(ValueError):
        fnet.forward_frame_list(frames + frames)                        # more than max_batch frames


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2"])
def test_calibration_on_a_list_equals_the_step_on_its_resized_frames(arch):
    """two steps of calibrate_frame_list against two steps of calibrate_frames(resize_frame_list(...)) on a second identical
    model: exponents, tracker scales and first_a, max_out; the models' state_dict buffers follow"""
    ma, mb = _model(arch, "cuda:0", seed=6), _model(arch, "cuda:0", seed=6)
    na, nb = ma._get_net(MAXB, int8=True), mb._get_net(MAXB, int8=True)
    lists = [_three_frames(11), [_noise(91, 375, 500), _noise(92, 51, 33), _three_frames(12)[2], _noise(93, 224, 320)]]
    for k, frames in enumerate(lists):
        ea = ma.calibrate_frame_list(frames, freeze=(k == 0))
        eb = mb.calibrate_frames(nb.resize_frame_list(frames), freeze=(k == 0))
        assert ma._get_net(MAXB, int8=True) is na and mb._get_net(MAXB, int8=True) is nb
        assert ea == eb and na.get_act_exponents() == nb.get_act_exponents()
        for u, v in zip(na.trackers, nb.trackers):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
        assert (na.trackers[1] != 0).all()
        assert np.array_equal(na.last_calibration_max.view(np.uint32), nb.last_calibration_max.view(np.uint32))
        sda, sdb = ma.state_dict(), mb.state_dict()
        for key, idx in (("act_tracker_scale", 0), ("act_tracker_first_a", 1)):
            assert np.array_equal(sda[key].cpu().numpy(), sdb[key].cpu().numpy())
            assert np.array_equal(sda[key].cpu().numpy(), na.trackers[idx])
    _same_dets(ma.forward_frame_list(lists[0], quantization=True), mb.forward_frame_list(lists[0], quantization=True))


@pytest.mark.gpu
def test_errors_on_a_live_handle_leave_it_usable():
    import torch
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import _ffi
    m, fnet, qnet = _setup("tiny_yolo_v3")
    lib = _ffi.lib()
    f = _noise(95, 37, 53)
    want = resize_linear_u8(f, SIZE[0], SIZE[1])
    fd = torch.from_numpy(f).cuda()
    out = torch.empty((MAXB + 1, SIZE[0], SIZE[1], 3), dtype=torch.uint8, device="cuda:0")
    ob, os_, oc, on = fnet._buffers(1)
    good = (fd.data_ptr(), 37, 53, 0)
    n = qnet.num_trackers
    sa, mx = (C.c_int32 * n)(), (C.c_float * n)()
    bad = {"pitch": [(fd.data_ptr(), 37, 53, 3 * 53 - 1)], "null": [good, (None, 37, 53, 0)], "wide": [(fd.data_ptr(), 1, 16385, 0)],
           "batch": [good] * (MAXB + 1)}
    for name, desc in bad.items():
        arr = _frame_array(desc)
        for net in (fnet, qnet):
            assert lib.y355_net_resize_frames(net._h, arr, len(desc), out.data_ptr()) == _ffi.EINVAL, name
            assert lib.y355_last_error().decode()
            assert lib.y355_net_forward_frames(net._h, arr, len(desc), 0, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(),
                                               on.data_ptr()) == _ffi.EINVAL, name
            assert np.array_equal(net.resize_frame_list([f]).cpu().numpy()[0], want), name
        assert lib.y355_net_calibrate_frames(qnet._h, arr, len(desc), 0, 0.1, sa, sa, mx, n) == _ffi.EINVAL, name
    arr = _frame_array([good])
    assert lib.y355_net_calibrate_frames(fnet._h, arr, 1, 0, 0.1, sa, sa, mx, n) == _ffi.EINVAL       # a bf16 net
    assert lib.y355_net_calibrate_frames(qnet._h, arr, 1, 0, 0.1, sa, sa, mx, n - 1) == _ffi.EINVAL   # a wrong n
    assert lib.y355_net_forward_frames(qnet._h, arr, 1, 0, None, os_.data_ptr(), oc.data_ptr(), on.data_ptr()) == _ffi.EINVAL
    for net in (fnet, qnet):                                            # exponents and trackers untouched: same detections
        _same_dets(net.forward_frame_list([f]), net.forward_frames(f[None]))


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCH_IDS)
def test_model_forward_frame_list_matches_forward_batch(arch):
    """_NetModel.forward_frame_list (bf16 and int8) against forward_batch on normalize_frames(resize_linear_u8(frame))"""
    import torch
    m, fnet, qnet = _setup(arch)
    frames = _three_frames(15)
    for q in (False, True):
        net = qnet if q else fnet
        _scramble(net)
        got = m.forward_frame_list(frames, quantization=q)
        want = []
        for f in frames:
            _scramble(net)
            want.append(m.forward_batch(torch.from_numpy(_ref_input(f[None])), quantization=q)[0])
        _same_dets(want, got)
    assert sum(len(d[1]) for d in got) > 0
