"""uint8 camera frames as the first input of the y355_net families (y355_net_forward_u8 / Net.forward_frames /
_NetModel.forward_frames) and the GPU rescale of their boxes (y355_net_scale_boxes, forward_batch(sizes_wh=...)).
The frames route must equal, bit for bit, y355_net_forward on synth.normalize_frames(resize_linear_u8(frames)): every tensor
of a tap forward, the int8 clamp count and the detections."""
import ctypes as C

import numpy as np
import pytest

from cases import synth_state_dict

SIZE = [224, 320]
B = 2
# (arch, module, class, anchors attribute of synth)
ARCHS = [("slim_yolo_v2", "slim_yolo_v2", "SlimYOLOv2", "ANCHOR_SIZE"),
         ("tiny_yolo_v3", "tiny_yolo_v3", "YOLOv3tiny", "TINY_MULTI_ANCHOR_SIZE"),
         ("yolo_v2", "yolo_v2", "myYOLOv2", "ANCHOR_SIZE"),
         ("yolo_v3", "yolo_v3", "myYOLOv3", "MULTI_ANCHOR_SIZE"),
         ("yolo_v3_spp", "yolo_v3", "myYOLOv3Spp", "MULTI_ANCHOR_SIZE")]
ARCH_IDS = [a[0] for a in ARCHS]


def _model(arch, device="cpu", seed=5, conf=0.02):
    import importlib
    from yolo355 import synth
    spec = dict((a[0], a[1:]) for a in ARCHS)[arch]
    mod = importlib.import_module("yolo355.models." + spec[0])
    anchors = getattr(synth, spec[2])
    m = getattr(mod, spec[1])(device, input_size=SIZE, num_classes=3, trainable=False, conf_thresh=conf, nms_thresh=0.5,
                              anchor_size=anchors)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed, weight_gain=2.0))
    m.eval()
    return m


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_ffi_declare_the_frame_entry_points():
    from yolo355 import _ffi
    names = ("y355_net_set_normalization", "y355_net_forward_u8", "y355_net_resize_u8", "y355_net_scale_boxes")
    declared = _ffi.declared_symbols()
    for n in names:
        assert n in declared and n in _ffi._SIGS, n


def test_frame_entry_points_reject_null_arguments_without_hip():
    """argument checks come first: a NULL handle or NULL frames is Y355_EINVAL with a message, no HIP call is made"""
    from yolo355 import _ffi
    lib = _ffi.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    calls = [
        lambda h, f: lib.y355_net_set_normalization(h, buf, buf),
        lambda h, f: lib.y355_net_forward_u8(h, f, 224, 320, 1, 0, p, p, p, p),
        lambda h, f: lib.y355_net_resize_u8(h, f, 480, 640, 1, p),
        lambda h, f: lib.y355_net_scale_boxes(h, f, p, p, 1),
    ]
    for call in calls:
        for h, f in ((None, p), (p, None)):
            if h is not None and call is calls[0]:
                continue                                   # (no frames argument; a live handle is needed past the null check)
            rc = call(h, f)
            assert rc == _ffi.EINVAL, rc
            assert lib.y355_last_error().decode()
    assert lib.y355_net_set_normalization(None, None, buf) == _ffi.EINVAL


@pytest.mark.parametrize("bad", ["float", "rank", "channels", "list"])
def test_forward_frames_validates_before_any_engine(bad):
    """float input, a wrong rank, a channel count other than 3: ValueError before an engine is created (no GPU here)"""
    import torch
    m = _model("tiny_yolo_v3")
    frames = {"float": np.zeros((1, 224, 320, 3), np.float32), "rank": np.zeros((224, 320, 3), np.uint8),
              "channels": torch.zeros((1, 224, 320, 4), dtype=torch.uint8), "list": [[0, 1, 2]]}[bad]
    with pytest.raises(ValueError):
        m.forward_frames(frames)
    assert not m.__dict__.get("_nets")


def test_forward_frames_quantized_needs_frozen_exponents():
    m = _model("yolo_v2")
    with pytest.raises(RuntimeError, match=r"forward_batch\(x, quantization=True\)"):
        m.forward_frames(np.zeros((1, 224, 320, 3), np.uint8), quantization=True)
    assert not m.__dict__.get("_nets")


def test_host_rescale_equals_one_fp32_product():
    """The evaluators' `b *= np.array([[w, h, w, h]])`: float32 boxes times integer sizes is computed in float64 and rounded
    once; a 24-bit box times an integer below 2^24 is exact in float64, so it equals one fp32 multiply (the GPU rescale)."""
    rng = np.random.default_rng(3)
    boxes = (rng.random((20000, 4)) * rng.choice([1e-3, 1.0, 7.0], (20000, 1))).astype(np.float32)
    boxes[:8] = [[0, 1, 0.5, 0.25]] * 8
    for w, h in [(500, 375), (640, 480), (1, 1), (16383, 9999), (333, 77)]:
        host = boxes.copy()
        host *= np.array([[w, h, w, h]])                   # int64 sizes (numpy upcasts to float64, casts back)
        fp32 = boxes * np.array([[w, h, w, h]], np.float32)
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), fp32.view(np.uint32)), (w, h)
        host32 = boxes.copy()
        host32 *= np.array([[np.float32(w), np.float32(h), np.float32(w), np.float32(h)]])
        assert np.array_equal(host32.view(np.uint32), fp32.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- GPU
_CACHE = {}


def _setup(arch):
    """(model, bf16 net, int8 net, frames at the network size) with the int8 exponents frozen"""
    if arch not in _CACHE:
        import torch
        from yolo355 import synth
        m = _model(arch, "cuda:0")
        frames = synth.make_frames_u8(21, B, SIZE[0], SIZE[1], "blocks")
        m.forward_batch(torch.from_numpy(synth.normalize_frames(frames)), quantization=True)
        _CACHE[arch] = (m, m._get_net(B), m._get_net(B, int8=True), frames)
    return _CACHE[arch]


def _ref_input(frames):
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    return synth.normalize_frames(resize_linear_u8(frames, SIZE[0], SIZE[1]))


def _tensors(net, tap, fused_front):
    skip = {0} if (not tap and fused_front) else set()
    return [None if t in skip else net.get_tensor(t, B) for t in range(net.num_tensors)]


def _same_dets(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        for s, t in zip(u, v):
            assert s.dtype == t.dtype and np.array_equal(s, t)


def _scramble(net):
    """overwrite every activation tensor and the net's resize buffer with what other frames make of them, so that a frames
    forward that follows is compared on what IT wrote (a pixel it missed keeps a different value)"""
    import torch
    from yolo355 import _ffi, synth
    other = synth.make_frames_u8(99, B, 480, 640, "noise")
    net.forward_frames_device(torch.from_numpy(other).cuda(), _ffi.F_TAP)           # the resize stage's buffer (slim / tiny)
    net.forward_device(torch.from_numpy(_ref_input(other)).cuda(), _ffi.F_TAP)     # every tensor, conv1's map included
    net.overflow()                                             # (clears the flag: these detections are never read)


def _check_pair(net, frames, tap, int8, fused_front, frames_dev=None):
    """the frames route, run first on a scrambled net, against the fp32 route on the normalised tensor of the resized frames;
    returns (dets, clamp count).  frames_dev: the same frames as a CUDA tensor to pass instead (e.g. a misaligned view)."""
    from yolo355 import _ffi
    _scramble(net)
    got = net.forward_frames(frames if frames_dev is None else frames_dev, tap=tap)
    gt = _tensors(net, tap, fused_front)
    gc = net.counters() if int8 else None
    if fused_front and not tap:                                # the fused front end ran: conv1's own map was not written
        with pytest.raises(_ffi.Y355Error):
            net.get_tensor(0, B)
    _scramble(net)
    want = net.forward(_ref_input(frames), tap=tap)
    wt = _tensors(net, tap, fused_front)
    wc = net.counters() if int8 else None
    _same_dets(want, got)
    for t, (a, b) in enumerate(zip(wt, gt)):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b), "tensor %d differs" % t
    assert wc == gc
    return want, wc


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCH_IDS)
@pytest.mark.parametrize("dtype", ["bf16", "int8"])
def test_frames_route_is_bit_exact(arch, dtype):
    """every arch x {bf16, int8} x {plain, tap} x {frames at the network size, 480 x 640}"""
    from yolo355 import synth
    m, fnet, qnet, frames = _setup(arch)
    net = qnet if dtype == "int8" else fnet
    big = synth.make_frames_u8(22, B, 480, 640, "blocks")
    fused_front = arch in ("slim_yolo_v2", "tiny_yolo_v3")
    ndet = 0
    for fr in (frames, big):
        for tap in (False, True):
            dets, _ = _check_pair(net, fr, tap, dtype == "int8", fused_front)
            ndet += sum(len(d[1]) for d in dets)
    assert ndet > 0


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["slim_yolo_v2", "tiny_yolo_v3", "yolo_v2"])
@pytest.mark.parametrize("dtype", ["bf16", "int8"])
def test_frames_at_a_misaligned_address(arch, dtype):
    """a CUDA view that starts at an odd byte: the slim / tiny fronts (12-byte loads) get the frames through the aligned
    resize-stage buffer, the DarkNet input op reads bytes; both bit-exact"""
    import torch
    m, fnet, qnet, frames = _setup(arch)
    net = qnet if dtype == "int8" else fnet
    flat = torch.empty(frames.size + 1, dtype=torch.uint8, device="cuda:0")
    view = flat[1:].view(frames.shape)
    view.copy_(torch.from_numpy(frames))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    for tap in (False, True):
        _check_pair(net, frames, tap, dtype == "int8", arch != "yolo_v2", frames_dev=view)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2", "slim_yolo_v2"])
def test_int8_input_clamps_are_counted_alike(arch):
    """sa_in raised until the input quantisation clamps: the same count (> 0) on both routes"""
    from yolo355 import synth
    m, fnet, qnet, frames = _setup(arch)
    sa_in, sa = m.act_exponents
    try:
        qnet.set_act_exponents(sa_in + 3, sa)
        for fr in (frames, synth.make_frames_u8(23, B, 480, 640, "blocks")):
            for tap in (False, True):
                _, c = _check_pair(qnet, fr, tap, True, arch != "yolo_v2")
                assert c > 0
    finally:
        qnet.set_act_exponents(sa_in, sa)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["slim_yolo_v2", "tiny_yolo_v3"])
def test_int8_conv1_route_when_the_front_is_ineligible(arch):
    """the first layer's bias with a finer exponent (same values) puts |t| above 2^24: the fused int8 front end is not
    eligible and a plain forward runs conv1 on its own (its map is then readable) -- also from frames"""
    from yolo355 import prep, synth
    from yolo355.utils.modules import folded_f32
    m, fnet, qnet, frames = _setup(arch)
    q = prep.quantize_folded([folded_f32(md) for md in m._conv_modules()[:1]])[0]
    sa_in = m.act_exponents[0]
    s = max(0, sa_in + q["e_w"] - q["e_b"] + 14)
    assert np.abs(q["q_b"]).max() * 2 ** s < 2 ** 31
    qb = (np.asarray(q["q_b"], np.int64) << s).astype(np.int32)
    try:
        qnet.load_layer_i8(0, q["q_w"], qb, q["e_w"], q["e_b"] + s)
        qnet.set_act_exponents(*m.act_exponents)
        for fr in (frames, synth.make_frames_u8(24, B, 480, 640, "blocks")):
            for tap in (False, True):
                _check_pair(qnet, fr, tap, True, False)
        qnet.forward_frames(frames)
        assert qnet.get_tensor(0, B).shape[0] == B            # conv1's map was written: the front end did not run
    finally:
        qnet.load_layer_i8(0, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
        qnet.set_act_exponents(*m.act_exponents)


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", [((480, 640), (416, 416)), ((375, 500), (320, 416)), ((120, 160), (240, 320)),
                                     ((96, 160), (96, 160)), ((833, 417), (416, 416))])
def test_net_resize_matches_oracle(src, dst):
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    from yolo355.netengine import Net
    net = Net("slim_yolo_v2", list(dst), 3, synth.ANCHOR_SIZE, max_batch=B, device="cuda:0")
    frames = synth.make_frames_u8(77, B, src[0], src[1], "blocks")
    got = net.resize_frames(frames).cpu().numpy()
    want = resize_linear_u8(frames, dst[0], dst[1])
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["yolo_v2", "tiny_yolo_v3", "slim_yolo_v2"])
def test_non_default_normalization(arch):
    """set_normalization (BGR order) on the frames route equals a host normalisation with the same constants"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    m, fnet, qnet, frames = _setup(arch)
    mean_bgr = np.array([0.5, 0.25, 0.125], np.float32)
    std_bgr = np.array([0.3, 0.2, 0.35], np.float32)
    big = synth.make_frames_u8(25, B, 480, 640, "blocks")
    x = resize_linear_u8(big, SIZE[0], SIZE[1]).astype(np.float32)
    x /= np.float32(255.0)
    x -= mean_bgr
    x /= std_bgr
    x = np.ascontiguousarray(np.transpose(x[..., ::-1], (0, 3, 1, 2)))
    try:
        for net in (fnet, qnet):
            net.set_normalization(mean_bgr, std_bgr)
            for tap in (False, True):
                _scramble(net)
                got = net.forward_frames(big, tap=tap)
                gt = [net.get_tensor(t, B) for t in range(net.num_tensors)] if tap else None
                _scramble(net)
                _same_dets(net.forward(x, tap=tap), got)
                if tap:
                    for t in range(net.num_tensors):
                        assert np.array_equal(net.get_tensor(t, B), gt[t]), "tensor %d differs" % t
    finally:
        for net in (fnet, qnet):
            net.set_normalization(synth.MEAN_RGB[::-1], synth.STD_RGB[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCH_IDS)
def test_model_forward_frames_matches_forward_batch(arch):
    """_NetModel.forward_frames (bf16 and int8) against forward_batch on the normalised tensor, with and without sizes_wh"""
    import torch
    from yolo355 import synth
    m, fnet, qnet, frames = _setup(arch)
    big = synth.make_frames_u8(26, B, 480, 640, "blocks")
    x = torch.from_numpy(_ref_input(big))
    wh = np.array([[640, 480], [500, 375]], np.float32)
    for q in (False, True):
        net = qnet if q else fnet
        _scramble(net)
        got = m.forward_frames(big, quantization=q)
        _scramble(net)
        _same_dets(m.forward_batch(x, quantization=q), got)
        _scramble(net)
        got = m.forward_frames(torch.from_numpy(big), quantization=q, sizes_wh=wh)
        _scramble(net)
        _same_dets(m.forward_batch(x, quantization=q, sizes_wh=wh), got)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["yolo_v3", "tiny_yolo_v3"])
def test_gpu_rescale_equals_the_host_rescale(arch):
    """forward_batch(x, sizes_wh=...) and voc_all_boxes on a _NetModel (which now take the GPU rescale) equal the reference's
    per-image host rescale bit for bit"""
    import torch
    from yolo355 import synth
    from yolo355.utils.evaluator_batch import voc_all_boxes
    m, fnet, qnet, frames = _setup(arch)
    x = torch.from_numpy(synth.normalize_frames(frames))
    sizes = [(500, 375), (333, 640)]
    for q in (False, True):
        plain = m.forward_batch(x, quantization=q)
        host = []
        for (b, s, c), (w, h) in zip(plain, sizes):
            b = b.copy()
            b *= np.array([[w, h, w, h]])
            host.append((b, s, c))
        assert sum(len(d[1]) for d in host) > 0
        _same_dets(host, m.forward_batch(x, quantization=q, sizes_wh=np.asarray(sizes, np.float32)))

    class DS:
        def __len__(self):
            return B

        def pull_item(self, i):
            return x[i], None, sizes[i][1], sizes[i][0]
    allb = voc_all_boxes(m, DS(), 3, batch_size=B)
    plain = m.forward_batch(x)
    for i, ((b, s, c), (w, h)) in enumerate(zip(plain, sizes)):
        b = b * np.array([[w, h, w, h]])
        for j in range(3):
            inds = np.where(c == j)[0]
            want = np.hstack((b[inds], s[inds][:, None])).astype(np.float32) if len(inds) else np.empty([0, 5], np.float32)
            assert np.array_equal(allb[j][i], want)
