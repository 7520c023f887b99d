"""yolo355.augment on the GPU: the kernel's batch equals the reference's images (tests/golden/augment.npz) and tests/augment_ref.py's
restatement BIT FOR BIT -- every operation on both sides is one correctly rounded fp32 operation in one stated order, so there is
no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_ref as R
from yolo355 import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return AC.load_golden()


@pytest.fixture(scope="module")
def drawn(gold):
    """per golden sample: (tag, frame, target, size, AugParams of its seed)"""
    out = []
    for tag, shape, seed, si in AC.samples(gold):
        frame, tgt = AC.frame(shape, seed), AC.target(shape, seed)
        p, _, _ = A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4], rng=np.random.RandomState(seed))
        out.append((tag, frame, tgt, AC.SIZES[si], p, seed))
    return out


def same(got, want, what=""):
    """equal as bits, over finite values (the same positions are non-finite)"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = fin & (g != w)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r want %r" % (what, bad.sum(), bad.size, i, got[i], want[i]))


def run(frames, params, size, **kw):
    return A.apply(frames, params, size, mean=AC.MEAN, std=AC.STD, **kw)


def test_apply_equals_the_reference_images(gold, drawn):
    for tag, frame, _, size, p, _ in drawn:
        x = run([frame], [p], size, to_rgb=False)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (1, 3) + size
        same(x[0].permute(1, 2, 0).contiguous(), gold[tag + "/image"], tag)
        same(run([frame], [p], size)[0], np.ascontiguousarray(gold[tag + "/image"][:, :, ::-1].transpose(2, 0, 1)), tag + " rgb")


def test_the_batch_equals_each_sample_alone_at_two_sizes_in_succession(drawn):
    for size in AC.SIZES + AC.SIZES[:1]:
        frames, params = [d[1] for d in drawn], [d[4] for d in drawn]
        x = run(frames, params, size)
        same(x, R.batch(frames, params, size, AC.MEAN, AC.STD), "batch %s" % (size,))
        for i in range(len(frames)):
            same(run(frames[i:i + 1], params[i:i + 1], size)[0], x[i].cpu().numpy(), "alone %d" % i)


def test_mixed_frame_kinds_equal_the_numpy_list(drawn):
    frames, params = [d[1] for d in drawn], [d[4] for d in drawn]
    size = AC.SIZES[0]
    want = run(frames, params, size).cpu().numpy()
    mixed = []
    for i, f in enumerate(frames):
        if i % 4 == 1:
            mixed.append(torch.from_numpy(f.copy()))
        elif i % 4 == 2:
            mixed.append(torch.from_numpy(f.copy()).to(DEV))
        elif i % 4 == 3:                                                    # a row-pitched view of a wider CUDA image, odd offset
            wide = torch.full((f.shape[0], f.shape[1] + 5, 3), 201, dtype=torch.uint8, device=DEV)
            wide[:, 3:3 + f.shape[1]] = torch.from_numpy(f.copy()).to(DEV)
            v = wide[:, 3:3 + f.shape[1]]
            assert not v.is_contiguous() or f.shape[0] == 1
            mixed.append(v)
        else:
            mixed.append(f)
    assert sum(isinstance(m, torch.Tensor) and m.is_cuda for m in mixed) >= 2
    same(run(mixed, params, size), want, "mixed list")


def test_more_frames_than_one_chunk_and_a_width_that_is_no_multiple_of_four():
    n = A.chunk() + 3
    rs = np.random.RandomState(11)
    frames, params = [], []
    for i in range(n):
        shape = 3 if i % 3 == 0 else 2                                      # 1x1 and 5x7 frames
        f, t = AC.frame(shape, i), AC.target(shape, i)
        p, _, _ = A.draw(f.shape[0], f.shape[1], t[:, :4], t[:, 4], rng=rs)
        frames.append(f)
        params.append(p)
    for size in ((6, 7), (5, 8)):                                           # scalar stores; 16-byte stores
        same(run(frames, params, size), R.batch(frames, params, size, AC.MEAN, AC.STD), "chunks %s" % (size,))


def test_out_is_written_in_place_whatever_its_alignment(drawn):
    frames, params = [d[1] for d in drawn], [d[4] for d in drawn]
    size, B = AC.SIZES[1], len(drawn)
    want = R.batch(frames, params, size, AC.MEAN, AC.STD)
    out = torch.zeros((B, 3) + size, dtype=torch.float32, device=DEV)
    x = run(frames, params, size, out=out)
    assert x is out
    same(out, want, "out")
    n = out.numel()
    buf = torch.full((n + 2,), 7.0, dtype=torch.float32, device=DEV)
    off = buf[1:1 + n].view((B, 3) + size)                                  # 4 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 4 and run(frames, params, size, out=off) is off
    same(off, want, "misaligned out")
    assert buf[0].item() == 7.0 and buf[-1].item() == 7.0
    for bad in (torch.zeros((B, 3, size[1], size[0]), dtype=torch.float32, device=DEV), torch.zeros((B, 3) + size, dtype=torch.float64, device=DEV),
                torch.zeros((B, 3) + size, dtype=torch.float32), out[:, :, :, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            run(frames, params, size, out=bad)


def test_on_another_stream(drawn):
    frames, params = [d[1] for d in drawn], [d[4] for d in drawn]
    want = R.batch(frames, params, AC.SIZES[0], AC.MEAN, AC.STD)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        x = run(frames, params, AC.SIZES[0])
        y = x.clone()
    s.synchronize()
    same(y, want, "side stream")


def test_identity_parameters():
    f = AC.frame(0, 1)
    mean, std = np.array(AC.MEAN, np.float32), np.array(AC.STD, np.float32)
    want = ((f.astype(np.float32) / np.float32(255)) - mean) / std
    x = run([f], [A.AugParams.identity(37, 53)], (37, 53), to_rgb=False)    # equal sizes: exactly the normalised frame
    same(x[0].permute(1, 2, 0).contiguous(), want, "identity")
    big = AC.frame(1, 2)                                                    # 64x48
    for size in ((32, 24), (32, 64), (64, 32), (7, 5), (100, 90)):          # exact 2x decimation (the area path), then the bilinear ones
        p = A.AugParams.identity(64, 48)
        ref = R.resize(big.astype(np.float32), (size[1], size[0]))
        ref = ((ref / np.float32(255)) - mean) / std
        same(run([big], [p], size, to_rgb=False)[0].permute(1, 2, 0).contiguous(), ref, "float resize %s" % (size,))
    # the area path with the photometric chain and a window off the frame
    p = A.AugParams(64, 48, oy=-3, ox=5, mirror=True, hsv=True, brightness=-20.5, brightness_on=True, contrast=1.4, contrast_on=True,
                    saturation=1.3, saturation_on=True, hue=17.0, hue_on=True)
    same(run([big], [p], (32, 24)), R.batch([big], [p], (32, 24), AC.MEAN, AC.STD), "area path, distorted")


def test_augment_frame_list_end_to_end_under_the_global_seed(gold, drawn):
    for tag, frame, tgt, size, p, seed in drawn:
        before = tgt.copy()
        np.random.seed(seed)
        x, tout, params = A.augment_frame_list([frame], [tgt], list(size), to_rgb=False)
        assert int(np.random.randint(1 << 30)) == int(gold[tag + "/next"][0])
        same(x[0].permute(1, 2, 0).contiguous(), gold[tag + "/image"], tag)
        assert len(tout) == 1 and tout[0].dtype == np.float64 and tout[0].tobytes() == gold[tag + "/target"].tobytes(), tag
        assert repr(params[0]) == repr(p) and np.array_equal(tgt, before)
    # a list draws in order from the one stream
    frames, targets = [d[1] for d in drawn], [d[2] for d in drawn]
    x, tout, params = A.augment_frame_list(frames, targets, AC.SIZES[0], rng=np.random.RandomState(3))
    p2, t2 = A.draw_list([f.shape[:2] for f in frames], targets, rng=np.random.RandomState(3))
    assert [repr(p) for p in params] == [repr(p) for p in p2] and all(a.tobytes() == b.tobytes() for a, b in zip(tout, t2))
    same(x, R.batch(frames, params, AC.SIZES[0], AC.MEAN, AC.STD), "list")


def test_the_drop_in_class(gold, drawn):
    from yolo355.utils.augmentations import SSDAugmentation
    tag, frame, tgt, size, p, seed = drawn[0]
    np.random.seed(seed)
    boxes_in = tgt[:, :4].copy()
    img, boxes, labels = SSDAugmentation(list(size))(frame, boxes_in, tgt[:, 4])
    assert isinstance(img, np.ndarray) and np.array_equal(boxes_in, tgt[:, :4])
    same(img, gold[tag + "/image"], "SSDAugmentation")
    assert np.hstack((boxes, labels[:, None])).tobytes() == gold[tag + "/target"].tobytes()


def test_the_bench_tool_on_three_frames(capsys):
    import json
    from yolo355.tools import augment_bench
    res = augment_bench.main(["--frames", "3", "--reps", "2"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(res))
    assert res["equals_host_numpy"] is True and res["compulsory_bytes"] == 3 * (3 * 416 * 416 * 4 + 375 * 500 * 3)
    assert all(res[k] > 0 for k in ("draw_ms", "apply_ms", "frame_list_ms", "host_numpy_ms", "bound_ms")) and "kernel_ms" not in res


def test_losses_on_an_augmented_batch_equal_those_on_the_restated_batch():
    """the batch feeds loss_batch as it is: the four losses of the smallest SlimYOLOv2 configuration equal, bit for bit, those of the
    same batch built by tests/augment_ref.py and uploaded -- because the inputs are equal"""
    from cases import synth_state_dict
    from yolo355 import synth
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2
    size, C = [64, 64], 3
    m = SlimYOLOv2(DEV, input_size=size, num_classes=C, trainable=True, conf_thresh=0.01, nms_thresh=0.5, anchor_size=synth.ANCHOR_SIZE)
    m.load_state_dict(synth_state_dict(m.state_dict(), 11, weight_gain=2.0))
    m.eval()
    frames = [AC.frame(0, 40), AC.frame(1, 41)]
    targets = [AC.target(0, 40), AC.target(1, 41)]
    for t in targets:
        t[:, 4] %= C
    x, tout, params = A.augment_frame_list(frames, targets, size, rng=np.random.RandomState(2))
    ref = R.batch(frames, params, size, AC.MEAN, AC.STD)
    same(x, ref, "batch")
    out, parts = m.loss_batch(x, tout, quantization=False)
    out2, parts2 = m.loss_batch(torch.from_numpy(ref), tout, quantization=False)
    assert np.isfinite(out).all() and out.shape == (4,) and sum(len(t) for t in tout) >= 1
    assert out.tobytes() == out2.tobytes() and parts.tobytes() == parts2.tobytes(), (out, out2)
