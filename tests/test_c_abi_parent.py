"""The C ABI of libyolo355.so, pinned to tests/golden/c_abi_parent.json (recorded by tests/golden/gen_golden_c_abi.py at the
commit named in the file): the library exports the recorded symbols, and every recorded call still answers with the recorded
return code and y355_last_error() text -- wherever the code behind it lives now.  The "records" need no GPU; the
"gpu_records" are replayed on a live handle of each family.  The owned stream of a y355_net (own_stream = 1), which no Python
class asks for, is run here against a Net on torch's stream."""
import ctypes as C
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_c_abi", os.path.join(GOLDEN, "gen_golden_c_abi.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the generator's calls: one definition of a record

with open(os.path.join(GOLDEN, "c_abi_parent.json")) as _f:
    DOC = json.load(_f)


def _compare(got, want):
    assert [r[0] for r in got] == [r[0] for r in want]          # the same calls, in the recorded order
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad


def test_the_snapshot_covers_both_families():
    labels = [r[0] for r in DOC["records"]]
    assert len(labels) == len(set(labels)) == 90 and len(DOC["gpu_records"]) == 59
    assert sum(lb.startswith("y355_net_") for lb in labels) >= 44 and sum(lb.startswith("y355_create") for lb in labels) == 12
    assert {"null engine", "null net", "unknown arch", "unknown dtype"} <= {r[2] for r in DOC["records"]}


def test_exported_symbols():
    from yolo355 import _ffi
    assert G.symbols(_ffi.LIB_PATH) == DOC["symbols"]


def test_answers_before_any_device_work():
    from yolo355 import _ffi
    lib = _ffi.lib()
    _compare(G.run(lib, G.cpu_calls(_ffi, lib)), DOC["records"])


@pytest.mark.gpu
def test_answers_of_live_handles():
    from yolo355 import _ffi
    lib = _ffi.lib()
    eng, net = G.live_handles()
    try:
        got = G.run(lib, G.gpu_calls(_ffi, lib, eng._h, net._h, net.num_trackers))
        G.drain_last_error(lib, eng)
    finally:
        eng.close()
        net.close()
    _compare(got, DOC["gpu_records"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "int8"])
def test_net_on_its_own_stream(dtype):
    """y355_net_create with own_stream = 1: one forward and y355_net_sync on the net's non-blocking stream, then destroy; the
    four output arrays equal, byte for byte, those of a Net on torch's stream with the same weights and input"""
    import torch
    from yolo355 import _ffi, prep, synth
    from yolo355._handle import out_buffers
    from yolo355.netengine import Net

    class OwnStreamNet(Net):
        def _create(self, lib, cfg, create):
            self._stream = torch.cuda.current_stream(self.device)
            cfg.stream, cfg.own_stream = None, 1
            h = C.c_void_p()
            _ffi.check(create(C.byref(cfg), C.byref(h)))
            self._own(lib, h)

    size = [G.SIZE, G.SIZE]
    folded = G.folded_layers(synth.make_fp32_model("slim_yolo_v2", 5, G.CLASSES, 5, pred_gain=1.5, obj_bias=-2.0))
    x = torch.from_numpy(synth.make_images(3, G.BATCH, size[0], size[1], "blocks")).cuda()
    outs = []
    exponents = None
    for cls in (Net, OwnStreamNet):
        net = cls("slim_yolo_v2", size, G.CLASSES, synth.ANCHOR_SIZE_MASK, 0.01, 0.5, max_batch=G.BATCH, dtype=dtype)
        try:
            if dtype == "bf16":
                for i, (w, b) in enumerate(folded):
                    net.load_layer(i, w, b)
            else:
                for i, q in enumerate(prep.quantize_folded(folded)):
                    net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
                if exponents is None:
                    net.calibrate(x)
                    exponents = net.get_act_exponents()
                net.set_act_exponents(*exponents)
            out = out_buffers(G.BATCH, net.max_det, net.device)
            for t in out:
                t.fill_(0)
            torch.cuda.synchronize()                      # the input and the buffers are ready before the other stream starts
            net.forward_device(x, out=out)
            net.sync()
            outs.append([t.cpu().numpy() for t in out])
        finally:
            net.close()
    assert outs[0][3].min() > 0                           # detections in both images
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
