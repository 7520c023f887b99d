"""voc_map's admission rule for the device-resident route (_pipeline_admits) is a restatement of the one _submit applies:
the two must pick the pipeline for exactly the same (model, batch, arguments)."""
import itertools

import numpy as np
import torch

from yolo355 import _ffi
from yolo355.utils import evaluator_batch as EB


class _Tracker:
    def __init__(self, first_a):
        self.first_a = first_a


def _net(calibrated, has_submit, has_trackers, chunk):
    class Net:
        def forward_batch(self, x, quantization=False, find=False, sizes_wh=None):
            return "ran"
    n = Net()
    if has_submit:
        n.submit_batch = lambda x, quantization=True, find=False, sizes_wh=None: "token"
        n.collect_batch = lambda token: "collected"
    if has_trackers:
        n._tracker_states = lambda: [_Tracker(1), _Tracker(1 if calibrated else 0)]
    if chunk is not None:
        n.PIPELINE_CHUNK = chunk
    return n


def test_pipeline_admits_is_the_rule_of_submit():
    limit = 2 * _ffi.PIPE_DEFAULT_HANDLES * 64
    seen = set()
    for cal, sub, trk, chunk, q, find, batch in itertools.product((0, 1), (0, 1), (0, 1), (None, 64), (False, True), (False, True),
                                                                   (1, limit, limit + 1)):
        if q and trk and not cal:
            continue                   # _run would calibrate on image 0 first: needs a real model; the rule is covered by cal = 1 / trk = 0
        net = _net(cal, sub, trk, chunk)
        x = torch.zeros(batch, 3, 2, 2)
        took_pipeline = EB._submit(net, x, np.ones((batch, 2), np.float32), quantization=q, find=find)() == "collected"
        assert took_pipeline == EB._pipeline_admits(net, batch, quantization=q, find=find), (cal, sub, trk, chunk, q, find, batch)
        seen.add(took_pipeline)
    assert seen == {False, True}
    net = _net(0, 1, 1, 64)            # an un-calibrated model is never admitted
    assert not EB._pipeline_admits(net, 1, quantization=True, find=False)
