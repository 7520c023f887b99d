"""The two training libraries, libyolo355_train.so and libyolo355_bntrain.so, pinned to tests/golden/trainers_parent.json
(recorded by tests/golden/gen_golden_trainers_parent.py at the commit named in the file): every recorded call still answers
with the recorded return code and its family's last-error text, and two training steps on the four smallest cases still leave
the recorded bits -- P, every tensor, gradient, statistic, loss, parameter, momentum and pack, as SHA-256 of their raw bytes --
wherever the host code behind them lives now.  The "records" need no GPU; the "gpu_records" are replayed in the recorded order
on one live handle a case.  Nothing here skips: the toolchain line in the file is for information, and any difference is a
failure that names the records that differ.

A later change that moves the arithmetic on purpose (another rounding, another order of a sum) regenerates the file at its own
commit with the generator and says so; one that only moves code must leave it as it is."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_trainers_parent", os.path.join(GOLDEN, "gen_golden_trainers_parent.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the generator's calls: one definition of a record

with open(os.path.join(GOLDEN, "trainers_parent.json")) as _f:
    DOC = json.load(_f)


def _compare(got, want):
    assert [r[0] for r in got] == [r[0] for r in want]          # the same calls, in the recorded order
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, "%d records differ (got, recorded): %s" % (len(bad), bad[:8])


def test_the_snapshot_covers_every_entry_point():
    from yolo355 import bntrain as B, train as T
    assert len(DOC["commit"]) == 40 and "version" in DOC["hipcc"]
    for key in ("records", "gpu_records"):
        labels = [r[0] for r in DOC[key]]
        assert len(labels) == len(set(labels))
    for mod, prefix, count in ((T, "y355_train_", 17), (B, "y355_bntrain_", 23)):
        names = {r[0].split("(")[0] for r in DOC["records"] if r[0].startswith(prefix)}
        assert names | {prefix + "last_error"} == set(mod._SIGS) and len(mod._SIGS) == count          # every entry point of the header
        assert sum(r[0].startswith(prefix + "create(") for r in DOC["records"]) == len(G.CREATE_RULES) + 1
        live = {r[0].split(", ", 1)[1].split("(")[0] for r in DOC["gpu_records"] if len(r) == 3 and (", " + prefix) in r[0]}
        assert live == set(mod._SIGS) - {prefix + n for n in ("last_error", "create", "destroy")}
    assert all(r[1] in (-1, None) for r in DOC["records"])
    assert {r[1] for r in DOC["gpu_records"] if len(r) == 3} == {-3, -1, 0}                           # ENOTREADY, EINVAL, set_size's success
    hashed = [r for r in DOC["gpu_records"] if len(r) == 2]
    for tag in G.TRAIN_CASES + G.BNTRAIN_CASES:
        bn = tag in G.BNTRAIN_CASES
        # P, 2 x losses, A_0..9, I_1,2,4,6, G_1..10, dW/db, then W, b, their momenta and the pack of ten layers; BatchNorm adds
        # Z, dY, dgamma, dbeta, three statistics, four buffers, the count and two momenta of nine layers
        assert sum(r[0].startswith(tag + ": ") for r in hashed) == 3 + 10 + 4 + 10 + 20 + 50 + (9 * 14 if bn else 0), tag
    texts = {r[2] for r in DOC["gpu_records"] if len(r) == 3}
    for t in ("y355_train_backward: no forward pass has run at this size", "y355_bntrain_get_tensor: no backward pass has run",
              "y355_train_get_packed: layer index must be 1..10", "y355_bntrain_get_bn: layer index must be 1..9",
              "y355_bntrain_set_size: size beyond the handle's maximum", "y355_bntrain_get_batch_stats: no forward pass has run",
              "y355_train_get_tensor: no such tensor", "y355_bntrain_sgd_step: lr, momentum and weight_decay must be numbers"):
        assert t in texts, t
    assert any("needs more than one value per channel" in t for t in texts)


def test_answers_before_any_device_work():
    from yolo355 import bntrain as B, train as T
    _compare(G.run_cpu(T, B), DOC["records"])


@pytest.mark.gpu
def test_two_steps_and_the_refusals_of_live_handles():
    from yolo355 import bntrain as B, train as T
    _compare(G.run_gpu(T, B), DOC["gpu_records"])
