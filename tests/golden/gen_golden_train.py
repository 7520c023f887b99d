#!/usr/bin/env python3
"""Golden vectors of the training step, from the REFERENCE itself -> tests/golden/train.npz.

Runs only where the reference is checked out (import recipe of gen_golden.py), on the CPU; nothing of its source travels.
Inputs come from tests/train_cases.py (seeded), so only the reference's outputs are stored.  For every case the reference's
own SlimYOLOv2_quantize_bnfuse(trainable=True) in fp32, forward(x, target=tools.gt_creator(...)) and total_loss.backward() under
a torch.optim.SGD(momentum=0.9, weight_decay=5e-4) whose zero_grad() precedes it (the update itself is element-wise and is
pinned to torch.optim.SGD by tests/test_train_ref.py):

  train/<case>/losses                 fp32 [4]: conf, cls, txtytwth, total
  train/<case>/db/<layer>             fp32 [cout]
  train/<case>/dw/<layer>             fp32: the whole gradient (flattened) up to 20 000 elements, else the elements
                                      train_cases.sample_index keeps (at most 4 096); at most 512 in the cases after the
                                      first three, which keeps the file below the largest fixture there is
  train/<case>/dw_norm/<layer>        float64: the L2 norm of the whole weight gradient
  train/<case>/gap/<layer>            float64 [2]: max |reference - float64 restatement (tests/train_ref.py)| over the kept
                                      elements of dw and over db, not below one fp32 ulp of the largest |gradient|
  train/<case>/sides                  int64 [n, 3], only where n > 0: (t, flat index into A_t, 1 = positive side) of the
                                      elements at which an fp32 forward and a float64 forward lie on different sides of
                                      a LeakyReLU (train_ref.undecided_sides); the restatement of the gap takes these
  train/<case>/emu_relerr/<layer>   float64 [2]: relative L2 distance of the fp32 emulation of the contract
                                      (train_ref.step(contract=True)) from the reference, weights (kept elements) and bias

    python tests/golden/gen_golden_train.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402

import torch  # noqa: E402
import train_cases as TC  # noqa: E402
import train_ref as TR  # noqa: E402

LR = 1e-3


def main():
    ref = G.import_reference()
    tools = sys.modules["tools"]
    out = {}
    for tag in TC.GOLDEN_TAGS:
        size, B, C = TC.CASES[tag]
        ws, x, labels = TC.weights(tag), TC.images(tag), TC.labels(tag)
        model = ref.Q("cpu", input_size=size, num_classes=C, trainable=True, anchor_size=TC.ANCHORS)
        missing = model.load_state_dict(TC.state_dict(ws), strict=False)
        assert not missing.unexpected_keys, missing
        target = tools.gt_creator(size, TC.STRIDE, labels, TC.ANCHORS)
        mine_t = TR.targets(size, labels)
        assert np.array_equal(np.asarray(target, np.float64), mine_t), "targets of the restatement"
        opt = torch.optim.SGD(model.parameters(), lr=LR, momentum=0.9, weight_decay=5e-4)
        tgt = torch.tensor(target).float()
        losses = model(torch.from_numpy(x), target=tgt)
        opt.zero_grad()
        losses[3].backward()
        out["train/%s/losses" % tag] = np.array([float(v.detach()) for v in losses], np.float32)
        # where the fp32 forward lands on the other side of a LeakyReLU than float64 (a pre-activation fp32 cannot tell from
        # zero), the restatement takes the fp32 side; no pooling window may be undecided in the same way
        fwd = {}
        for dt in (torch.float32, torch.float64):
            fwd[dt] = TR.forward([(torch.from_numpy(w).to(dt), torch.from_numpy(b).to(dt)) for w, b in ws], torch.from_numpy(x).to(dt), False)
        assert all(torch.equal(fwd[torch.float32][1][k], fwd[torch.float64][1][k]) for k in fwd[torch.float64][1]), "an undecided pooling window"
        sides = TR.undecided_sides(fwd[torch.float32][0], fwd[torch.float64][0])
        if len(sides):
            out["train/%s/sides" % tag] = sides
            print(tag, "undecided LeakyReLU sides (A_t, flat index, positive in fp32):", sides.tolist())
        del fwd
        r_out, r_grads, _ = TR.step(ws, x, mine_t, size, C, False, sides)
        e_out, e_grads, _ = TR.step(ws, x, mine_t, size, C, True)
        sd = dict(model.named_parameters())
        for k, name in enumerate(TC.LAYERS, 1):
            kw, kb = TC.keys(k)
            dw, db = sd[kw].grad.numpy().reshape(-1), sd[kb].grad.numpy()
            assert dw.dtype == np.float32
            ix = TC.sample_index(dw.size, tag)
            out["train/%s/dw/%s" % (tag, name)] = dw[ix].copy()
            out["train/%s/db/%s" % (tag, name)] = db.copy()
            out["train/%s/dw_norm/%s" % (tag, name)] = np.float64(np.linalg.norm(dw.astype(np.float64)))
            rw, rbias = r_grads[k - 1][0].reshape(-1)[ix], r_grads[k - 1][1]
            gap = [max(np.abs(dw[ix] - rw).max(), float(np.spacing(np.abs(dw[ix]).max()))),
                   max(np.abs(db - rbias).max(), float(np.spacing(np.abs(db).max())))]
            out["train/%s/gap/%s" % (tag, name)] = np.array(gap, np.float64)
            ew, eb = e_grads[k - 1][0].reshape(-1)[ix], e_grads[k - 1][1]
            out["train/%s/emu_relerr/%s" % (tag, name)] = np.array([TC.rel_l2(ew, dw[ix]), TC.rel_l2(eb, db)], np.float64)
            print(tag, name, "kept %d of %d" % (ix.size, dw.size), "gap / max %.2g %.2g" % (gap[0] / np.abs(dw).max(), gap[1] / np.abs(db).max()),
                  "emu_relerr %.3g %.3g" % tuple(out["train/%s/emu_relerr/%s" % (tag, name)]))
        print(tag, "losses", out["train/%s/losses" % tag], "restatement", r_out, "emulation", e_out)
    path = os.path.join(HERE, "train.npz")
    if os.path.exists(path):                      # adding a case leaves the entries of the cases before it byte for byte as they were
        with np.load(path) as z:
            for key in z.files:
                assert key in out and out[key].dtype == z[key].dtype and out[key].shape == z[key].shape and out[key].tobytes() == z[key].tobytes(), key
            print("the %d entries of the fixture that was here come out byte for byte" % len(z.files))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
