#!/usr/bin/env python3
"""Golden vectors of the BatchNorm training step, from the REFERENCE itself -> tests/golden/bntrain.npz.

Runs only where the reference is checked out (import recipe of gen_golden.py), on the CPU; nothing of its source travels.
Inputs come from tests/bntrain_cases.py (seeded), so only the reference's outputs are stored.  For every case the reference's
own SlimYOLOv2(trainable=True).train() in fp32, forward(x, target=tools.gt_creator(...)) and total_loss.backward() under a
torch.optim.SGD(momentum=0.9, weight_decay=5e-4) whose zero_grad() precedes it:

  bntrain/<case>/losses               fp32 [4]: conf, cls, txtytwth, total
  bntrain/<case>/dw/<layer>           fp32: the elements of the flattened weight gradient bntrain_cases.sample_index keeps
  bntrain/<case>/db/<layer>           fp32 [cout]
  bntrain/<case>/dgamma/<layer>       fp32 [cout], layers 1..9
  bntrain/<case>/dbeta/<layer>        fp32 [cout], layers 1..9
  bntrain/<case>/running_mean/<layer> fp32 [cout] after the forward, layers 1..9 (and running_var; num_batches_tracked is 1)
  bntrain/<case>/gap/<layer>          float64 [4]: max |reference - float64 restatement (tests/bntrain_ref.py)| over the kept
                                      elements of dw and over db, dgamma, dbeta (pred: the last two 0), not below one fp32
                                      ulp of the largest |gradient|
  bntrain/<case>/stat_gap/<layer>     float64 [2]: the same for running_mean and running_var
  bntrain/<case>/picks                int64 [n, 3], only where n > 0: bntrain_ref.undecided_windows between an fp32 and a
                                      float64 forward of the restatement (pooling windows fp32 cannot decide)
  bntrain/<case>/sides                int64 [n, 3], only where n > 0: train_ref.undecided_sides between the two forwards;
                                      the restatement of the gap takes both
  bntrain/<case>/emu_relerr/<layer>   float64 [4]: relative L2 distance of the fp32 emulation of the contract
                                      (bntrain_ref.step(contract=True)) from the reference: dw (kept elements), db, dgamma, dbeta

    python tests/golden/gen_golden_bntrain.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402

import torch  # noqa: E402
import bntrain_cases as BC  # noqa: E402
import bntrain_ref as BR  # noqa: E402
import train_ref as TR  # noqa: E402

LR = 1e-3


def main():
    ref = G.import_reference()
    tools = sys.modules["tools"]
    out = {}
    for tag in BC.GOLDEN_TAGS:
        size, B, C = BC.CASES[tag]
        layers, x, labels = BC.params(tag), BC.images(tag), BC.labels(tag)
        model = ref.SlimYOLOv2("cpu", input_size=size, num_classes=C, trainable=True, anchor_size=BC.ANCHORS)
        missing = model.load_state_dict(BC.state_dict(tag), strict=False)
        assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
        model.train()
        target = tools.gt_creator(size, BC.STRIDE, labels, BC.ANCHORS)
        mine_t = TR.targets(size, labels)
        assert np.array_equal(np.asarray(target, np.float64), mine_t), "targets of the restatement"
        opt = torch.optim.SGD(model.parameters(), lr=LR, momentum=0.9, weight_decay=5e-4)
        seen = {}                                             # the reference's own activations, before the pools
        hooks = [getattr(model, name).register_forward_hook(lambda m, i, o, k=k: seen.__setitem__(k, o.detach().clone()))
                 for k, name in enumerate(BC.LAYERS[:9], 1)]
        losses = model(torch.from_numpy(x), target=torch.tensor(target).float())
        opt.zero_grad()
        losses[3].backward()
        out["bntrain/%s/losses" % tag] = np.array([float(v.detach()) for v in losses], np.float32)
        for h in hooks:
            h.remove()
        # where the reference's fp32 forward selects another window position or lands on the other side of a LeakyReLU than
        # float64 (two values fp32 cannot tell apart), the restatement takes the reference's choice
        I_ref = {k: TR.pool_first(seen[k])[1] for k in range(1, 10) if BC.POOL[k - 1]}
        A_ref = [torch.from_numpy(x)] + [TR.pool_first(seen[k])[0] if BC.POOL[k - 1] else seen[k] for k in range(1, 10)]
        fwd = BR.forward(BR.tensors(layers, torch.float64), torch.from_numpy(x).double(), False)
        picks = BR.undecided_windows(I_ref, fwd[1])
        if len(picks):
            out["bntrain/%s/picks" % tag] = picks
            print(tag, "undecided pooling windows (layer, flat index, position in fp32):", picks.tolist())
            fwd = BR.forward(BR.tensors(layers, torch.float64), torch.from_numpy(x).double(), False, picks)
            assert all(torch.equal(I_ref[k], fwd[1][k]) for k in I_ref)
        sides = TR.undecided_sides(A_ref, fwd[0])
        if len(sides):
            out["bntrain/%s/sides" % tag] = sides
            print(tag, "undecided LeakyReLU sides (A_t, flat index, positive in fp32):", sides.tolist())
        del fwd
        r = BR.step(layers, x, mine_t, size, C, False, sides, picks)
        e = BR.step(layers, x, mine_t, size, C, True)
        run = BR.running_after(layers, r["stats"])
        sd, bufs = dict(model.named_parameters()), dict(model.named_buffers())
        floor = lambda v: float(np.spacing(np.abs(v).max()))
        for k, name in enumerate(BC.LAYERS, 1):
            kw, kb = BC.keys(k)
            dw, db = sd[kw].grad.numpy().reshape(-1), sd[kb].grad.numpy()
            assert dw.dtype == np.float32
            ix = BC.sample_index(dw.size, tag)
            want = [dw[ix].copy(), db.copy()]
            got_r, got_e = [r["grads"][k - 1][0].reshape(-1)[ix], r["grads"][k - 1][1]], [e["grads"][k - 1][0].reshape(-1)[ix], e["grads"][k - 1][1]]
            out["bntrain/%s/dw/%s" % (tag, name)], out["bntrain/%s/db/%s" % (tag, name)] = want
            if k <= 9:
                g, be, mu, var = BC.bn_keys(k)
                want += [sd[g].grad.numpy().copy(), sd[be].grad.numpy().copy()]
                got_r += list(r["grads"][k - 1][2:])
                got_e += list(e["grads"][k - 1][2:])
                out["bntrain/%s/dgamma/%s" % (tag, name)], out["bntrain/%s/dbeta/%s" % (tag, name)] = want[2:]
                rm, rv = bufs[mu].numpy().copy(), bufs[var].numpy().copy()
                out["bntrain/%s/running_mean/%s" % (tag, name)], out["bntrain/%s/running_var/%s" % (tag, name)] = rm, rv
                out["bntrain/%s/stat_gap/%s" % (tag, name)] = np.array([max(np.abs(rm - run[k][0]).max(), floor(rm)), max(np.abs(rv - run[k][1]).max(), floor(rv))])
                assert int(bufs[mu.replace("running_mean", "num_batches_tracked")]) == 1
            gap = [max(np.abs(w - g_).max(), floor(w)) for w, g_ in zip(want, got_r)] + [0.0] * (4 - len(want))
            rel = [BC.rel_l2(g_, w) for w, g_ in zip(want, got_e)] + [0.0] * (4 - len(want))
            out["bntrain/%s/gap/%s" % (tag, name)] = np.array(gap, np.float64)
            out["bntrain/%s/emu_relerr/%s" % (tag, name)] = np.array(rel, np.float64)
            print(tag, name, "kept %d of %d" % (ix.size, dw.size), "gap / max", " ".join("%.2g" % (g_ / max(np.abs(w).max(), 1e-300)) for g_, w in zip(gap, want)),
                  "emu_relerr", " ".join("%.3g" % v for v in rel))
        print(tag, "losses", out["bntrain/%s/losses" % tag], "restatement", r["losses"], "emulation", e["losses"])
    path = os.path.join(HERE, "bntrain.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
