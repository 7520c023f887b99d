"""Records tests/golden/trainers_parent.json: what the two training libraries, libyolo355_train.so (include/yolo355_train.h,
yolo355.train.SlimTrainer) and libyolo355_bntrain.so (include/yolo355_bntrain.h, yolo355.bntrain.SlimBNTrainer), answer and
compute at one commit, as tests/golden/gen_golden_companion_abi.py records the loss and anchor libraries:
  * "records": calls that answer before any device work and need no handle -- every entry point with a null handle, create
    with each of its rules broken and with a null out, the destroys of NULL (no return value: null) -- as
    [label, return code, the family's last-error text];
  * "gpu_records" (--gpu, on a GPU): SlimTrainer on the cases t16x32_b3_c20 and t48x80_b3_c2 of tests/train_cases.py and
    SlimBNTrainer on b16x32_b1_c20 and b48x80_b3_c2 of tests/bntrain_cases.py, each with the case's own images, labels and
    parameters, two steps a handle (the second takes the momentum branch of the update).  [label, SHA-256 of the raw bytes]
    of P after the first forward; of every tensor get_tensor serves, every layer's gradient (and BatchNorm's, and the batch
    statistics) after the first backward; of the four losses of each step; of every layer's parameters, momentum and packed
    weights (and BatchNorm's) after the second update.  Around them, on the same live handle, [label, return code, text] of
    the refusals a live handle gives: before the first forward, after the second step (ranges and null arguments), after a
    set_size to another size, and after a forward without a backward.  The calls change the handle, so their order is part
    of the record.
Both trainers promise the same bits from run to run, so two runs of --gpu at one commit write the same file.  Run at the commit
whose answers are to be pinned -- the parent of a change that must not move them:

    python tests/golden/gen_golden_trainers_parent.py [output.json]            # no GPU needed: commit, hipcc, records
    python tests/golden/gen_golden_trainers_parent.py --gpu [output.json]      # adds gpu_records to the file

tests/test_trainers_parent.py replays run_cpu() / run_gpu() on the built libraries and compares."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"), ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

TRAIN_CASES = ("t16x32_b3_c20", "t48x80_b3_c2")
BNTRAIN_CASES = ("b16x32_b1_c20", "b48x80_b3_c2")
LR = 1e-3
PTR = C.c_void_p(64)                             # a non-null pointer for calls that are refused before they would read it
NAN = float("nan")
# (tag, max_h, max_w, num_classes, num_anchors, max_batch) of create's rules, one broken each
CREATE_RULES = (("max_h 0", 0, 64, 2, 5, 1), ("max_h 60", 60, 64, 2, 5, 1), ("max_h 4112", 4112, 64, 2, 5, 1), ("max_w 8", 64, 8, 2, 5, 1),
                ("max_w 100", 64, 100, 2, 5, 1), ("max_w 4112", 64, 4112, 2, 5, 1), ("num_classes 0", 64, 64, 0, 5, 1),
                ("num_classes 201", 64, 64, 201, 5, 1), ("num_anchors 0", 64, 64, 2, 0, 1), ("num_anchors 17", 64, 64, 2, 17, 1),
                ("max_batch 0", 64, 64, 2, 5, 0), ("max_batch 1025", 64, 64, 2, 5, 1025))


class Family:
    """one library: its binding module, its prefix and whether it is the BatchNorm one"""

    def __init__(self, mod, bn):
        self.mod, self.bn, self.prefix = mod, bn, "y355_bntrain_" if bn else "y355_train_"

    def call(self, label, name, *args):
        """one call -> [label, return code, last-error text of a negative code]"""
        lib = self.mod.lib()
        rc = getattr(lib, self.prefix + name)(*args)
        return [label, rc, getattr(lib, self.prefix + "last_error")().decode() if rc is not None and rc < 0 else ""]


def cpu_records(F):
    """every entry point without a handle, create's rules"""
    out = C.c_void_p()
    i4, i3, i2 = (C.c_int32 * 4)(), (C.c_int32 * 3)(), (C.c_int32 * 2)()
    rec = lambda name, tag, *a: F.call("%s%s(%s)" % (F.prefix, name, tag), name, *a)       # noqa: E731
    got = [rec("create", "null out", 64, 64, 2, 5, 1, None)]
    got += [rec("create", r[0], *r[1:], C.byref(out)) for r in CREATE_RULES]
    assert not out.value
    null = "null handle"
    got += [rec("destroy", "NULL", None), rec("set_size", null, None, 64, 64), rec("layer_shape", null, None, 1, i2),
            rec("load_layer", null, None, 1, PTR, PTR), rec("get_layer", null, None, 1, PTR, PTR), rec("forward", null, None, PTR, 1, None),
            rec("pred", null, None, C.byref(out)), rec("backward", null, None, PTR, None), rec("get_grad", null, None, 1, PTR, PTR),
            rec("get_momentum", null, None, 1, PTR, PTR), rec("get_packed", null, None, 1, PTR), rec("wgrad_plan", null, None, 1, 1, i4),
            rec("sgd_step", null, None, 0.1, 0.9, 0.0, None), rec("tensor_shape", null, None, 0, 0, i4), rec("get_tensor", null, None, 0, 0, PTR)]
    if F.bn:
        n = C.c_int64()
        got += [rec("load_bn", null, None, 1, PTR, PTR, PTR, PTR, 0), rec("get_bn", null, None, 1, PTR, PTR, PTR, PTR, C.byref(n)),
                rec("get_bn_grad", null, None, 1, PTR, PTR), rec("get_bn_momentum", null, None, 1, PTR, PTR),
                rec("get_batch_stats", null, None, 1, PTR, PTR, PTR), rec("stats_plan", null, None, 1, 1, i3)]
    return got


def run_cpu(T, B):
    return cpu_records(Family(T, False)) + cpu_records(Family(B, True))


# ------------------------------------------------------------------------------------------------------------ live handles
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_trainer(F, tag):
    """(trainer, images on the device, labels) of a case, built as tests/test_train.py and tests/test_bntrain.py build theirs"""
    import torch
    if F.bn:
        import bntrain_cases as BC
        size, batch, classes = BC.CASES[tag]
        t = F.mod.SlimBNTrainer(size, classes, BC.ANCHORS, batch, LR)
        for k, L in enumerate(BC.params(tag), 1):
            t.load_layer(k, L["w"], L["b"])
            if L["bn"]:
                t.load_bn(k, *L["bn"])
        x, labels = BC.images(tag), BC.labels(tag)
    else:
        import train_cases as TC
        size, batch, classes = TC.CASES[tag]
        t = F.mod.SlimTrainer(size, classes, TC.ANCHORS, batch, LR)
        t.load_weights(TC.weights(tag))
        x, labels = TC.images(tag), TC.labels(tag)
    return t, torch.from_numpy(np.ascontiguousarray(x)).cuda(), labels


def refusals(F, t, tag, when):
    """the refusals of the live handle t in one of its states"""
    h, M = t._h, F.mod
    i4, i3, i2 = (C.c_int32 * 4)(), (C.c_int32 * 3)(), (C.c_int32 * 2)()
    rec = lambda name, what, *a: F.call("%s: %s, %s%s(%s)" % (tag, when, F.prefix, name, what), name, h, *a)       # noqa: E731
    if when != "after two steps":
        # no backward since the last forward: what needs one is refused ...
        got = [rec("get_grad", "", 1, PTR, PTR), rec("sgd_step", "", 0.1, 0.9, 0.0, None), rec("get_tensor", "GRAD 10", M.GRAD, 10, PTR)]
        if F.bn:
            got += [rec("get_bn_grad", "", 1, PTR, PTR), rec("get_tensor", "DY 1", M.DY, 1, PTR)]
        if when == "forward alone":
            return got
        # ... and with no forward at this size (fresh, another size), what needs that (PTR is never read)
        got += [rec("backward", "", PTR, None), rec("get_tensor", "ACT 0", M.ACT, 0, PTR)]
        if F.bn:
            got += [rec("get_tensor", "Z 1", M.Z, 1, PTR)]
        if when == "fresh" and F.bn:
            got += [rec("get_batch_stats", "", 1, PTR, PTR, PTR), rec("set_size", "16 x 16", 16, 16),
                    rec("forward", "one value per channel", PTR, 1, None), rec("set_size", "back", *t.max_size)]
        return got
    got = []
    for name, args in (("layer_shape", (i2,)), ("load_layer", (PTR, PTR)), ("get_layer", (PTR, PTR)), ("get_grad", (PTR, PTR)),
                       ("get_momentum", (PTR, PTR)), ("get_packed", (PTR,)), ("wgrad_plan", (1, i4))):
        got += [rec(name, "layer %d" % k, k, *args) for k in (0, 11)]
    got += [rec("layer_shape", "null shape", 1, None), rec("load_layer", "null w", 1, None, PTR), rec("load_layer", "null b", 1, PTR, None),
            rec("get_packed", "null", 1, None), rec("wgrad_plan", "null out", 1, 1, None), rec("wgrad_plan", "batch 0", 1, 0, i4),
            rec("wgrad_plan", "batch max_batch + 1", 1, t.max_batch + 1, i4), rec("forward", "null x", None, 1, None),
            rec("forward", "batch 0", PTR, 0, None), rec("forward", "batch max_batch + 1", PTR, t.max_batch + 1, None), rec("pred", "null out", None),
            rec("backward", "null dpred", None, None), rec("sgd_step", "lr nan", NAN, 0.9, 0.0, None), rec("sgd_step", "momentum nan", 0.1, NAN, 0.0, None),
            rec("sgd_step", "weight_decay nan", 0.1, 0.9, NAN, None), rec("tensor_shape", "null shape", M.ACT, 0, None),
            rec("get_tensor", "null out", M.ACT, 0, None), rec("set_size", "24 x 16", 24, 16), rec("set_size", "16 x 0", 16, 0),
            rec("set_size", "height beyond", t.max_size[0] + 16, 16), rec("set_size", "width beyond", 16, t.max_size[1] + 16)]
    kinds = [("ACT -1", M.ACT, -1), ("ACT 10", M.ACT, 10), ("IDX 0", M.IDX, 0), ("IDX 3", M.IDX, 3), ("IDX 10", M.IDX, 10), ("GRAD 0", M.GRAD, 0),
             ("GRAD 11", M.GRAD, 11), ("kind 9", 9, 1), ("kind -1", -1, 1)]
    if F.bn:
        kinds += [("Z 0", M.Z, 0), ("Z 10", M.Z, 10), ("DY 0", M.DY, 0), ("DY 10", M.DY, 10)]
        n = C.c_int64()
        for name, args in (("load_bn", (PTR, PTR, PTR, PTR, 0)), ("get_bn", (PTR, PTR, PTR, PTR, C.byref(n))), ("get_bn_grad", (PTR, PTR)),
                           ("get_bn_momentum", (PTR, PTR)), ("get_batch_stats", (PTR, PTR, PTR)), ("stats_plan", (1, i3))):
            got += [rec(name, "layer %d" % k, k, *args) for k in (0, 10)]
        got += [rec("load_bn", "null gamma", 1, None, PTR, PTR, PTR, 0), rec("load_bn", "null running_var", 1, PTR, PTR, PTR, None, 0),
                rec("load_bn", "num_batches_tracked -1", 1, PTR, PTR, PTR, PTR, -1), rec("stats_plan", "null out", 1, 1, None),
                rec("stats_plan", "batch 0", 1, 0, i3), rec("stats_plan", "batch max_batch + 1", 1, t.max_batch + 1, i3)]
    else:
        kinds += [("kind 3", 3, 1), ("kind 4", 4, 1)]
    got += [rec("tensor_shape", what, kind, idx, i4) for what, kind, idx in kinds]
    got += [rec("get_tensor", what, kind, idx, PTR) for what, kind, idx in kinds]
    return got


def run_case(F, tag):
    M = F.mod
    t, x, labels = make_trainer(F, tag)
    got = []
    put = lambda what, a: got.append(["%s: %s" % (tag, what), sha(a)])       # noqa: E731
    layers, bns = range(1, M.NUM_LAYERS + 1), range(1, M.NUM_BN + 1) if F.bn else ()
    try:
        got += refusals(F, t, tag, "fresh")
        t.forward_backward(x, labels)
        put("P after forward 1", t.pred().cpu().numpy())
        put("losses of step 1", np.asarray(t.losses, np.float64))
        for k in range(10):
            put("A_%d" % k, t.get_tensor(M.ACT, k))
        for k in M.POOLED:
            put("I_%d" % k, t.get_tensor(M.IDX, k))
        for k in bns:
            put("Z_%d" % k, t.get_tensor(M.Z, k))
            put("dY_%d" % k, t.get_tensor(M.DY, k))
        for k in layers:
            put("G_%d" % k, t.get_tensor(M.GRAD, k))
        for k in layers:
            w, b = t.get_grad(k)
            put("dW_%d" % k, w)
            put("db_%d" % k, b)
        for k in bns:
            for name, a in zip(("dgamma", "dbeta"), t.get_bn_grad(k)):
                put("%s_%d" % (name, k), a)
            for name, a in zip(("mean", "var", "invstd"), t.batch_stats(k)):
                put("batch %s_%d" % (name, k), a)
        t.update()
        t.step(x, labels)
        put("losses of step 2", np.asarray(t.losses, np.float64))
        for k in layers:
            for name, pair in (("", t.get_layer(k)), ("momentum of ", t.get_momentum(k))):
                put("%sW_%d after update 2" % (name, k), pair[0])
                put("%sb_%d after update 2" % (name, k), pair[1])
            put("packed W_%d after update 2" % k, t.get_packed(k))
        for k in bns:
            bn = t.get_bn(k)
            for name, a in zip(("gamma", "beta", "running_mean", "running_var"), bn[:4]):
                put("%s_%d after update 2" % (name, k), a)
            got.append(["%s: num_batches_tracked_%d after update 2" % (tag, k), str(bn[4])])
            for name, a in zip(("gamma", "beta"), t.get_bn_momentum(k)):
                put("momentum of %s_%d after update 2" % (name, k), a)
        got += refusals(F, t, tag, "after two steps")
        t.set_grid([16, 16])
        got += refusals(F, t, tag, "another size")
        t.set_grid(t.max_size)
        t.forward(x)
        got += refusals(F, t, tag, "forward alone")
    finally:
        t.close()
    return got


def run_gpu(T, B):
    got = []
    for tag in TRAIN_CASES:
        got += run_case(Family(T, False), tag)
    for tag in BNTRAIN_CASES:
        got += run_case(Family(B, True), tag)
    return got


def main():
    from yolo355 import bntrain as B, train as T
    args = [a for a in sys.argv[1:] if a != "--gpu"]
    out = args[0] if args else os.path.join(HERE, "trainers_parent.json")
    if "--gpu" in sys.argv:
        with open(out) as f:
            doc = json.load(f)
        doc["gpu_records"] = run_gpu(T, B)
    else:
        commit = os.environ.get("Y355_GOLDEN_COMMIT")
        if not commit:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        hipcc = [l for l in subprocess.check_output(["hipcc", "--version"], text=True).splitlines() if "version" in l]
        doc = {"commit": commit, "hipcc": hipcc[0] if hipcc else "", "records": run_cpu(T, B)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "with", len(doc["records"]), "records,", len(doc.get("gpu_records", [])), "gpu records")


if __name__ == "__main__":
    main()
