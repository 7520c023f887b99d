"""Training of the BatchNorm SlimYOLOv2 (models/slim_yolo_v2.py::SlimYOLOv2, the network train.py -v slim_yolo_v2 trains from
scratch) on the GPU: ctypes binding of include/yolo355_bntrain.h (csrc/bntrain.hip, the companion library
libyolo355_bntrain.so, loaded the first time it is asked for) and SlimBNTrainer, one object for the reference's loop body --
forward in train() mode (batch statistics, the running ones move), tools.loss, total_loss.backward(),
optim.SGD(model.parameters(), lr, momentum, weight_decay).step(), zero_grad() -- with SlimTrainer's surface.  The loss and its
gradient with respect to the prediction map are yolo355.grad's.  fused_state_dict() hands the trained network over to the
folded trainer (yolo355.train.SlimTrainer), the SlimYOLOv2_quantize_bnfuse drop-in and the int8 preparation; LrSchedule is
the learning-rate rule of the reference's loop.  The arithmetic contract is DESIGN.md section 6n.  No CPU path: without a
GPU every device entry point raises."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _ffi
from ._trainer import ACT, GRAD, IDX, LAYER_NAMES, NUM_LAYERS, POOLED, STRIDE, Trainer, _np, common_sigs, layer_keys  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_bntrain.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_bntrain.h"))

P = C.POINTER
_V, _I = C.c_void_p, C.c_int32
_SIGS = dict(common_sigs("y355_bntrain_"), **{
    "y355_bntrain_load_bn": (C.c_int, [_V, _I, _V, _V, _V, _V, C.c_int64]),
    "y355_bntrain_get_bn": (C.c_int, [_V, _I, _V, _V, _V, _V, P(C.c_int64)]),
    "y355_bntrain_get_batch_stats": (C.c_int, [_V, _I, _V, _V, _V]),
    "y355_bntrain_get_bn_grad": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_bn_momentum": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_stats_plan": (C.c_int, [_V, _I, _I, P(_I)]),
})
_lib = None
# libyolo355_bntrain.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_bntrain_", "extensions first (make -C csrc)")

NUM_BN = 9
Z, DY = 3, 4
EPS, BN_MOMENTUM = 1e-5, 0.1
BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def bn_keys(k):
    """the five BatchNorm keys of layer k = 1..9 in the reference's state_dict (gamma, beta, running_mean, running_var,
    num_batches_tracked)"""
    return tuple("%s.convs.1.%s" % (LAYER_NAMES[k - 1], f) for f in BN_FIELDS)


def fuse_state_dict(sd, corrected=False):
    """The BN-folded parameters of a state_dict in the reference's BatchNorm layout, under SlimTrainer's keys
    (convK.convs.0.{weight,bias}, pred.{weight,bias}): prep.fuse_conv_and_bn per layer on the running statistics, the
    reference's fold by default (utils/bn_fuse.py, which leaves the conv bias unscaled), the exact one with corrected=True."""
    from . import prep
    out = {}
    for k in range(1, NUM_BN + 1):
        kw, kb = layer_keys(k)
        g, be, mu, var, _ = bn_keys(k)
        w = torch.as_tensor(_np(sd[kw]), dtype=torch.float32)
        conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1, bias=True)
        bn = torch.nn.BatchNorm2d(w.shape[0], eps=EPS, momentum=BN_MOMENTUM)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(torch.as_tensor(_np(sd[kb]), dtype=torch.float32))
            bn.weight.copy_(torch.as_tensor(_np(sd[g]), dtype=torch.float32))
            bn.bias.copy_(torch.as_tensor(_np(sd[be]), dtype=torch.float32))
            bn.running_mean.copy_(torch.as_tensor(_np(sd[mu]), dtype=torch.float32))
            bn.running_var.copy_(torch.as_tensor(_np(sd[var]), dtype=torch.float32))
        f = prep.fuse_conv_and_bn(conv, bn, corrected=corrected)
        out[kw], out[kb] = f.weight.detach().clone(), f.bias.detach().clone()
    kw, kb = layer_keys(NUM_LAYERS)
    out[kw] = torch.as_tensor(_np(sd[kw]), dtype=torch.float32).clone()
    out[kb] = torch.as_tensor(_np(sd[kb]), dtype=torch.float32).clone()
    return out


class LrSchedule:
    """The learning rate of the reference's loop (train.py:252-281): epoch_start(epoch) before an epoch's first batch,
    iteration(epoch, iter_i) before every batch; both return the rate to set.  Warm-up: base_lr times the fourth power of the
    fraction of the wp_epoch * epoch_size warm-up iterations done, base_lr itself at the first iteration of epoch wp_epoch.
    Steps: a tenth at every epoch of lr_epoch.  cos: between epochs 20 and max_epoch - 20 (exclusive, inclusive) half a cosine
    over max_epoch - 20 epochs down towards 1e-5, and 1e-5 after that."""
    FLOOR = 0.00001

    def __init__(self, base_lr, epoch_size, max_epoch, lr_epoch, cos=False, warm_up=True, wp_epoch=2):
        self.base_lr, self.epoch_size, self.max_epoch = float(base_lr), int(epoch_size), int(max_epoch)
        self.lr_epoch, self.cos, self.warm_up, self.wp_epoch = tuple(lr_epoch), bool(cos), bool(warm_up), int(wp_epoch)
        self.lr = self.base_lr

    def epoch_start(self, epoch):
        if self.cos and 20 < epoch <= self.max_epoch - 20:
            self.lr = self.FLOOR + 0.5 * (self.base_lr - self.FLOOR) * (1 + math.cos(math.pi * (epoch - 20) * 1. / (self.max_epoch - 20)))
        elif self.cos and epoch > self.max_epoch - 20:
            self.lr = self.FLOOR
        elif epoch in self.lr_epoch:
            self.lr = self.lr * 0.1
        return self.lr

    def iteration(self, epoch, iter_i):
        if self.warm_up:
            if epoch < self.wp_epoch:
                self.lr = self.base_lr * pow((iter_i + epoch * self.epoch_size) * 1. / (self.wp_epoch * self.epoch_size), 4)
            elif epoch == self.wp_epoch and iter_i == 0:
                self.lr = self.base_lr
        return self.lr


class SlimBNTrainer(Trainer):
    """The training step of SlimYOLOv2(trainable=True).train() with torch.optim.SGD(model.parameters(), lr, momentum,
    weight_decay): a forward moves the running statistics, update() steps W, b, gamma and beta and leaves them.  input_size
    [H, W] (multiples of 16) is the largest size the trainer takes; set_grid switches within it."""
    _destroy = "y355_bntrain_destroy"
    _prefix, _lib_fn, _check = "y355_bntrain_", staticmethod(lib), staticmethod(check)

    # ------------------------------------------------------------------ parameters
    def load_bn(self, k, gamma, beta, running_mean, running_var, num_batches_tracked=0):
        """BatchNorm of layer k = 1..9: four float [cout] arrays and the count"""
        if not 1 <= k <= NUM_BN:
            raise ValueError("BatchNorm exists on layers 1..9, got %d" % k)
        cout = self.layer_shape(k)[0]
        a = [np.ascontiguousarray(np.asarray(v, np.float32)) for v in (gamma, beta, running_mean, running_var)]
        if any(v.shape != (cout,) for v in a):
            raise ValueError("layer %d: expected four arrays [%d], got %s" % (k, cout, [v.shape for v in a]))
        self._call("load_bn", k, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, int(num_batches_tracked))

    def _channels(self, name, k, n, *tail):
        cout = self.layer_shape(k)[0]
        out = [np.empty((cout,), np.float32) for _ in range(n)]
        self._call(name, k, *[v.ctypes.data for v in out], *tail)
        return tuple(out)

    def get_bn(self, k):
        """(gamma, beta, running_mean, running_var, num_batches_tracked) of layer k = 1..9"""
        n = C.c_int64()
        return self._channels("get_bn", k, 4, C.byref(n)) + (int(n.value),)

    def get_bn_grad(self, k):
        """(dgamma, dbeta) of the last backward"""
        return self._channels("get_bn_grad", k, 2)

    def get_bn_momentum(self, k):
        return self._channels("get_bn_momentum", k, 2)

    def batch_stats(self, k):
        """(mean, biased var, invstd) of layer k = 1..9 in the last forward, float32 [cout]"""
        return self._channels("get_batch_stats", k, 3)

    def load_state_dict(self, sd):
        """a state_dict in the reference's key layout: convK.convs.0.{weight,bias}, convK.convs.1.{weight,bias,running_mean,
        running_var[,num_batches_tracked]}, pred.{weight,bias} (what synth.state_dict_fp32 writes); other keys are ignored"""
        for k in range(1, NUM_LAYERS + 1):
            need = list(layer_keys(k)) + (list(bn_keys(k)[:4]) if k <= NUM_BN else [])
            missing = [n for n in need if n not in sd]
            if missing:
                raise KeyError("state_dict lacks %s" % ", ".join(missing))
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            self.load_layer(k, _np(sd[kw]), _np(sd[kb]))
            if k <= NUM_BN:
                g, be, mu, var, nbt = bn_keys(k)
                self.load_bn(k, _np(sd[g]), _np(sd[be]), _np(sd[mu]), _np(sd[var]), int(_np(sd[nbt])) if nbt in sd else 0)

    def state_dict(self):
        """the fp32 master parameters and the BatchNorm buffers as CPU torch tensors under the reference's keys, in the
        reference's order"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            w, b = self.get_layer(k)
            kw, kb = layer_keys(k)
            out[kw], out[kb] = torch.from_numpy(w), torch.from_numpy(b)
            if k <= NUM_BN:
                vals = self.get_bn(k)
                for key, v in zip(bn_keys(k), vals):
                    out[key] = torch.tensor(v, dtype=torch.int64) if isinstance(v, int) else torch.from_numpy(v)
        return out

    def fused_state_dict(self, corrected=False):
        """the BN-folded network under SlimTrainer's keys (fuse_state_dict on state_dict()): what SlimTrainer.load_state_dict,
        the SlimYOLOv2_quantize_bnfuse drop-in and the int8 preparation take"""
        return fuse_state_dict(self.state_dict(), corrected=corrected)

    def gradients(self):
        """{key: float32 array} of the last backward pass, under the state_dict's parameter keys"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            out[kw], out[kb] = self.get_grad(k)
            if k <= NUM_BN:
                out[bn_keys(k)[0]], out[bn_keys(k)[1]] = self.get_bn_grad(k)
        return out

    def stats_plan(self, k, batch=None):
        """How forward and backward cut the BatchNorm reductions of layer k = 1..9 at the current size: dict(N, runs, chunk) --
        runs workgroup runs of chunk pixels each, the last one the rest (y355_bntrain_stats_plan, what the passes launch from)"""
        s = (C.c_int32 * 3)()
        self._call("stats_plan", int(k), self._plan_batch(batch), s)
        return dict(N=int(s[0]), runs=int(s[1]), chunk=int(s[2]))

    # ------------------------------------------------------------------ taps (tests)
    def get_tensor(self, kind, t):
        """tensor t of a kind (ACT: A_t, Z: Z_t, DY: dY_t, GRAD: G_t as bf16 bits; IDX: I_t uint8) as a numpy array in NCHW order"""
        return super().get_tensor(kind, t)
