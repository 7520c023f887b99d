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
from ._handle import Handle, _require_gpu
from . import grad as _grad
from .train import LAYER_NAMES, POOLED, STRIDE, layer_keys, _np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_bntrain.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_bntrain.h"))

P = C.POINTER
_V, _I = C.c_void_p, C.c_int32
_SIGS = {
    "y355_bntrain_last_error": (C.c_char_p, []),
    "y355_bntrain_create": (C.c_int, [_I, _I, _I, _I, _I, P(_V)]),
    "y355_bntrain_destroy": (None, [_V]),
    "y355_bntrain_set_size": (C.c_int, [_V, _I, _I]),
    "y355_bntrain_load_layer": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_layer": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_layer_shape": (C.c_int, [_V, _I, P(_I)]),
    "y355_bntrain_load_bn": (C.c_int, [_V, _I, _V, _V, _V, _V, C.c_int64]),
    "y355_bntrain_get_bn": (C.c_int, [_V, _I, _V, _V, _V, _V, P(C.c_int64)]),
    "y355_bntrain_forward": (C.c_int, [_V, _V, _I, _V]),
    "y355_bntrain_pred": (C.c_int, [_V, P(_V)]),
    "y355_bntrain_get_batch_stats": (C.c_int, [_V, _I, _V, _V, _V]),
    "y355_bntrain_backward": (C.c_int, [_V, _V, _V]),
    "y355_bntrain_get_grad": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_bn_grad": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_momentum": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_bn_momentum": (C.c_int, [_V, _I, _V, _V]),
    "y355_bntrain_get_packed": (C.c_int, [_V, _I, _V]),
    "y355_bntrain_wgrad_plan": (C.c_int, [_V, _I, _I, P(_I)]),
    "y355_bntrain_stats_plan": (C.c_int, [_V, _I, _I, P(_I)]),
    "y355_bntrain_sgd_step": (C.c_int, [_V, C.c_float, C.c_float, C.c_float, _V]),
    "y355_bntrain_tensor_shape": (C.c_int, [_V, _I, _I, P(_I)]),
    "y355_bntrain_get_tensor": (C.c_int, [_V, _I, _I, _V]),
}
_lib = None
# libyolo355_bntrain.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_bntrain_", "extensions first (make -C csrc)")

NUM_LAYERS, NUM_BN = 10, 9
ACT, IDX, GRAD, Z, DY = 0, 1, 2, 3, 4
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


class SlimBNTrainer(Handle):
    """The training step of SlimYOLOv2(trainable=True).train() with torch.optim.SGD(model.parameters(), lr, momentum,
    weight_decay).  input_size [H, W] (multiples of 16) is the largest size the trainer takes; set_grid switches within it."""
    _destroy = "y355_bntrain_destroy"

    def __init__(self, input_size, num_classes, anchor_size, max_batch, lr, momentum=0.9, weight_decay=5e-4, device=None):
        l = lib()
        self.device = _require_gpu(device)
        self.max_size = [int(input_size[0]), int(input_size[1])]
        self.input_size = list(self.max_size)
        self.num_classes, self.max_batch = int(num_classes), int(max_batch)
        self.anchor_size = [[float(v) for v in a] for a in np.asarray(anchor_size, np.float64).reshape(-1, 2)]
        self.num_anchors = len(self.anchor_size)
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(l.y355_bntrain_create(self.max_size[0], self.max_size[1], self.num_classes, self.num_anchors, self.max_batch, C.byref(h)))
        self._own(l, h)
        self._criteria = {}
        self._dpred = None
        self._batch = 0

    # ------------------------------------------------------------------ parameters
    def layer_shape(self, k):
        s = (C.c_int32 * 2)()
        check(self._lib.y355_bntrain_layer_shape(self._h, k, s))
        return int(s[0]), int(s[1])

    def load_layer(self, k, w, b):
        cout, cin = self.layer_shape(k)
        w = np.ascontiguousarray(np.asarray(w, np.float32))
        b = np.ascontiguousarray(np.asarray(b, np.float32))
        if w.shape != (cout, cin, 3, 3) or b.shape != (cout,):
            raise ValueError("layer %d: expected w [%d,%d,3,3] and b [%d], got %s and %s" % (k, cout, cin, cout, w.shape, b.shape))
        check(self._lib.y355_bntrain_load_layer(self._h, k, w.ctypes.data, b.ctypes.data))

    def load_bn(self, k, gamma, beta, running_mean, running_var, num_batches_tracked=0):
        """BatchNorm of layer k = 1..9: four float [cout] arrays and the count"""
        if not 1 <= k <= NUM_BN:
            raise ValueError("BatchNorm exists on layers 1..9, got %d" % k)
        cout = self.layer_shape(k)[0]
        a = [np.ascontiguousarray(np.asarray(v, np.float32)) for v in (gamma, beta, running_mean, running_var)]
        if any(v.shape != (cout,) for v in a):
            raise ValueError("layer %d: expected four arrays [%d], got %s" % (k, cout, [v.shape for v in a]))
        check(self._lib.y355_bntrain_load_bn(self._h, k, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, int(num_batches_tracked)))

    def _pair(self, fn, k):
        cout, cin = self.layer_shape(k)
        w, b = np.empty((cout, cin, 3, 3), np.float32), np.empty((cout,), np.float32)
        check(fn(self._h, k, w.ctypes.data, b.ctypes.data))
        return w, b

    def _channels(self, fn, k, n):
        cout = self.layer_shape(k)[0]
        out = [np.empty((cout,), np.float32) for _ in range(n)]
        check(fn(self._h, k, *[v.ctypes.data for v in out]))
        return tuple(out)

    def get_layer(self, k):
        return self._pair(self._lib.y355_bntrain_get_layer, k)

    def get_momentum(self, k):
        return self._pair(self._lib.y355_bntrain_get_momentum, k)

    def get_grad(self, k):
        return self._pair(self._lib.y355_bntrain_get_grad, k)

    def get_bn(self, k):
        """(gamma, beta, running_mean, running_var, num_batches_tracked) of layer k = 1..9"""
        cout = self.layer_shape(k)[0]
        out = [np.empty((cout,), np.float32) for _ in range(4)]
        n = C.c_int64()
        check(self._lib.y355_bntrain_get_bn(self._h, k, *[v.ctypes.data for v in out], C.byref(n)))
        return tuple(out) + (int(n.value),)

    def get_bn_grad(self, k):
        """(dgamma, dbeta) of the last backward"""
        return self._channels(self._lib.y355_bntrain_get_bn_grad, k, 2)

    def get_bn_momentum(self, k):
        return self._channels(self._lib.y355_bntrain_get_bn_momentum, k, 2)

    def batch_stats(self, k):
        """(mean, biased var, invstd) of layer k = 1..9 in the last forward, float32 [cout]"""
        return self._channels(self._lib.y355_bntrain_get_batch_stats, k, 3)

    def get_packed(self, k):
        """rb(W_k) as the forward reads it: uint16 bf16 bits [cout, cin, 3, 3]"""
        cout, cin = self.layer_shape(k)
        w = np.empty((cout, cin, 3, 3), np.uint16)
        check(self._lib.y355_bntrain_get_packed(self._h, k, w.ctypes.data))
        return w

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

    @classmethod
    def from_model(cls, model, max_batch, lr, momentum=0.9, weight_decay=5e-4, device=None):
        """a trainer with the size, classes, anchors, parameters and buffers of a SlimYOLOv2"""
        anchors = getattr(model, "_anchor_size64", None) or torch.as_tensor(model.anchor_size).double().view(-1, 2).tolist()
        dev = device if device is not None else (model.device if isinstance(model.device, (str, torch.device)) else None)
        t = cls(model.input_size, model.num_classes, anchors, max_batch, lr, momentum, weight_decay, device=dev)
        t.load_state_dict(model.state_dict())
        return t

    # ------------------------------------------------------------------ the step
    def set_lr(self, lr):
        self.lr = float(lr)

    def set_grid(self, input_size):
        """the reference's set_grid (multi-scale training): the size of the following batches, within the constructor's"""
        check(self._lib.y355_bntrain_set_size(self._h, int(input_size[0]), int(input_size[1])))
        self.input_size = [int(input_size[0]), int(input_size[1])]
        self._batch = 0

    def criterion(self):
        """the yolo355.grad.YoloLossGrad of the current size"""
        key = tuple(self.input_size)
        if key not in self._criteria:
            self._criteria[key] = _grad.YoloLossGrad(self.input_size, STRIDE, self.anchor_size, self.num_classes, max_batch=self.max_batch,
                                                     max_labels_per_image=1024, device=self.device)
        return self._criteria[key]

    def _stream(self):
        return _grad._stream(self.device)

    def forward(self, images):
        """images: float32 [B, 3, H, W] on the device.  A forward in train() mode: the running statistics move.  Returns P, fp32
        [B, A(5+C), H/16, W/16], as a view of the handle's own map (valid until the next forward)."""
        if not isinstance(images, torch.Tensor) or images.device != self.device:
            raise ValueError("images: expected a tensor on %s" % (self.device,))
        B = int(images.shape[0])
        if images.dim() != 4 or list(images.shape[1:]) != [3] + self.input_size:
            raise ValueError("expected [B,3,%d,%d], got %s" % (self.input_size[0], self.input_size[1], tuple(images.shape)))
        x = images.detach().to(torch.float32).contiguous()
        self._batch = 0
        check(self._lib.y355_bntrain_forward(self._h, x.data_ptr(), B, self._stream()))
        self._batch, self._held = B, x
        return self.pred()

    def pred(self):
        """P of the last forward, fp32 [B, A(5+C), H/16, W/16]: a view of the handle's own map (no copy)"""
        if self._batch == 0:
            raise RuntimeError("no forward pass has run at this size")
        p = C.c_void_p()
        check(self._lib.y355_bntrain_pred(self._h, C.byref(p)))
        shape = (self._batch, self.num_anchors * (5 + self.num_classes), self.input_size[0] // STRIDE, self.input_size[1] // STRIDE)
        return torch.as_tensor(_grad._DeviceArray(p.value, shape, self), device=self.device)

    def backward(self, dpred):
        """dpred: float32 device tensor of P's shape; leaves the gradients in the handle"""
        d = dpred.detach().to(device=self.device, dtype=torch.float32).contiguous()
        check(self._lib.y355_bntrain_backward(self._h, d.data_ptr(), self._stream()))
        self._held_d = d

    def _plan_batch(self, batch):
        if batch is None:
            if self._batch == 0:
                raise RuntimeError("no forward pass has run at this size")
            batch = self._batch
        return int(batch)

    def wgrad_plan(self, k, batch=None):
        """How the backward splits layer k's weight gradient at the current size: dict(npix, max_runs, runs, chunk), as
        SlimTrainer.wgrad_plan.  batch: None for that of the last forward."""
        s = (C.c_int32 * 4)()
        check(self._lib.y355_bntrain_wgrad_plan(self._h, int(k), self._plan_batch(batch), s))
        return dict(npix=int(s[0]), max_runs=int(s[1]), runs=int(s[2]), chunk=int(s[3]))

    def stats_plan(self, k, batch=None):
        """How forward and backward cut the BatchNorm reductions of layer k = 1..9 at the current size: dict(N, runs, chunk) --
        runs workgroup runs of chunk pixels each, the last one the rest (y355_bntrain_stats_plan, what the passes launch from)"""
        s = (C.c_int32 * 3)()
        check(self._lib.y355_bntrain_stats_plan(self._h, int(k), self._plan_batch(batch), s))
        return dict(N=int(s[0]), runs=int(s[1]), chunk=int(s[2]))

    def forward_backward(self, images, label_lists=None, target=None):
        """One forward, the loss and the backward pass -> (conf_loss, cls_loss, txtytwth_loss, total_loss) as tools.loss returns
        them (0-dim float32 tensors); the gradients stay in the handle (gradients()).  label_lists: per image
        [[xmin, ymin, xmax, ymax, cls], ...]; or target: dense [B, N, 11] as tools.gt_creator makes it; or neither: the labels
        of the last call."""
        if label_lists is not None and target is not None:
            raise ValueError("give label_lists or target, not both")
        pred = self.forward(images)
        crit = self.criterion()
        if label_lists is not None:
            if len(label_lists) != pred.shape[0]:
                raise ValueError("%d label lists for a batch of %d" % (len(label_lists), pred.shape[0]))
            crit.set_labels(label_lists)
        if self._dpred is None or self._dpred.shape != pred.shape:
            self._dpred = torch.empty_like(pred)
        out, self.per_image, _ = crit.forward_backward([pred], target=target, grad_maps=[self._dpred])
        self.losses = out
        self.backward(self._dpred)
        return _grad._loss_tensors(out, self.device)

    def update(self):
        """optimizer.step() and zero_grad() on every parameter (W, b, gamma, beta); the running statistics stay"""
        check(self._lib.y355_bntrain_sgd_step(self._h, self.lr, self.momentum, self.weight_decay, self._stream()))

    def step(self, images, label_lists=None, target=None):
        """forward_backward, then the update; returns the four losses (of the parameters before the update)"""
        out = self.forward_backward(images, label_lists, target)
        self.update()
        return out

    def step_frame_list(self, frames, labels, seed=None):
        """SSDAugmentation on a list of camera frames (yolo355.augment.augment_frame_list), then step() on the augmented
        batch and its labels, as SlimTrainer.step_frame_list"""
        from . import augment
        rng = None if seed is None else np.random.RandomState(seed)
        x, targets, _ = augment.augment_frame_list(frames, labels, self.input_size, rng=rng, device=self.device)
        return self.step(x, [np.asarray(t, np.float64).reshape(-1, 5).tolist() for t in targets])

    def gradients(self):
        """{key: float32 array} of the last backward pass, under the state_dict's parameter keys"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            out[kw], out[kb] = self.get_grad(k)
            if k <= NUM_BN:
                out[bn_keys(k)[0]], out[bn_keys(k)[1]] = self.get_bn_grad(k)
        return out

    # ------------------------------------------------------------------ taps (tests)
    def get_tensor(self, kind, t):
        """tensor t of a kind (ACT: A_t, Z: Z_t, DY: dY_t, GRAD: G_t as bf16 bits; IDX: I_t uint8) as a numpy array in NCHW order"""
        s = (C.c_int32 * 4)()
        check(self._lib.y355_bntrain_tensor_shape(self._h, kind, t, s))
        a = np.empty(tuple(int(v) for v in s), np.uint8 if kind == IDX else np.uint16)
        check(self._lib.y355_bntrain_get_tensor(self._h, kind, t, a.ctypes.data))
        return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))

    def close(self):
        for c in getattr(self, "_criteria", {}).values():
            c.close()
        self._criteria = {}
        super().close()
