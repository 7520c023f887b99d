"""What the trainers share (train.SlimTrainer over include/yolo355_train.h, bntrain.SlimBNTrainer over
include/yolo355_bntrain.h, qtrain.SlimQatTrainer over include/yolo355_qtrain.h): the seventeen entry points the headers declare under their own prefix (common_sigs), the layer
names of the network, and Trainer, the handle with the reference's loop body -- parameters in and out per layer, forward, the
loss and its gradient of yolo355.grad, backward, the SGD update -- written once.  A trainer class names its prefix and its
binding module's lib and check (_prefix, _lib_fn, _check) and adds what is its own."""
import ctypes as C

import numpy as np
import torch

from ._handle import Handle, _require_gpu
from . import grad as _grad

P = C.POINTER
_V, _I = C.c_void_p, C.c_int32

NUM_LAYERS = 10
ACT, IDX, GRAD = 0, 1, 2
# the reference's module names (models/slim_yolo_v2.py:59-87), layers 1..10
LAYER_NAMES = ["conv1", "conv2", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5", "conv6", "conv7", "pred"]
POOLED = (1, 2, 4, 6)
STRIDE = 16


def common_sigs(prefix):
    """{name: (restype, argtypes)} of the entry points yolo355_train.h and yolo355_bntrain.h both declare"""
    rows = {
        "last_error": (C.c_char_p, []),
        "create": (C.c_int, [_I, _I, _I, _I, _I, P(_V)]),
        "destroy": (None, [_V]),
        "set_size": (C.c_int, [_V, _I, _I]),
        "load_layer": (C.c_int, [_V, _I, _V, _V]),
        "get_layer": (C.c_int, [_V, _I, _V, _V]),
        "layer_shape": (C.c_int, [_V, _I, P(_I)]),
        "forward": (C.c_int, [_V, _V, _I, _V]),
        "pred": (C.c_int, [_V, P(_V)]),
        "backward": (C.c_int, [_V, _V, _V]),
        "get_grad": (C.c_int, [_V, _I, _V, _V]),
        "get_momentum": (C.c_int, [_V, _I, _V, _V]),
        "get_packed": (C.c_int, [_V, _I, _V]),
        "wgrad_plan": (C.c_int, [_V, _I, _I, P(_I)]),
        "sgd_step": (C.c_int, [_V, C.c_float, C.c_float, C.c_float, _V]),
        "tensor_shape": (C.c_int, [_V, _I, _I, P(_I)]),
        "get_tensor": (C.c_int, [_V, _I, _I, _V]),
    }
    return {prefix + name: sig for name, sig in rows.items()}


def layer_keys(k):
    """(weight key, bias key) of layer k = 1..10 in the reference's state_dict"""
    n = LAYER_NAMES[k - 1]
    return (n + ".weight", n + ".bias") if n == "pred" else (n + ".convs.0.weight", n + ".convs.0.bias")


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


class Trainer(Handle):
    """A training step with torch.optim.SGD(lr, momentum, weight_decay) behind one of the two C ABIs.  input_size [H, W]
    (multiples of 16) is the largest size the trainer takes; set_grid switches within it."""
    _prefix = None              # of the entry points, "y355_train_" / "y355_bntrain_" / "y355_qtrain_"
    _lib_fn = _check = None     # the binding module's lib and check (staticmethod)

    def __init__(self, input_size, num_classes, anchor_size, max_batch, lr, momentum=0.9, weight_decay=5e-4, device=None):
        l = self._lib_fn()
        self.device = _require_gpu(device)
        self.max_size = [int(input_size[0]), int(input_size[1])]
        self.input_size = list(self.max_size)
        self.num_classes, self.max_batch = int(num_classes), int(max_batch)
        self.anchor_size = [[float(v) for v in a] for a in np.asarray(anchor_size, np.float64).reshape(-1, 2)]
        self.num_anchors = len(self.anchor_size)
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            self._check(getattr(l, self._prefix + "create")(self.max_size[0], self.max_size[1], self.num_classes, self.num_anchors, self.max_batch,
                                                            C.byref(h)))
        self._own(l, h)
        self._criteria = {}
        self._dpred = None
        self._batch = 0

    def _call(self, name, *args):
        """<prefix><name>(handle, *args), checked"""
        self._check(getattr(self._lib, self._prefix + name)(self._h, *args))

    # ------------------------------------------------------------------ parameters
    def layer_shape(self, k):
        s = (C.c_int32 * 2)()
        self._call("layer_shape", k, s)
        return int(s[0]), int(s[1])

    def load_layer(self, k, w, b):
        cout, cin = self.layer_shape(k)
        w = np.ascontiguousarray(np.asarray(w, np.float32))
        b = np.ascontiguousarray(np.asarray(b, np.float32))
        if w.shape != (cout, cin, 3, 3) or b.shape != (cout,):
            raise ValueError("layer %d: expected w [%d,%d,3,3] and b [%d], got %s and %s" % (k, cout, cin, cout, w.shape, b.shape))
        self._call("load_layer", k, w.ctypes.data, b.ctypes.data)

    def _pair(self, name, k):
        cout, cin = self.layer_shape(k)
        w, b = np.empty((cout, cin, 3, 3), np.float32), np.empty((cout,), np.float32)
        self._call(name, k, w.ctypes.data, b.ctypes.data)
        return w, b

    def get_layer(self, k):
        return self._pair("get_layer", k)

    def get_momentum(self, k):
        return self._pair("get_momentum", k)

    def get_grad(self, k):
        return self._pair("get_grad", k)

    def get_packed(self, k):
        """rb(W_k) as the forward reads it: uint16 bf16 bits [cout, cin, 3, 3]"""
        cout, cin = self.layer_shape(k)
        w = np.empty((cout, cin, 3, 3), np.uint16)
        self._call("get_packed", k, w.ctypes.data)
        return w

    @classmethod
    def from_model(cls, model, max_batch, lr, momentum=0.9, weight_decay=5e-4, device=None):
        """a trainer with the size, classes, anchors and state_dict of the reference's model"""
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
        self._call("set_size", int(input_size[0]), int(input_size[1]))
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
        """images: float32 [B, 3, H, W] on the device (what augment_frame_list returns).  Returns P, fp32 [B, A(5+C), H/16, W/16],
        as a view of the handle's own map (valid until the next forward)."""
        if not isinstance(images, torch.Tensor) or images.device != self.device:
            raise ValueError("images: expected a tensor on %s" % (self.device,))
        B = int(images.shape[0])
        if images.dim() != 4 or list(images.shape[1:]) != [3] + self.input_size:
            raise ValueError("expected [B,3,%d,%d], got %s" % (self.input_size[0], self.input_size[1], tuple(images.shape)))
        x = images.detach().to(torch.float32).contiguous()
        self._batch = 0
        self._call("forward", x.data_ptr(), B, self._stream())
        self._batch, self._held = B, x
        return self.pred()

    def pred(self):
        """P of the last forward, fp32 [B, A(5+C), H/16, W/16]: a view of the handle's own map (no copy)"""
        if self._batch == 0:
            raise RuntimeError("no forward pass has run at this size")
        p = C.c_void_p()
        self._call("pred", C.byref(p))
        shape = (self._batch, self.num_anchors * (5 + self.num_classes), self.input_size[0] // STRIDE, self.input_size[1] // STRIDE)
        return torch.as_tensor(_grad._DeviceArray(p.value, shape, self), device=self.device)

    def backward(self, dpred):
        """dpred: float32 device tensor of P's shape; leaves the gradients in the handle"""
        d = dpred.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self._call("backward", d.data_ptr(), self._stream())
        self._held_d = d

    def _plan_batch(self, batch):
        if batch is None:
            if self._batch == 0:
                raise RuntimeError("no forward pass has run at this size")
            batch = self._batch
        return int(batch)

    def wgrad_plan(self, k, batch=None):
        """How the backward splits layer k's weight gradient at the current size: dict(npix, max_runs, runs, chunk) -- runs
        workgroup runs of chunk pixels each, the last one the rest (<prefix>wgrad_plan, what the backward itself launches
        from).  batch: None for that of the last forward."""
        s = (C.c_int32 * 4)()
        self._call("wgrad_plan", int(k), self._plan_batch(batch), s)
        return dict(npix=int(s[0]), max_runs=int(s[1]), runs=int(s[2]), chunk=int(s[3]))

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
        """optimizer.step() and zero_grad() on every parameter"""
        self._call("sgd_step", self.lr, self.momentum, self.weight_decay, self._stream())

    def step(self, images, label_lists=None, target=None):
        """forward_backward, then the update; returns the four losses (of the parameters before the update)"""
        out = self.forward_backward(images, label_lists, target)
        self.update()
        return out

    def step_frame_list(self, frames, labels, seed=None):
        """SSDAugmentation on a list of camera frames (yolo355.augment.augment_frame_list), then step() on the augmented
        batch and its labels: the pixels never visit the host.  labels[i]: float [n_i, 5] = (xmin, ymin, xmax, ymax, cls);
        seed: of the augmentation's draws (None: numpy's global stream, as in the reference)."""
        from . import augment
        rng = None if seed is None else np.random.RandomState(seed)
        x, targets, _ = augment.augment_frame_list(frames, labels, self.input_size, rng=rng, device=self.device)
        return self.step(x, [np.asarray(t, np.float64).reshape(-1, 5).tolist() for t in targets])

    # ------------------------------------------------------------------ taps (tests)
    def get_tensor(self, kind, t):
        """tensor t of a kind (ACT: A_t bf16 bits, IDX: I_t uint8, GRAD: G_t bf16 bits) as a numpy array in NCHW order"""
        s = (C.c_int32 * 4)()
        self._call("tensor_shape", kind, t, s)
        a = np.empty(tuple(int(v) for v in s), np.uint8 if kind == IDX else np.uint16)
        self._call("get_tensor", kind, t, a.ctypes.data)
        return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))

    def close(self):
        for c in getattr(self, "_criteria", {}).values():
            c.close()
        self._criteria = {}
        super().close()
