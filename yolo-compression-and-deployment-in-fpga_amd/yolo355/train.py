"""Fine-tuning of the BN-folded SlimYOLOv2 (SlimYOLOv2_quantize_bnfuse, the network retune_bias_quantize.py trains without
-q) on the GPU: ctypes binding of include/yolo355_train.h (csrc/train.hip, the companion library libyolo355_train.so, loaded
the first time it is asked for) and SlimTrainer, one object for the reference's loop body -- forward, tools.loss,
total_loss.backward(), optim.SGD(lr, momentum, weight_decay).step(), zero_grad().  The loss and its gradient with respect to
the prediction map are yolo355.grad's (libyolo355_grad.so); the prediction and gradient maps never leave the device.  The
arithmetic contract is DESIGN.md section 6m.  The loop body itself is yolo355._trainer.Trainer's, which SlimBNTrainer
(yolo355.bntrain) shares.  No CPU path: without a GPU every entry point raises."""
import os

import torch

from . import _ffi
from ._trainer import ACT, GRAD, IDX, LAYER_NAMES, NUM_LAYERS, POOLED, STRIDE, Trainer, _np, common_sigs, layer_keys  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_train.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_train.h"))

_SIGS = common_sigs("y355_train_")
_lib = None
# libyolo355_train.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_train_", "extensions first (make -C csrc)")


class SlimTrainer(Trainer):
    """The training step of SlimYOLOv2_quantize_bnfuse(trainable=True) with torch.optim.SGD(lr, momentum, weight_decay).
    input_size [H, W] (multiples of 16) is the largest size the trainer takes; set_grid switches within it."""
    _destroy = "y355_train_destroy"
    _prefix, _lib_fn, _check = "y355_train_", staticmethod(lib), staticmethod(check)

    def load_weights(self, weights):
        """[(name, w, b)] of synth.make_weights, or [(w, b)], layers 1..10"""
        for k, L in enumerate(weights, 1):
            self.load_layer(k, L[-2], L[-1])

    def load_state_dict(self, sd):
        """a state_dict in the reference's key layout (convK.convs.0.{weight,bias}, pred.{weight,bias}): a *_bnfuse.pth; other
        keys (the trackers' buffers) are ignored"""
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            if kw not in sd or kb not in sd:
                raise KeyError("state_dict lacks %s / %s" % (kw, kb))
            self.load_layer(k, _np(sd[kw]), _np(sd[kb]))

    def state_dict(self):
        """the fp32 master parameters as CPU torch tensors under the reference's keys"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            w, b = self.get_layer(k)
            kw, kb = layer_keys(k)
            out[kw], out[kb] = torch.from_numpy(w), torch.from_numpy(b)
        return out

    def gradients(self):
        """{key: float32 array} of the last backward pass, under the state_dict's keys"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            out[kw], out[kb] = self.get_grad(k)
        return out
