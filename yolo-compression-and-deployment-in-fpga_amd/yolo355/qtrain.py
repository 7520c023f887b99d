"""Quantisation-aware fine-tuning of the BN-folded SlimYOLOv2 on the GPU: ctypes binding of include/yolo355_qtrain.h
(csrc/qtrain.hip, the companion library libyolo355_qtrain.so, loaded the first time it is asked for) and SlimQatTrainer, the
loop body of yolo355.train.SlimTrainer whose forward is the network the int8 engine deploys -- power-of-two 8-bit weights,
biases and activations, computed as a fake quantisation in fp32, bit for bit -- and whose backward is the straight-through
estimator.  The reference has no such step: its activation quantiser builds a new leaf under torch.no_grad()
(models/slim_yolo_v2.py:21-38), so retune_bias_quantize.py -q can only calibrate.  quantized_layers() and act_exponents() hand
the trained network to yolo355.engine.Engine (load_quantized, set_act_exponents).  The arithmetic contract is DESIGN.md
section 6o.  No CPU path: without a GPU every device entry point raises."""
import ctypes as C
import os

import numpy as np
import torch

from . import _ffi
from ._trainer import ACT, GRAD, IDX, LAYER_NAMES, NUM_LAYERS, POOLED, STRIDE, Trainer, _np, common_sigs, layer_keys  # noqa: F401

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_qtrain.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_qtrain.h"))

P = C.POINTER
_V, _I = C.c_void_p, C.c_int32
_SIGS = dict(common_sigs("y355_qtrain_"), **{
    "y355_qtrain_set_act_exponents": (C.c_int, [_V, P(_I)]),
    "y355_qtrain_get_act_exponents": (C.c_int, [_V, P(_I)]),
    "y355_qtrain_get_act_stats": (C.c_int, [_V, _V, _V]),
    "y355_qtrain_get_weight_exponents": (C.c_int, [_V, P(_I)]),
    "y355_qtrain_get_qbias": (C.c_int, [_V, _I, _V]),
})
_lib = None
# libyolo355_qtrain.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_qtrain_", "extensions first (make -C csrc)")

NUM_TRACKERS = 11
STATE = 3
S_POS, S_NEG, S_CLIP = 3, 4, 8
MAX_ACT_EXPONENT = 96
# the trackers' module names in the reference's checkpoint (models/slim_yolo_v2.py:58-89), trackers 0..10
TRACKER_NAMES = ["a_tracker_in", "a_tracker1", "a_tracker2", "a_tracker3_1", "a_tracker3_2", "a_tracker4_1", "a_tracker4_2", "a_tracker5",
                 "a_tracker6", "a_tracker7", "a_tracker_pred"]


def bf16_to_f32(bits):
    """float32 array of bf16 bit patterns (uint16)"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _exponent_list(source):
    """eleven activation exponents from a list of ints, a list of prep.RangeTracker, an Engine (get_act_exponents) or a
    calibrated state_dict (the a_tracker*.scale buffers)"""
    from . import prep
    if hasattr(source, "get_act_exponents"):
        source = source.get_act_exponents()
    elif hasattr(source, "keys"):
        missing = [n + ".scale" for n in TRACKER_NAMES if n + ".scale" not in source]
        if missing:
            raise KeyError("state_dict lacks %s" % ", ".join(missing))
        source = [prep.RangeTracker(scale=torch.as_tensor(_np(source[n + ".scale"])), first_a=1) for n in TRACKER_NAMES]
    out = [int(v.exponent()) if isinstance(v, prep.RangeTracker) else int(v) for v in source]
    if len(out) != NUM_TRACKERS:
        raise ValueError("expected %d activation exponents, got %d" % (NUM_TRACKERS, len(out)))
    return out


class SlimQatTrainer(Trainer):
    """SlimTrainer's step on the quantised network: fp32 masters, a forward that equals the int8 engine's feature maps, a
    straight-through backward, SGD on the masters.  The activation exponents are frozen values (set_act_exponents; a forward
    is refused until they are set); update_trackers() moves them between steps."""
    _destroy = "y355_qtrain_destroy"
    _prefix, _lib_fn, _check = "y355_qtrain_", staticmethod(lib), staticmethod(check)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.trackers = None

    # ------------------------------------------------------------------ parameters
    def load_weights(self, weights):
        """[(name, w, b)] of synth.make_weights, or [(w, b)], layers 1..10"""
        for k, L in enumerate(weights, 1):
            self.load_layer(k, L[-2], L[-1])

    def load_state_dict(self, sd):
        """a state_dict in the reference's key layout (convK.convs.0.{weight,bias}, pred.{weight,bias}): a *_bnfuse.pth, as
        fp32 masters; where it holds every a_tracker*.scale buffer (a calibrated checkpoint) the trackers and the activation
        exponents are taken from them; other keys are ignored"""
        from . import prep
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            if kw not in sd or kb not in sd:
                raise KeyError("state_dict lacks %s / %s" % (kw, kb))
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            self.load_layer(k, _np(sd[kw]), _np(sd[kb]))
        if all(n + ".scale" in sd for n in TRACKER_NAMES):
            tr = []
            for n in TRACKER_NAMES:
                first = int(_np(sd[n + ".first_a"]).reshape(-1)[0]) if n + ".first_a" in sd else 1
                tr.append(prep.RangeTracker(scale=torch.as_tensor(_np(sd[n + ".scale"])), first_a=first))
            if all(t.first_a for t in tr):
                self.set_act_exponents(tr)

    def state_dict(self):
        """the fp32 master parameters as CPU torch tensors under the reference's keys, and the trackers' buffers where the
        trainer holds trackers"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            w, b = self.get_layer(k)
            kw, kb = layer_keys(k)
            out[kw], out[kb] = torch.from_numpy(w), torch.from_numpy(b)
        if self.trackers is not None:
            for n, t in zip(TRACKER_NAMES, self.trackers):
                out[n + ".scale"] = t.scale.clone()
                out[n + ".first_a"] = torch.tensor([float(t.first_a)])
        return out

    def gradients(self):
        """{key: float32 array} of the last backward pass, under the state_dict's parameter keys"""
        out = {}
        for k in range(1, NUM_LAYERS + 1):
            kw, kb = layer_keys(k)
            out[kw], out[kb] = self.get_grad(k)
        return out

    # ------------------------------------------------------------------ the quantiser
    def set_act_exponents(self, source):
        """the frozen activation exponents e_a[0..10] of the following forwards: eleven ints, eleven prep.RangeTracker (kept:
        update_trackers moves them), an Engine (its get_act_exponents()), or a calibrated state_dict"""
        from . import prep
        e = _exponent_list(source)
        self._call("set_act_exponents", (C.c_int32 * NUM_TRACKERS)(*e))
        if not hasattr(source, "keys") and not hasattr(source, "get_act_exponents") and all(isinstance(v, prep.RangeTracker) for v in source):
            self.trackers = list(source)

    def act_exponents(self):
        """the eleven exponents the next forward uses, for Engine.set_act_exponents"""
        e = (C.c_int32 * NUM_TRACKERS)()
        self._call("get_act_exponents", e)
        return [int(v) for v in e]

    def act_stats(self):
        """(max_abs float32 [11], clipped int64 [11]) of the last forward: per tracker the batch's max|v| before quantisation and
        the number of elements with |rne(v 2^e)| > 127, counted before the pool"""
        mx, n = np.empty(NUM_TRACKERS, np.float32), np.empty(NUM_TRACKERS, np.int64)
        self._call("get_act_stats", mx.ctypes.data, n.ctypes.data)
        return mx, n

    def update_trackers(self, freeze=False):
        """feeds the last forward's maxima to the host trackers (prep.RangeTracker.update: first call, frozen or moving
        average) and sets the resulting exponents for the next forward -- one step later than the reference's forward, which
        quantises a map with the scale that map's own maximum has just moved.  Returns the exponents."""
        from . import prep
        if self.trackers is None:
            self.trackers = [prep.RangeTracker() for _ in range(NUM_TRACKERS)]
        mx, _ = self.act_stats()
        e = [t.update(float(m), freeze) for t, m in zip(self.trackers, mx)]
        self._call("set_act_exponents", (C.c_int32 * NUM_TRACKERS)(*e))
        return e

    def weight_exponents(self):
        """[(e_w, e_b)] of layers 1..10 as the device computed them from the masters"""
        e = (C.c_int32 * (2 * NUM_LAYERS))()
        self._call("get_weight_exponents", e)
        return [(int(e[2 * k]), int(e[2 * k + 1])) for k in range(NUM_LAYERS)]

    def get_qbias(self, k):
        """bq_k, float32 [cout]"""
        b = np.empty((self.layer_shape(k)[0],), np.float32)
        self._call("get_qbias", k, b.ctypes.data)
        return b

    def quantized_layers(self):
        """[{q_w, e_w, q_b, e_b}] of layers 1..10, the integers the forward computes with: what prep.quantize_folded gives on
        state_dict()'s masters, ready for Engine.load_quantized"""
        out = []
        for k, (ew, eb) in enumerate(self.weight_exponents(), 1):
            qw = np.rint(np.ldexp(bf16_to_f32(self.get_packed(k)).astype(np.float64), ew)).astype(np.int32)
            qb = np.rint(np.ldexp(self.get_qbias(k).astype(np.float64), eb)).astype(np.int32)
            out.append(dict(q_w=qw, e_w=ew, q_b=qb, e_b=eb))
        return out

    # ------------------------------------------------------------------ taps (tests)
    def get_tensor(self, kind, t):
        """tensor t of a kind (ACT: A_t, GRAD: G_t as bf16 bits; STATE: S_t uint8, IDX: S_t of a pooled layer) as a numpy array
        in NCHW order"""
        s = (C.c_int32 * 4)()
        self._call("tensor_shape", kind, t, s)
        a = np.empty(tuple(int(v) for v in s), np.uint8 if kind in (IDX, STATE) else np.uint16)
        self._call("get_tensor", kind, t, a.ctypes.data)
        return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))
