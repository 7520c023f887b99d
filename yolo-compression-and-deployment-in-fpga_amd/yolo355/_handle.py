"""What every Python handle over the C ABI shares (engine.Engine / Pipeline, netengine.Net, ops.ConvOp, apeval.ApEval): the
ownership of the C handle and its place in the interpreter-exit order, the ordering against the construction-time stream, and
the marshalling of configurations, inputs, weights and detection outputs -- each written once."""
import atexit
import ctypes as C
import weakref

import numpy as np
import torch

from . import _ffi, framelist

# Handles that own HIP streams / events must be destroyed while the HIP runtime is still alive: at interpreter shutdown the
# order of module teardown is arbitrary, and a __del__ that reaches hipStreamDestroy after the runtime's own atexit handlers
# have run crashes the process.  Every live owning Handle is closed from one atexit hook registered at import (i.e. after
# torch's and before its teardown, atexit being LIFO).
_live = weakref.WeakSet()


@atexit.register
def _close_all():
    for o in list(_live):
        try:
            o.close()
        except Exception:
            pass


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise RuntimeError("yolo355 needs an MI355X (HIP) device; no GPU is visible and there is no CPU fallback")
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda":
        raise RuntimeError("yolo355 engines live on a GPU; got device %r" % (device,))
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


class Handle:
    """A handle of the C ABI: _h, the library _lib, and _destroy, the name of the symbol that frees it.  close() is
    idempotent and leaves a handle somebody else owns (Engine._borrowed) alone; owning handles are closed at exit (_live)."""
    _h = None                   # until _own: close() and __del__ are safe on an object whose constructor raised
    _destroy = None

    def _own(self, lib, h, owned=True):
        self._lib, self._h, self._owned = lib, h, owned
        if owned:
            _live.add(self)

    def close(self):
        if self._h is not None:
            if self._owned:
                getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamBound:
    """A Handle whose kernels all go to the stream that was current when it was built (the C ABI takes the stream at
    creation).  A caller that has since switched streams (`with torch.cuda.stream(s)`) is ordered explicitly: the handle's
    stream waits for the caller's pending work before a launch, and the caller's stream waits for the handle's before it
    reads results.  Same stream: no-ops.  The class sets device, max_batch, max_det and _out (None)."""

    def _create(self, lib, cfg, create):
        """create(cfg) -> the owned handle, on torch's current stream (handle 0 = the default stream), so that torch copies /
        allocations and the handle's kernels are ordered without extra syncs"""
        with torch.cuda.device(self.device):
            self._stream = torch.cuda.current_stream(self.device)
            cfg.stream = C.c_void_p(self._stream.cuda_stream)
            cfg.own_stream = 0
            h = C.c_void_p()
            _ffi.check(create(C.byref(cfg), C.byref(h)))
        self._own(lib, h)

    def _enter(self):
        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)
        return cur

    def _leave(self, cur):
        if cur != self._stream:
            cur.wait_stream(self._stream)

    def _call(self, fn, *args):
        cur = self._enter()
        _ffi.check(fn(self._h, *args))
        self._leave(cur)

    def _frame_list(self, frames):
        """(y355_frame array, B, sizes) of framelist.frame_list on the handle's stream.  Every tensor the launch reads is
        held until this handle's next list call."""
        arr, B, sizes, self._held_frames = framelist.frame_list(frames, self.max_batch, self.device, self._stream)
        return arr, B, sizes

    def _buffers(self, B):
        """the handle's own output tensors (out_buffers for max_batch images; dropped when max_det changes)"""
        if self._out is None:
            self._out = out_buffers(self.max_batch, self.max_det, self.device)
        return self._out

    def _launch(self, fn, head, B, flags, out, tail=()):
        """one forward of the C ABI, fn(handle, *head, B, flags, boxes, scores, cls, count, *tail), into `out` or the handle's
        own buffers; returns the four device tensors"""
        ob, os_, oc, on = out if out is not None else self._buffers(B)
        self._call(fn, *head, B, int(flags), ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), on.data_ptr(), *tail)
        return ob, os_, oc, on


def fill_config(cfg, device, input_size, num_classes, anchors, conf, nms, max_batch, max_det):
    """the fields y355_config and y355_net_config share"""
    cfg.device_id = device.index
    cfg.height, cfg.width = input_size
    cfg.num_classes = num_classes
    cfg.num_anchors = len(anchors)
    for i, (w, h) in enumerate(anchors):
        cfg.anchors[2 * i], cfg.anchors[2 * i + 1] = w, h
    cfg.conf_thresh, cfg.nms_thresh = float(conf), float(nms)
    cfg.max_batch, cfg.max_det = max_batch, int(max_det)


def out_buffers(max_batch, max_det, device):
    """(boxes [max_batch,max_det,4], scores, cls int32, count int32) device tensors for a forward to fill"""
    return (torch.empty((max_batch, max_det, 4), dtype=torch.float32, device=device),
            torch.empty((max_batch, max_det), dtype=torch.float32, device=device),
            torch.empty((max_batch, max_det), dtype=torch.int32, device=device),
            torch.zeros((max_batch,), dtype=torch.int32, device=device))


def dev_input(x, input_size, device, max_batch=None):
    """a batch [B,3,H,W] (numpy or torch) at the network size as a contiguous float32 tensor on device"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if x.dim() != 4 or x.shape[1] != 3 or list(x.shape[2:]) != input_size:
        raise ValueError("expected [B,3,%d,%d], got %s" % (input_size[0], input_size[1], tuple(x.shape)))
    if max_batch is not None and x.shape[0] > max_batch:
        raise ValueError("batch %d > max_batch %d" % (x.shape[0], max_batch))
    return x.to(device=device, dtype=torch.float32).contiguous()


def i8_layer(q_w, q_b):
    """(q_w int8, q_b int32) contiguous; the range of q_w is checked on the caller's array, before the cast wraps it"""
    if np.abs(np.asarray(q_w)).max() > 127:
        raise ValueError("|q_w| > 127")
    return np.ascontiguousarray(q_w, dtype=np.int8), np.ascontiguousarray(q_b, dtype=np.int32)


def float3_pair(mean_bgr, std_bgr):
    return (C.c_float * 3)(*[float(v) for v in mean_bgr]), (C.c_float * 3)(*[float(v) for v in std_bgr])


def _host(a, B):
    return a[:B].cpu().numpy() if isinstance(a, torch.Tensor) else a[:B]


def split_dets(boxes, scores, cls, count, B):
    """The reference's eval-mode return for the first B images of a forward's outputs (torch tensors on any device, or numpy
    arrays): list of (bboxes float32 [n,4], scores float32 [n], cls_inds int64 [n]), each owning its memory."""
    b, s, c, n = _host(boxes, B), _host(scores, B), _host(cls, B), _host(count, B)
    return [(b[i, :n[i]].copy(), s[i, :n[i]].copy(), c[i, :n[i]].astype(np.int64)) for i in range(B)]


def raise_if_guard(guard):
    """find=True: a forward's count of conv outputs beyond the 16-bit head-room, as the reference raises it"""
    if guard:
        print("too high!!!")
        raise AssertionError("conv output exceeds the 16-bit head-room (find=True): %d positions" % guard)


def _overflow_message(cap):
    return "more than %d anchors of an image pass conf_thresh: raise the threshold%s" % (cap, " or max_candidates" if cap > 4096 else "")


def raise_overflow(cap):
    """a forward dropped candidates beyond the capacity `cap` (max_candidates)"""
    raise _ffi.Y355Error(-1, _overflow_message(cap))
