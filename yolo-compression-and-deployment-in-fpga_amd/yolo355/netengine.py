"""Python handle over the y355_net_* C ABI (include/yolo355.h): the table-driven executor of
csrc/net.hip for SlimYOLOv2 (fp32 model -> bf16 MFMA), YOLOv3tiny, YOLOv2, YOLOv3 and YOLOv3-SPP, in bf16 or int8.  PyTorch is used for
device memory and the stream only; all compute is in libyolo355.so."""
import ctypes as C

import numpy as np
import torch

from . import _ffi, framelist
from ._handle import (Handle, StreamBound, _require_gpu, dev_input, fill_config, float3_pair, i8_layer, raise_overflow, split_dets)

ARCH = {"slim_yolo_v2": _ffi.ARCH_SLIM_V2, "tiny_yolo_v3": _ffi.ARCH_TINY_V3, "yolo_v2": _ffi.ARCH_YOLO_V2,
        "yolo_v3": _ffi.ARCH_YOLO_V3, "yolo_v3_spp": _ffi.ARCH_YOLO_V3_SPP}
NLEV = {"slim_yolo_v2": 1, "tiny_yolo_v3": 2, "yolo_v2": 1, "yolo_v3": 3, "yolo_v3_spp": 3}
DTYPE = {"int8": _ffi.DT_INT8, "bf16": _ffi.DT_BF16}
# prediction maps (fp32 in bf16 nets) by their index from the end of the tensor list (graph order of csrc/net.hip)
PRED_TAIL = {"slim_yolo_v2": (1,), "tiny_yolo_v3": (2, 1), "yolo_v2": (1,), "yolo_v3": (5, 3, 1), "yolo_v3_spp": (5, 3, 1)}


class Net(StreamBound, Handle):
    _destroy = "y355_net_destroy"

    def __init__(self, arch, input_size, num_classes, anchors, conf_thresh=0.01, nms_thresh=0.5,
                 max_batch=1, max_det=0, device=None, dtype="bf16", max_candidates=None, head_route=None):
        """anchors: [[w, h], ...] -- A pairs for slim_yolo_v2 (grid units), 2*A pairs for tiny_yolo_v3
        (pixels; the stride-16 level first, data/config.py:27-31).  max_candidates (default 4096, up to min(anchors per
        image, 65536)): the most anchors of an image that may pass conf_thresh; head_route 1: every image through the NMS route
        for more than 4096 candidates (Y355_NET_OPT_MAX_CANDIDATES / Y355_NET_OPT_HEAD_ROUTE)."""
        lib = _ffi.lib()
        self.device = _require_gpu(device)
        self.arch = arch
        self.input_size = [int(input_size[0]), int(input_size[1])]
        self.num_classes = int(num_classes)
        self.anchors = [[float(a), float(b)] for a, b in anchors]
        nlev = NLEV[arch]
        if len(self.anchors) % nlev:
            raise ValueError("%s needs a multiple of %d anchors" % (arch, nlev))
        self.max_batch = int(max_batch)
        cfg = _ffi.NetConfig()
        cfg.arch, cfg.dtype = ARCH[arch], DTYPE[dtype]
        if len(self.anchors) > _ffi.MAX_ANCHORS:
            raise ValueError("too many anchors")
        fill_config(cfg, self.device, self.input_size, self.num_classes, self.anchors, conf_thresh, nms_thresh, self.max_batch, max_det)
        cfg.num_anchors = len(self.anchors) // nlev       # per level; the anchor array holds every level's
        self._create(lib, cfg, lib.y355_net_create)
        h = self._h
        self.max_det = lib.y355_net_max_det(h)
        self.num_anchors_total = lib.y355_net_num_anchors_total(h)
        self.num_layers = lib.y355_net_num_layers(h)
        self.num_tensors = lib.y355_net_num_tensors(h)
        self._out = None
        if max_candidates is not None:
            self.set_max_candidates(max_candidates)
        if head_route is not None:
            self.set_head_route(head_route)

    def layer_shape(self, idx):
        s = (C.c_int32 * 4)()
        _ffi.check(self._lib.y355_net_layer_shape(self._h, idx, s))
        return tuple(s)

    def tensor_shape(self, idx):
        s = (C.c_int32 * 3)()
        _ffi.check(self._lib.y355_net_tensor_shape(self._h, idx, s))
        return tuple(s)

    def load_layer(self, idx, w, b=None):
        """w fp32 [cout,cin,k,k] (BN already folded), b fp32 [cout] or None."""
        w = np.ascontiguousarray(w, dtype=np.float32)
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
        _ffi.check(self._lib.y355_net_load_layer_f32(self._h, idx, w.ctypes.data, None if bb is None else bb.ctypes.data,
                                                     w.shape[0], w.shape[1], w.shape[2]))

    def load_layer_i8(self, idx, q_w, q_b, e_w, e_b):
        """int8 nets: q_w [cout,cin,k,k] (|q| <= 127, value q / 2^e_w), q_b int32 [cout] (value q / 2^e_b).
        e_w: one exponent, or an array [cout] with one per output channel (prep.quantize_folded(channel_level=True))."""
        qw, qb = i8_layer(q_w, q_b)
        if np.ndim(e_w) == 0:
            _ffi.check(self._lib.y355_net_load_layer_i8(self._h, idx, qw.ctypes.data, qb.ctypes.data, qw.shape[0], qw.shape[1],
                                                        qw.shape[2], int(e_w), int(e_b)))
            return
        ew = np.ascontiguousarray(e_w, dtype=np.int32)
        if ew.shape != (qw.shape[0],):
            raise ValueError("e_w: one exponent per output channel expected, got shape %s" % (ew.shape,))
        _ffi.check(self._lib.y355_net_load_layer_i8_pc(self._h, idx, qw.ctypes.data, qb.ctypes.data, qw.shape[0], qw.shape[1],
                                                       qw.shape[2], ew.ctypes.data, int(e_b)))

    # y355_net_layer_route: kernel family (route & 0xff) and flags of the last forward's launch of a layer
    ROUTE_FIRST, ROUTE_FRONT, ROUTE_RING, ROUTE_POINTWISE, ROUTE_GENERIC4, ROUTE_GENERIC8 = 1, 2, 3, 4, 5, 6
    ROUTE_EPI64, ROUTE_RESIDUAL, ROUTE_PER_CHANNEL = 0x100, 0x200, 0x400

    def layer_route(self, idx):
        r = C.c_int32()
        _ffi.check(self._lib.y355_net_layer_route(self._h, int(idx), C.byref(r)))
        return r.value

    def set_act_exponents(self, sa_in, sa):
        arr = (C.c_int32 * len(sa))(*[int(v) for v in sa])
        _ffi.check(self._lib.y355_net_set_act_exponents(self._h, int(sa_in), arr, len(sa)))

    def get_act_exponents(self):
        sa_in = C.c_int32()
        arr = (C.c_int32 * self.num_tensors)()
        _ffi.check(self._lib.y355_net_get_act_exponents(self._h, C.byref(sa_in), arr, self.num_tensors))
        return sa_in.value, list(arr)

    def counters(self):
        s = C.c_int64()
        _ffi.check(self._lib.y355_net_counters(self._h, C.byref(s)))
        return s.value

    def set_option(self, option, value):
        """1 = Y355_NET_OPT_WORKGROUPS (throughput mode: persistent workgroups per ring launch, 0 = one per CU)"""
        _ffi.check(self._lib.y355_net_set_option(self._h, int(option), int(value)))
        if int(option) in (_ffi.NET_OPT_MAX_CANDIDATES, _ffi.NET_OPT_HEAD_ROUTE):      # max_det follows the capacity
            self.max_det = self._lib.y355_net_max_det(self._h)
            self._out = None

    @property
    def max_candidates(self):
        return self._lib.y355_net_max_candidates(self._h)

    def set_max_candidates(self, n):
        self.set_option(_ffi.NET_OPT_MAX_CANDIDATES, n)

    def set_head_route(self, route):
        self.set_option(_ffi.NET_OPT_HEAD_ROUTE, route)

    def set_thresholds(self, conf_thresh, nms_thresh):
        _ffi.check(self._lib.y355_net_set_thresholds(self._h, float(conf_thresh), float(nms_thresh)))

    def _dev_input(self, x):
        return dev_input(x, self.input_size, self.device, self.max_batch)

    def forward_device(self, xd, flags=0, out=None):
        return self._launch(self._lib.y355_net_forward, (xd.data_ptr(),), xd.shape[0], flags, out)

    def forward(self, x, tap=False, sizes_wh=None):
        """list of (bboxes [n,4], scores [n], cls_inds int64 [n]) per image, anchor-index order.
        sizes_wh: [B,2] original (width, height) per image -- the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU."""
        xd = self._dev_input(x)
        B = xd.shape[0]
        out = self.forward_device(xd, _ffi.F_TAP if tap else 0)
        return self._collect(B, out, sizes_wh)

    def _collect(self, B, out, sizes_wh=None):
        ob, os_, oc, on = out
        if sizes_wh is not None:
            self.scale_boxes(ob, on, sizes_wh, B)
        n = on[:B].cpu()                                  # synchronises: the flag below is this forward's
        if self.overflow():
            raise_overflow(self.max_candidates)
        return split_dets(ob, os_, oc, n, B)

    @staticmethod
    def check_frames(frames):
        """uint8 [B,h,w,3] (numpy or torch), checked before any device work"""
        if not isinstance(frames, (np.ndarray, torch.Tensor)):
            raise ValueError("frames must be a numpy array or a torch tensor, got %s" % type(frames).__name__)
        dt = frames.dtype
        if not (dt == np.uint8 if isinstance(frames, np.ndarray) else dt == torch.uint8):
            raise ValueError("frames must be uint8, got %s" % (dt,))
        if len(frames.shape) != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be [B,h,w,3] (HWC BGR), got %s" % (tuple(frames.shape),))
        if frames.shape[0] < 1 or frames.shape[1] < 1 or frames.shape[2] < 1:
            raise ValueError("empty frames %s" % (tuple(frames.shape),))

    def _dev_frames(self, frames):
        self.check_frames(frames)
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.shape[0] > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (frames.shape[0], self.max_batch))
        return frames.to(self.device).contiguous()

    def forward_frames_device(self, frames, flags=0, out=None):
        """Asynchronous batched forward on camera frames: CUDA uint8 [B,h,w,3] BGR of any size (y355_net_forward_u8:
        BaseTransform's resize, normalisation, BGR->RGB and HWC->CHW inside the op that reads the network input).
        Returns the device tensors of forward_device."""
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise ValueError("expected a CUDA uint8 tensor [B,h,w,3]")
        self.check_frames(frames)
        frames = frames.contiguous()
        B, hh, ww = (int(v) for v in frames.shape[:3])
        if B > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (B, self.max_batch))
        return self._launch(self._lib.y355_net_forward_u8, (frames.data_ptr(), hh, ww), B, flags, out)

    def forward_frames(self, frames, tap=False, sizes_wh=None):
        """frames: uint8 [B,h,w,3] BGR (numpy or torch, any size).  Same return as forward() on
        synth.normalize_frames(resize_linear_u8(frames)) -- bit for bit."""
        fd = self._dev_frames(frames)
        B = fd.shape[0]
        out = self.forward_frames_device(fd, _ffi.F_TAP if tap else 0)
        return self._collect(B, out, sizes_wh)

    def resize_frames(self, frames):
        """cv2.resize(image, (W, H)) of BaseTransform for uint8 [B,h,w,3] frames on the GPU (the stage in front of the
        network); returns a CUDA uint8 tensor [B,H,W,3]."""
        fd = self._dev_frames(frames)
        B = fd.shape[0]
        out = torch.empty((B, self.input_size[0], self.input_size[1], 3), dtype=torch.uint8, device=self.device)
        self._call(self._lib.y355_net_resize_u8, fd.data_ptr(), int(fd.shape[1]), int(fd.shape[2]), B, out.data_ptr())
        return out

    # ---- frame lists: every frame of its own size (y355_net_forward_frames; include/yolo355.h and DESIGN.md section 6e)
    check_frame_list = staticmethod(framelist.check_frame_list)
    pack_frames = staticmethod(framelist.pack_frames)

    def forward_frame_list_device(self, frames, flags=0, out=None):
        """Asynchronous forward on a list of camera frames, uint8 [h,w,3] BGR each of its own size: numpy, CPU torch and
        CUDA torch frames may be mixed (y355_net_forward_frames).  Returns the device tensors of forward_device."""
        arr, B, _ = self._frame_list(frames)
        return self._launch(self._lib.y355_net_forward_frames, (arr,), B, flags, out)

    def forward_frame_list(self, frames, tap=False, sizes_wh=None):
        """Element i equals forward_frames(frames[i][None])[0], bit for bit.  sizes_wh: as forward(), or "own": every
        image's boxes rescaled by its own (width, height) -- the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU."""
        framelist.check_sizes_wh(sizes_wh)
        if isinstance(sizes_wh, str):
            sizes_wh = framelist.own_sizes_wh(framelist.check_frame_list(frames))
        return self._collect(len(frames), self.forward_frame_list_device(frames, _ffi.F_TAP if tap else 0), sizes_wh)

    def resize_frame_list(self, frames):
        """cv2.resize(image, (W, H)) of BaseTransform for every frame of a list on the GPU (the stage in front of the
        network); returns a CUDA uint8 tensor [B,H,W,3]."""
        arr, B, _ = self._frame_list(frames)
        out = torch.empty((B, self.input_size[0], self.input_size[1], 3), dtype=torch.uint8, device=self.device)
        self._call(self._lib.y355_net_resize_frames, arr, B, out.data_ptr())
        return out

    def calibrate_frame_list(self, frames, freeze=False, momentum=0.1):
        """calibrate_frames() on a list of frames of any sizes: the step on resize_frame_list(frames), bit for bit (a
        calibration step sees the maximum over the whole batch)."""
        arr, B, _ = self._frame_list(frames)
        return self._calibrate(self._lib.y355_net_calibrate_frames, (arr, B), freeze, momentum)

    def set_normalization(self, mean_bgr, std_bgr):
        """BaseTransform constants of the frame input, in the reference's BGR order."""
        _ffi.check(self._lib.y355_net_set_normalization(self._h, *float3_pair(mean_bgr, std_bgr)))

    def scale_boxes(self, boxes, count, sizes_wh, batch=None):
        """In place on a forward's device outputs: boxes[b, :count[b]] *= [w, h, w, h] with sizes_wh [B,2] (width, height)."""
        wh = framelist.wh_tensor(sizes_wh, None if batch is None else int(batch), self.device)
        self._call(self._lib.y355_net_scale_boxes, boxes.data_ptr(), count.data_ptr(), wh.data_ptr(), wh.shape[0])

    def overflow(self):
        """True if a forward since the last call dropped candidates (heads with more than 4096 anchors per image)."""
        v = C.c_int(0)
        _ffi.check(self._lib.y355_net_overflow(self._h, C.byref(v)))
        return bool(v.value)

    def candidates(self, batch):
        N = self.num_anchors_total
        b = np.empty((batch, N, 4), np.float32)
        s = np.empty((batch, N), np.float32)
        c = np.empty((batch, N), np.int32)
        _ffi.check(self._lib.y355_net_get_candidates(self._h, batch, b.ctypes.data, s.ctypes.data, c.ctypes.data))
        return b, s, c

    def get_tensor(self, idx, batch):
        """activation tensor idx of the last forward as fp32 [B,C,H,W] (parity tap)."""
        c, hh, ww = self.tensor_shape(idx)
        out = np.empty((batch, c, hh, ww), np.float32)
        _ffi.check(self._lib.y355_net_get_tensor(self._h, idx, batch, out.ctypes.data))
        return out

    def tensor_absmax(self, idx, batch):
        m = C.c_float()
        _ffi.check(self._lib.y355_net_tensor_absmax(self._h, idx, batch, C.byref(m)))
        return float(m.value)

    def calibration_exponents(self, x):
        """bf16 nets: run x and return (sa_in, [sa per tensor]) = floor(log2(127 / max|.|)) of the network
        input and of every activation tensor -- the AveragedRangeTracker first-call rule
        (models/slim_yolo_v2.py:22-33) applied to this graph.  Feeds set_act_exponents of the int8 net
        (which overrides the entries of max-pool outputs with their inputs' exponents)."""
        from .prep import RangeTracker
        xd = self._dev_input(x)
        B = xd.shape[0]
        self.forward_device(xd, _ffi.F_TAP)      # tap forward: every tensor is written (the fused front end skips conv1's map)
        sa_in = RangeTracker().update(float(xd.abs().max().item()), True)
        sa = []
        pred = {self.num_tensors - k for k in PRED_TAIL[self.arch]}
        for t in range(self.num_tensors):
            if t in pred:
                m = float(np.abs(self.get_tensor(t, B)).max())       # fp32 prediction maps
            else:
                m = self.tensor_absmax(t, B)
            sa.append(RangeTracker().update(m, True))
        return sa_in, sa

    # ---- calibration on the int8 graph itself (y355_net_calibrate; semantics in include/yolo355.h and DESIGN.md section 6)
    @property
    def num_trackers(self):
        return self.num_tensors + 1

    @property
    def trackers(self):
        """(scale float32 [1 + num_tensors], first_a int32 [...]): the AveragedRangeTracker state of the network input
        and of every tensor in graph order.  Assigning installs the state and the exponents of the trackers that have seen a
        batch (first_a != 0)."""
        n = self.num_trackers
        scale = np.zeros(n, np.float32)
        first = np.zeros(n, np.int32)
        _ffi.check(self._lib.y355_net_get_trackers(self._h, scale.ctypes.data_as(C.POINTER(C.c_float)),
                                                   first.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return scale, first

    @trackers.setter
    def trackers(self, state):
        scale = np.ascontiguousarray(np.asarray(state[0], np.float32).reshape(-1))
        first = np.ascontiguousarray(np.asarray(state[1]).reshape(-1).astype(np.int32))
        if scale.shape != first.shape:
            raise ValueError("trackers: scale and first_a differ in length")
        _ffi.check(self._lib.y355_net_set_trackers(self._h, scale.ctypes.data_as(C.POINTER(C.c_float)),
                                                   first.ctypes.data_as(C.POINTER(C.c_int32)), int(scale.shape[0])))

    def _calibrate(self, fn, head, freeze, momentum):
        n = self.num_trackers
        sa_in = C.c_int32()
        sa = (C.c_int32 * (n - 1))()
        mx = np.zeros(n, np.float32)
        self._call(fn, *head, 1 if freeze else 0, float(momentum), C.byref(sa_in), sa, mx.ctypes.data_as(C.POINTER(C.c_float)), n)
        self.last_calibration_max = mx
        return sa_in.value, list(sa)

    def calibrate(self, x, freeze=False, momentum=0.1):
        """One calibration step of an int8 net on batch x (fp32 [B,3,H,W]): every tracker sees the maximum of its tensor
        on the quantized graph, behind the exponents already updated in front of it.  Returns (sa_in, [sa per tensor]),
        which the handle now runs with; last_calibration_max holds the float32 maximum every tracker saw."""
        xd = self._dev_input(x)
        return self._calibrate(self._lib.y355_net_calibrate, (xd.data_ptr(), int(xd.shape[0])), freeze, momentum)

    def calibrate_frames(self, frames, freeze=False, momentum=0.1):
        """calibrate() on camera frames, uint8 [B,h,w,3] BGR of any size: the step on
        synth.normalize_frames(resize_linear_u8(frames)), bit for bit."""
        fd = self._dev_frames(frames)
        B, hh, ww = (int(v) for v in fd.shape[:3])
        return self._calibrate(self._lib.y355_net_calibrate_u8, (fd.data_ptr(), hh, ww, B), freeze, momentum)

    @classmethod
    def from_package(cls, path, conf_thresh=None, nms_thresh=None, max_batch=1, max_det=0, device=None):
        """An int8 net from a package of tools/prepare_net.py (integer weights, exponents, tracker state, meta): no fp32
        weights are needed.  It runs, and calibrates further (calibrate / calibrate_frames), from the package alone."""
        import json
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            net = cls(meta["arch"], meta["input_size"], meta["num_classes"], meta["anchors"],
                      meta["conf_thresh"] if conf_thresh is None else conf_thresh,
                      meta["nms_thresh"] if nms_thresh is None else nms_thresh, max_batch=max_batch, max_det=max_det,
                      device=device, dtype="int8")
            for i in range(net.num_layers):
                e_w = z["e_w_%d" % i]
                net.load_layer_i8(i, z["q_w_%d" % i], z["q_b_%d" % i], int(e_w) if e_w.ndim == 0 else e_w, int(z["e_b_%d" % i]))
            net.set_act_exponents(int(z["sa_in"]), [int(v) for v in z["sa"]])
            net.trackers = (z["tracker_scale"], z["tracker_first_a"])
        net.package_meta = meta
        return net

    def sync(self):
        _ffi.check(self._lib.y355_net_sync(self._h))

    def profile(self, enable=True):
        _ffi.check(self._lib.y355_net_profile(self._h, 1 if enable else 0))

    def profile_ms(self):
        n = self._lib.y355_net_num_timers(self._h)
        arr = (C.c_float * n)()
        _ffi.check(self._lib.y355_net_profile_get(self._h, arr))
        return list(arr)
