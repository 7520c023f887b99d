"""Python handles over the engine C ABI (include/yolo355.h): Engine, one GPU + one stream, and Pipeline, several engines on as
many streams.

The engine is the batched, integer implementation of
SlimYOLOv2_quantize_bnfuse.forward(x, quantization=True) (models/slim_yolo_v2.py:212-358).
PyTorch is used only for device memory and the stream; all compute is in libyolo355.so.  What every handle shares is in
_handle.py; the operator-level API (the Python face of csrc/ops.hip) is ops.py, re-exported here under its old names.
"""
import ctypes as C

import numpy as np
import torch

from . import _ffi, framelist
from ._handle import (Handle, StreamBound, _require_gpu, dev_input, fill_config, float3_pair, i8_layer, out_buffers, raise_if_guard,
                      raise_overflow, split_dets)
from .ops import (ConvOp, conv2d_bf16, conv2d_geom_bf16, conv3x3_i8_fused, conv3x3_i8_raw, conv_geom, conv_geom_i8_raw,  # noqa: F401
                  geom_out_size, head_f32, maxpool2x2_f32, maxpool2x2_f32_dev, maxpool2x2_i8, mfma_peak_i8, quantize_input_f32_i8,
                  reorg_f32, reorg_f32_dev, spp_f32, spp_f32_dev, upsample2x_f32, upsample2x_f32_dev)
from .prep import RETUNE, RangeTracker  # noqa: F401

NUM_LAYERS = 10
LAYER_NAMES = ["conv1", "conv2", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5", "conv6", "conv7", "pred"]


def _dev_frames(frames, device):
    return (torch.from_numpy(frames) if isinstance(frames, np.ndarray) else frames).to(device)


class Engine(StreamBound, Handle):
    _destroy = "y355_destroy"

    def __init__(self, input_size, num_classes, anchors, conf_thresh=0.01, nms_thresh=0.5,
                 max_batch=1, max_det=0, device=None, max_candidates=None, head_route=None):
        """max_candidates (default 4096, up to min(anchors per image, 65536)): the most anchors of an image that may pass
        conf_thresh; head_route 1 sends every image through the NMS route for more than 4096 candidates (Y355_OPT_MAX_CANDIDATES,
        Y355_OPT_HEAD_ROUTE of include/yolo355.h; set_max_candidates / set_head_route change them later)."""
        lib = _ffi.lib()
        self.device = _require_gpu(device)
        self.input_size = [int(input_size[0]), int(input_size[1])]
        self.num_classes = int(num_classes)
        self.anchors = [[float(a), float(b)] for a, b in anchors]
        self.max_batch = int(max_batch)
        cfg = _ffi.Config()
        fill_config(cfg, self.device, self.input_size, self.num_classes, self.anchors, conf_thresh, nms_thresh, self.max_batch, max_det)
        self._create(lib, cfg, lib.y355_create)
        self.max_det = lib.y355_max_det(self._h)
        self.num_anchors_total = lib.y355_num_anchors_total(self._h)
        self.conf_thresh, self.nms_thresh = float(conf_thresh), float(nms_thresh)
        self._out = None
        if max_candidates is not None:
            self.set_max_candidates(max_candidates)
        if head_route is not None:
            self.set_head_route(head_route)

    @classmethod
    def _borrowed(cls, handle, like, stream):
        """Engine view of a handle somebody else owns (a pipeline's handle i): the taps / statistics / profiling calls of the
        engine ABI on it.  `like` supplies the configuration; the view launches on the handle's own stream."""
        e = cls.__new__(cls)
        e._own(like._lib, handle, owned=False)
        e.device, e.input_size, e.num_classes, e.anchors = like.device, like.input_size, like.num_classes, like.anchors
        e.max_batch, e.max_det = like.max_batch, like.max_det
        e.num_anchors_total = e._lib.y355_num_anchors_total(handle)
        e.conf_thresh, e.nms_thresh = like.conf_thresh, like.nms_thresh
        e._stream = stream
        e._out = None
        return e

    # ------------------------------------------------------------------ weights / exponents
    def load_layer(self, idx, q_w, q_b, e_w, e_b):
        qw, qb = i8_layer(q_w, q_b)
        _ffi.check(self._lib.y355_load_layer(self._h, idx, qw.ctypes.data, qb.ctypes.data,
                                             qw.shape[0], qw.shape[1], int(e_w), int(e_b)))

    def load_quantized(self, qlayers):
        """qlayers: 10 dicts with q_w [cout,cin,3,3], q_b [cout], e_w, e_b (conv1..conv7, pred)."""
        for i, L in enumerate(qlayers):
            self.load_layer(i, L["q_w"], L["q_b"], L["e_w"], L["e_b"])

    def set_act_exponents(self, sa):
        arr = (C.c_int32 * 11)(*[int(v) for v in sa])
        _ffi.check(self._lib.y355_set_act_exponents(self._h, arr))

    def get_act_exponents(self):
        arr = (C.c_int32 * 11)()
        _ffi.check(self._lib.y355_get_act_exponents(self._h, arr))
        return list(arr)

    def set_retune(self, retune=RETUNE):
        arr = (C.c_int32 * 10)(*[int(v) for v in retune])
        _ffi.check(self._lib.y355_set_retune(self._h, arr))

    def set_option(self, option, value):
        """Engine options of include/yolo355.h, e.g. set_option(_ffi.OPT_FUSE_FRONT, 0): one launch per layer."""
        _ffi.check(self._lib.y355_set_option(self._h, int(option), int(value)))
        if int(option) in (_ffi.OPT_MAX_CANDIDATES, _ffi.OPT_HEAD_ROUTE):      # max_det follows the capacity
            self.max_det = self._lib.y355_max_det(self._h)
            self._out = None

    def set_max_candidates(self, n):
        self.set_option(_ffi.OPT_MAX_CANDIDATES, n)

    def set_head_route(self, route):
        self.set_option(_ffi.OPT_HEAD_ROUTE, route)

    @property
    def max_candidates(self):
        return self._lib.y355_max_candidates(self._h)

    def overflow(self):
        """True if a forward since the last call dropped candidates beyond max_candidates (heads with more than 4096 anchors
        per image, or with the large route forced; always False otherwise)."""
        v = C.c_int(0)
        _ffi.check(self._lib.y355_overflow(self._h, C.byref(v)))
        return bool(v.value)

    def set_thresholds(self, conf_thresh, nms_thresh):
        self.conf_thresh, self.nms_thresh = float(conf_thresh), float(nms_thresh)
        _ffi.check(self._lib.y355_set_thresholds(self._h, self.conf_thresh, self.nms_thresh))

    def set_normalization(self, mean_bgr, std_bgr):
        _ffi.check(self._lib.y355_set_normalization(self._h, *float3_pair(mean_bgr, std_bgr)))

    # ------------------------------------------------------------------ inputs
    def _dev_input(self, x):
        return dev_input(x, self.input_size, self.device, self.max_batch)

    def _check_batch(self, B):
        if B > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (B, self.max_batch))

    # ------------------------------------------------------------------ calibration
    def calibrate(self, x, trackers, freeze=True):
        """One calibration step: the tracker semantics of models/slim_yolo_v2.py:16-38 layer by layer on the GPU, in ONE call
        of the C ABI (y355_calibrate: the state machine and its float32 arithmetic live in the library).
        trackers: 11 prep.RangeTracker (input, conv1..conv7, pred) -- the checkpoint buffers scale / first_a; they are handed
        to the handle, updated there (first call: scale = 127/max; frozen: unchanged; else EMA) and read back in place.
        Leaves the engine's feature maps and exponents as the reference's forward would.  Returns the exponents."""
        xd = self._dev_input(x)
        sa, mx = _calibrate_call(self._lib.y355_set_trackers, self._lib.y355_get_trackers, self._lib.y355_calibrate, self._h,
                                 xd, trackers, freeze, self._enter)
        self.calib_max = mx                               # max|.| seen by each tracker in this calibration
        return sa

    def layer_stats(self, idx):
        st = _ffi.LayerStats()
        _ffi.check(self._lib.y355_layer_stats_get(self._h, idx, C.byref(st)))
        return dict(absmax_t=st.absmax_t, frac_bits=st.frac_bits, saturated=st.saturated, guard=st.guard)

    def get_feature(self, idx, batch):
        """int8 [B,C,Ho,Wo] output of layer idx of the last run (parity tap)."""
        cout = [16, 32, 64, 64, 128, 128, 256, 256, 256, len(self.anchors) * (5 + self.num_classes)][idx]
        div = [2, 4, 4, 8, 8, 16, 16, 16, 16, 16][idx]
        out = np.empty((batch, cout, self.input_size[0] // div, self.input_size[1] // div), dtype=np.int8)
        _ffi.check(self._lib.y355_get_feature(self._h, idx, batch, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ the hot path
    def forward_device(self, xd, flags=0, out=None):
        """Asynchronous batched forward on device tensors.  xd: CUDA float32 [B,3,H,W] contiguous.
        Returns (boxes [max_batch,max_det,4], scores, cls int32, count int32) device tensors,
        rows >= B / entries >= count[b] undefined."""
        return self._launch(self._lib.y355_forward, (xd.data_ptr(),), xd.shape[0], flags, out)

    def forward_frames_device(self, frames, flags=0, out=None):
        """Asynchronous batched forward on camera frames: CUDA uint8 [B,H,W,3] BGR at the network size
        (BaseTransform fused into the first layer, y355_forward_u8)."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_cuda:
            raise ValueError("expected a CUDA uint8 tensor [B,h,w,3]")
        frames = frames.contiguous()
        B = frames.shape[0]
        self._check_batch(B)
        if list(frames.shape[1:3]) == self.input_size:
            return self._launch(self._lib.y355_forward_u8, (frames.data_ptr(),), B, flags, out)
        # frames of another size: BaseTransform's cv2.resize (data/__init__.py:36) on the GPU first
        return self._launch(self._lib.y355_forward_u8_resized, (frames.data_ptr(), int(frames.shape[1]), int(frames.shape[2])), B, flags,
                            out, (None,))

    def resize_frames(self, frames):
        """cv2.resize(image, (W, H)) of BaseTransform for a batch of uint8 [B,h,w,3] frames on the GPU (the stage
        y355_forward_u8_resized runs in front of the network); returns a CUDA uint8 tensor [B,H,W,3]."""
        fd = _dev_frames(frames, self.device).contiguous()
        B = fd.shape[0]
        self._check_batch(B)
        out = torch.empty((B, self.input_size[0], self.input_size[1], 3), dtype=torch.uint8, device=self.device)
        self._call(self._lib.y355_forward_u8_resized, fd.data_ptr(), int(fd.shape[1]), int(fd.shape[2]), B, 0,
                   None, None, None, None, out.data_ptr())
        return out

    # ---- frame lists: every frame of its own size (y355_forward_frames; include/yolo355.h and DESIGN.md section 6e)
    def resize_frame_list(self, frames):
        """cv2.resize(image, (W, H)) of BaseTransform for every frame of a list on the GPU (the ragged stage in front of the
        network, y355_resize_frames); returns a CUDA uint8 tensor [B,H,W,3]."""
        arr, B, _ = self._frame_list(frames)
        out = torch.empty((B, self.input_size[0], self.input_size[1], 3), dtype=torch.uint8, device=self.device)
        self._call(self._lib.y355_resize_frames, arr, B, out.data_ptr())
        return out

    def forward_frame_list_device(self, frames, flags=0, out=None):
        """Asynchronous forward on a list of camera frames, uint8 [h,w,3] BGR each of its own size: numpy, CPU torch and
        CUDA torch frames may be mixed (y355_forward_frames).  Returns the device tensors of forward_device."""
        arr, B, _ = self._frame_list(frames)
        return self._launch(self._lib.y355_forward_frames, (arr,), B, flags, out)

    # ---- the host lists: every entry point ends in _collect
    def _collect(self, B, out, find, wh=None):
        """The host lists of a forward's outputs, list of (bboxes float32 [n,4], scores float32 [n], cls_inds int64 [n]) per
        image in anchor-index order: the reference's eval-mode return for every image of the batch.  wh [B,2] (device):
        the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU first (y355_scale_boxes).  find: the head-room guard of that
        forward, as the reference raises it."""
        ob, os_, oc, on = out
        if wh is not None:
            self._call(self._lib.y355_scale_boxes, ob.data_ptr(), on.data_ptr(), wh.data_ptr(), B)
        n = on[:B].cpu()                                  # synchronises: the flag and the counters below are this forward's
        if self.overflow():
            raise_overflow(self.max_candidates)
        if find:
            raise_if_guard(self.counters()[1])
        return split_dets(ob, os_, oc, n, B)

    def forward(self, x, find=False, tap=False):
        """list of (bboxes float32 [n,4], scores float32 [n], cls_inds int64 [n]) per image,
        in anchor-index order: the reference's eval-mode return for every image of the batch."""
        xd = self._dev_input(x)
        out = self.forward_device(xd, (_ffi.F_GUARD if find else 0) | (_ffi.F_TAP if tap else 0))
        return self._collect(xd.shape[0], out, find)

    def forward_frames(self, frames, find=False):
        """frames: uint8 [B,H,W,3] BGR (numpy or torch).  Same return as forward(normalised tensor)."""
        fd = _dev_frames(frames, self.device)
        return self._collect(fd.shape[0], self.forward_frames_device(fd, _ffi.F_GUARD if find else 0), find)

    def forward_frame_list(self, frames, find=False, tap=False, sizes_wh=None):
        """Element i equals forward_frames(frames[i][None])[0] (the frame resized by BaseTransform's cv2.resize), bit for bit.
        sizes_wh: None, [B,2] original (width, height) per image, or "own": every image's boxes rescaled by its own source
        (width, height) -- the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU (y355_scale_boxes)."""
        framelist.check_sizes_wh(sizes_wh)
        wh = framelist.sizes_wh_tensor(sizes_wh, framelist.check_frame_list(frames), self.device)
        out = self.forward_frame_list_device(frames, (_ffi.F_GUARD if find else 0) | (_ffi.F_TAP if tap else 0))
        return self._collect(len(frames), out, find, wh)

    def forward_scaled(self, x, sizes_wh, find=False, frames=False):
        """Batched forward + the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU (y355_scale_boxes).
        x: float32 [B,3,H,W] (or uint8 frames [B,H,W,3] with frames=True); sizes_wh: [B,2] original (width, height).
        Returns a list over the batch of (bboxes in pixels of the original image, scores, cls_inds)."""
        xd = _dev_frames(x, self.device) if frames else self._dev_input(x)
        B = xd.shape[0]
        wh = framelist.wh_tensor(sizes_wh, B, self.device)
        out = (self.forward_frames_device if frames else self.forward_device)(xd, _ffi.F_GUARD if find else 0)
        return self._collect(B, out, find, wh)

    def counters(self):
        s, g = C.c_int64(), C.c_int64()
        _ffi.check(self._lib.y355_forward_counters(self._h, C.byref(s), C.byref(g)))
        return s.value, g.value

    def candidates(self, batch):
        N = self.num_anchors_total
        b = np.empty((batch, N, 4), np.float32)
        s = np.empty((batch, N), np.float32)
        c = np.empty((batch, N), np.int32)
        _ffi.check(self._lib.y355_get_candidates(self._h, batch, b.ctypes.data, s.ctypes.data, c.ctypes.data))
        return b, s, c

    def head_nms(self, pred_q, sa_pred):
        """Head only (slim_yolo_v2.py:330-358) on an int8 pred tensor [B,A*(5+C),Hs,Ws]."""
        pq = np.ascontiguousarray(pred_q, dtype=np.int8)
        B = pq.shape[0]
        out = out_buffers(B, self.max_det, "cpu")
        _ffi.check(self._lib.y355_head_nms(self._h, pq.ctypes.data, B, int(sa_pred), *[t.data_ptr() for t in out]))
        return self._collect(B, out, False)

    def sync(self):
        _ffi.check(self._lib.y355_sync(self._h))

    def profile(self, enable=True):
        """True / 1: intervals between HIP events around every launch (profile_ms); 2: also the launches' own start / end
        timestamps (profile_kernel_ms; the intervals of such a run are wider)."""
        _ffi.check(self._lib.y355_profile(self._h, int(enable)))

    def profile_ms(self):
        arr = (C.c_float * _ffi.NUM_TIMERS)()
        _ffi.check(self._lib.y355_profile_get(self._h, arr))
        return list(arr)

    def profile_kernel_ms(self):
        """the layers' own kernel durations of the last profiled forward (ms; 0 where the launch records none):
        start / end timestamps of the launch itself, i.e. what rocprofv3 reports, without the gaps between launches."""
        arr = (C.c_float * 10)()
        _ffi.check(self._lib.y355_profile_kernel_get(self._h, arr))
        return list(arr)

    def profile_kernels_ms(self):
        """own durations (ms) of EVERY launch of the last forward profiled with profile(2): slots 0..9 layers (the fused front
        end = slot 0), 10 head decode, 11 candidate sort, 12 NMS pair walk, 13 NMS rounds + output."""
        arr = (C.c_float * _ffi.NUM_KERNEL_TIMERS)()
        _ffi.check(self._lib.y355_profile_kernels_get(self._h, arr))
        return list(arr)


def _calibrate_call(set_fn, get_fn, cal_fn, handle, xd, trackers, freeze, enter):
    """push the 11 tracker states into the handle, run the C calibration step, read the states back into `trackers`"""
    if len(trackers) != 11:
        raise ValueError("expected 11 trackers (input, conv1..conv7, pred)")
    moms = {float(t.momentum) for t in trackers}
    if len(moms) != 1:
        raise ValueError("the 11 trackers must share one momentum")
    scale = (C.c_float * 11)(*[float(t.scale.reshape(-1)[0].item()) for t in trackers])
    first = (C.c_int32 * 11)(*[int(t.first_a) for t in trackers])
    _ffi.check(set_fn(handle, scale, first))
    sa = (C.c_int32 * 11)()
    mx = (C.c_float * 11)()
    enter()                                               # the call synchronises the engine's stream itself
    _ffi.check(cal_fn(handle, xd.data_ptr(), int(xd.shape[0]), 1 if freeze else 0, moms.pop(), sa, mx))
    _ffi.check(get_fn(handle, scale, first))
    for i, t in enumerate(trackers):
        t.scale = torch.tensor([scale[i]], dtype=torch.float32)
        t.first_a = int(first[i])
    return list(sa), [float(v) for v in mx]


class Pipeline(Handle):
    """The throughput regime behind the API (y355_pipeline, include/yolo355.h): `handles` engines on as many HIP streams, the
    submitted batches dealt to them round-robin, so that the head / NMS of one batch runs beside the convolutions of the next.

        pipe = Pipeline([416, 416], 2, ANCHOR_SIZE_MASK, max_batch=64)
        pipe.load_quantized(qlayers); pipe.calibrate(x0, trackers)
        t = pipe.submit(x_cuda)               # asynchronous; up to pipe.depth tickets in flight
        boxes, scores, cls, count = pipe.outputs(t)     # device tensors, valid after pipe.wait(t)
        dets = pipe.fetch(t)                  # or: the reference's per-image (bboxes, scores, cls_inds) lists on the host

    Results equal a stand-alone Engine's bit for bit (tests/test_pipeline.py).  forward(x) takes any batch size: chunks of
    max_batch in flight, results in order -- what models.SlimYOLOv2_quantize_bnfuse.forward_batch and the batched evaluators run."""
    _destroy = "y355_pipeline_destroy"

    def __init__(self, input_size, num_classes, anchors, conf_thresh=0.01, nms_thresh=0.5, max_batch=64, max_det=0,
                 device=None, handles=0, ring_workgroups=-1, max_candidates=None, head_route=None):
        lib = _ffi.lib()
        self.device = _require_gpu(device)
        self.input_size = [int(input_size[0]), int(input_size[1])]
        self.num_classes = int(num_classes)
        self.anchors = [[float(a), float(b)] for a, b in anchors]
        self.max_batch = int(max_batch)
        cfg = _ffi.Config()
        fill_config(cfg, self.device, self.input_size, self.num_classes, self.anchors, conf_thresh, nms_thresh, self.max_batch, max_det)
        h = C.c_void_p()
        nh = _ffi.PIPE_DEFAULT_HANDLES if int(handles) == 0 else int(handles)     # the C ABI's default (Y355_PIPE_DEFAULT_HANDLES)
        # the handles run on torch streams: PyTorch's allocator tracks memory per stream, so torch must own (and outlive)
        # every stream its tensors are used on -- y355_pipeline_create_on
        self._tstreams = [torch.cuda.Stream(device=self.device) for _ in range(max(nh, 1))]
        sp = (C.c_void_p * len(self._tstreams))(*[st.cuda_stream for st in self._tstreams])
        with torch.cuda.device(self.device):
            _ffi.check(lib.y355_pipeline_create_on(C.byref(cfg), nh, int(ring_workgroups), sp, C.byref(h)))
        self._own(lib, h)
        self.handles = lib.y355_pipeline_handles(h)
        self.depth = lib.y355_pipeline_depth(h)
        self.max_det = lib.y355_pipeline_max_det(h)
        self.conf_thresh, self.nms_thresh = float(conf_thresh), float(nms_thresh)
        self._bufs = [None] * self.depth                  # torch-owned output buffers, one set per ticket slot
        self._tickets = {}                                # slot -> (ticket, batch, outputs, input) of the ticket that holds it
        self._next = 0
        if max_candidates is not None:
            self.set_max_candidates(max_candidates)
        if head_route is not None:
            self.set_head_route(head_route)

    # ------------------------------------------------------------------ configuration (every handle)
    def load_layer(self, idx, q_w, q_b, e_w, e_b):
        qw, qb = i8_layer(q_w, q_b)
        _ffi.check(self._lib.y355_pipeline_load_layer(self._h, idx, qw.ctypes.data, qb.ctypes.data, qw.shape[0], qw.shape[1],
                                                      int(e_w), int(e_b)))

    def load_quantized(self, qlayers):
        for i, L in enumerate(qlayers):
            self.load_layer(i, L["q_w"], L["q_b"], L["e_w"], L["e_b"])

    def set_act_exponents(self, sa):
        _ffi.check(self._lib.y355_pipeline_set_act_exponents(self._h, (C.c_int32 * 11)(*[int(v) for v in sa])))

    def set_retune(self, retune=RETUNE):
        _ffi.check(self._lib.y355_pipeline_set_retune(self._h, (C.c_int32 * 10)(*[int(v) for v in retune])))

    def set_thresholds(self, conf_thresh, nms_thresh):
        self.conf_thresh, self.nms_thresh = float(conf_thresh), float(nms_thresh)
        _ffi.check(self._lib.y355_pipeline_set_thresholds(self._h, self.conf_thresh, self.nms_thresh))

    def set_option(self, option, value):
        _ffi.check(self._lib.y355_pipeline_set_option(self._h, int(option), int(value)))
        if int(option) in (_ffi.OPT_MAX_CANDIDATES, _ffi.OPT_HEAD_ROUTE):      # max_det follows the capacity: tickets still out are void
            self.max_det = self._lib.y355_pipeline_max_det(self._h)
            self._bufs = [None] * self.depth
            self._tickets = {}

    def set_max_candidates(self, n):
        """Y355_OPT_MAX_CANDIDATES on every handle; call it while no ticket is out"""
        self.set_option(_ffi.OPT_MAX_CANDIDATES, n)

    def set_head_route(self, route):
        self.set_option(_ffi.OPT_HEAD_ROUTE, route)

    @property
    def max_candidates(self):
        return self._lib.y355_max_candidates(self._lib.y355_pipeline_engine(self._h, 0))

    def overflow(self, ticket):
        """True if the forward of this ticket dropped candidates beyond max_candidates (waits for that ticket only)"""
        v = C.c_int(0)
        _ffi.check(self._lib.y355_pipeline_ticket_overflow(self._h, int(ticket), C.byref(v)))
        return bool(v.value)

    def set_normalization(self, mean_bgr, std_bgr):
        _ffi.check(self._lib.y355_pipeline_set_normalization(self._h, *float3_pair(mean_bgr, std_bgr)))

    def calibrate(self, x, trackers, freeze=True):
        """Engine.calibrate on handle 0 (y355_pipeline_calibrate); every handle gets the resulting trackers and exponents."""
        xd = self._dev_input(x)
        sa, mx = _calibrate_call(self._lib.y355_pipeline_set_trackers, self._lib.y355_pipeline_get_trackers,
                                 self._lib.y355_pipeline_calibrate, self._h, xd, trackers, freeze,
                                 lambda: torch.cuda.current_stream(self.device).synchronize())
        self.calib_max = mx
        return sa

    # ------------------------------------------------------------------ the hot path
    def _dev_input(self, x):
        return dev_input(x, self.input_size, self.device)         # any batch size: submit checks its chunk against max_batch

    def _slot_bufs(self, slot):
        if self._bufs[slot] is None:
            self._bufs[slot] = out_buffers(self.max_batch, self.max_det, self.device)
        return self._bufs[slot]

    def submit(self, xd, flags=0, out=None, frames=False, ordered=True):
        """Enqueue one forward; returns the ticket.  xd: CUDA float32 [B,3,H,W] contiguous (frames=True: uint8 [B,H,W,3] BGR at
        the network size).  out: (boxes, scores, cls int32, count int32) device tensors (default: the pipeline's buffer set of
        the ticket's slot, reused `depth` submits later).  ordered=True: the forward starts behind whatever torch's current
        stream has queued (the input's producer); False: the caller guarantees the input is complete."""
        B = int(xd.shape[0])
        if B > self.max_batch:
            raise ValueError("batch %d > max_batch %d" % (B, self.max_batch))
        slot = self._next % self.depth
        ob, os_, oc, on = out if out is not None else self._slot_bufs(slot)
        t = C.c_longlong()
        cur = torch.cuda.current_stream(self.device).cuda_stream if ordered else 0
        fn = self._lib.y355_pipeline_submit_u8 if frames else self._lib.y355_pipeline_submit
        _ffi.check(fn(self._h, xd.data_ptr(), B, int(flags) | (_ffi.PIPE_AFTER_STREAM if ordered else 0), cur,
                      ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), on.data_ptr(), C.byref(t)))
        self._next = t.value + 1
        self._tickets[t.value % self.depth] = (t.value, B, (ob, os_, oc, on), xd)   # keeps the input alive until its slot is reused
        return t.value

    def submit_frame_list(self, frames, flags=0, out=None, ordered=True):
        """submit() for a list of camera frames, uint8 [h,w,3] BGR each of its own size (numpy, CPU torch and CUDA torch frames
        may be mixed; at most max_batch): y355_pipeline_submit_frames.  Host frames go through one pinned buffer and one
        asynchronous copy on the ticket's stream, CUDA frames are read in place.  Every tensor the launch reads is held in the
        ticket's record until its slot is reused (`depth` submits later) and marked with record_stream on the handle's
        stream, so the caller may drop its frames right after the call."""
        slot = self._next % self.depth
        stream = self._tstreams[self._next % self.handles]
        arr, B, _, held = framelist.frame_list(frames, self.max_batch, self.device, stream)
        ob, os_, oc, on = out if out is not None else self._slot_bufs(slot)
        t = C.c_longlong()
        cur = torch.cuda.current_stream(self.device).cuda_stream if ordered else 0
        _ffi.check(self._lib.y355_pipeline_submit_frames(self._h, arr, B, int(flags) | (_ffi.PIPE_AFTER_STREAM if ordered else 0), cur,
                                                         ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), on.data_ptr(), C.byref(t)))
        self._next = t.value + 1
        self._tickets[t.value % self.depth] = (t.value, B, (ob, os_, oc, on), held)
        return t.value

    def forward_frame_list(self, frames, find=False, sizes_wh=None):
        """Any number of frames of any sizes: chunks of max_batch submitted back to back (up to `depth` in flight), results in
        order; element i equals Engine.forward_frame_list([frames[i]])[0], bit for bit.  sizes_wh: None, [n,2] original
        (width, height), or "own" (every image by its own source size).  find=True: the 2^15 head-room guard."""
        framelist.check_sizes_wh(sizes_wh)
        sizes = framelist.check_frame_list(frames)          # the whole list before the first submit
        wh = framelist.sizes_wh_tensor(sizes_wh, sizes, self.device)
        flags = _ffi.F_GUARD if find else 0
        return self._run_chunks(len(frames), lambda i0, i1: self.submit_frame_list(list(frames[i0:i1]), flags), wh, find)

    def _run_chunks(self, n, submit_chunk, wh, find):
        """chunks of max_batch through submit_chunk(i0, i1) -> ticket, up to `depth` in flight, results in order.  wh [n,2]
        (or None): scale_boxes per ticket, its rows kept in the ticket's record and marked for the ticket's stream like the
        ticket's inputs.  find: every ticket's guard count is read from its handle before that handle's next forward."""
        res, tickets = [], []
        guard = 0
        for i0 in range(0, n, self.max_batch):
            if len(tickets) == self.depth:                # the oldest ticket's slot is about to be reused: take its result first
                res.extend(self.fetch(tickets.pop(0)))
            t = submit_chunk(i0, min(n, i0 + self.max_batch))
            if wh is not None:
                self._scale_ticket(t, wh[i0:i0 + self.max_batch])
            tickets.append(t)
            if find:                                      # the guard count of THIS forward: its handle's counters, read before the next
                sat, g = C.c_int64(), C.c_int64()
                eh = C.c_void_p(self._lib.y355_pipeline_engine(self._h, t % self.handles))
                _ffi.check(self._lib.y355_forward_counters(eh, C.byref(sat), C.byref(g)))
                guard += g.value
        for t in tickets:
            res.extend(self.fetch(t))
        raise_if_guard(guard)
        return res

    def _scale_ticket(self, t, whc):
        """scale_boxes on ticket t by the rows whc, which are kept in the ticket's record and marked for the ticket's stream"""
        whc.record_stream(self._tstreams[t % self.handles])
        self._tickets[t % self.depth] += (whc,)
        self.scale_boxes(t, whc)

    def submit_batch(self, x, sizes_wh=None):
        """submit() for a host or device batch [n,3,H,W] of up to depth * max_batch images: its chunks of max_batch back to
        back, each with scale_boxes by its rows of sizes_wh [n,2] (held like the ticket's input).  Returns (tickets, wh): wh
        is the device tensor of sizes_wh, or None."""
        xd = self._dev_input(x)
        n = int(xd.shape[0])
        if n > self.depth * self.max_batch:
            raise ValueError("submit_batch takes at most %d images at a time" % (self.depth * self.max_batch))
        wh = None if sizes_wh is None else framelist.wh_tensor(sizes_wh, n, self.device)
        tickets = []
        for i0 in range(0, n, self.max_batch):
            tickets.append(self.submit(xd[i0:i0 + self.max_batch]))
            if wh is not None:
                self._scale_ticket(tickets[-1], wh[i0:i0 + self.max_batch])
        return tickets, wh

    def submit_frame_batch(self, frames, sizes_wh=None):
        """submit_batch for a list of up to depth * max_batch camera frames, each of its own size: its chunks of max_batch
        through submit_frame_list back to back, each with scale_boxes by its rows of sizes_wh (None, [n,2], or "own").  Returns
        (tickets, wh)."""
        framelist.check_sizes_wh(sizes_wh)
        sizes = framelist.check_frame_list(frames)
        n = len(frames)
        if n > self.depth * self.max_batch:
            raise ValueError("submit_frame_batch takes at most %d frames at a time" % (self.depth * self.max_batch))
        wh = framelist.sizes_wh_tensor(sizes_wh, sizes, self.device)
        tickets = []
        for i0 in range(0, n, self.max_batch):
            tickets.append(self.submit_frame_list(list(frames[i0:i0 + self.max_batch])))
            if wh is not None:
                self._scale_ticket(tickets[-1], wh[i0:i0 + self.max_batch])
        return tickets, wh

    def _record(self, ticket):
        rec = self._tickets.get(ticket % self.depth)
        if rec is None or rec[0] != ticket:
            raise _ffi.Y355Error(_ffi.ENOTREADY, "ticket %d is gone (a ticket lives for %d more submits)" % (ticket, self.depth))
        return rec

    def outputs(self, ticket):
        """(boxes [max_batch,max_det,4], scores, cls, count) device tensors of the ticket; rows >= B / entries >= count[b] undefined.
        Read them after wait(ticket)."""
        return self._record(ticket)[2]

    def wait(self, ticket, host=False):
        """host=False: torch's current stream waits for the ticket (no host block); True: the host blocks until it is done."""
        cur = torch.cuda.current_stream(self.device).cuda_stream
        _ffi.check(self._lib.y355_pipeline_wait(self._h, int(ticket), 0 if host else 1, cur))

    def release(self, ticket):
        """the work queued on torch's current stream so far is the last reader of the ticket's outputs"""
        _ffi.check(self._lib.y355_pipeline_release(self._h, int(ticket), torch.cuda.current_stream(self.device).cuda_stream))

    def stream(self, ticket):
        """torch view of the HIP stream of the handle that runs `ticket` (for work that must follow it without an event)"""
        return self._tstreams[int(ticket) % self.handles]

    def engine(self, i):
        """Engine view of handle i (not owning): taps, statistics, profiling, options.  Do not run forwards on it while tickets
        are in flight."""
        if not 0 <= i < self.handles:
            raise IndexError(i)
        return Engine._borrowed(C.c_void_p(self._lib.y355_pipeline_engine(self._h, i)), self, self._tstreams[i])

    @property
    def next_ticket(self):
        return self._next

    def scale_boxes(self, ticket, wh_dev):
        _ffi.check(self._lib.y355_pipeline_scale_boxes(self._h, int(ticket), wh_dev.data_ptr()))

    def fetch(self, ticket):
        """The reference's eval-mode return for every image of the ticket's batch: list of (bboxes float32 [n,4], scores
        float32 [n], cls_inds int64 [n]), anchor-index order (models/slim_yolo_v2.py:205-210)."""
        B = self._record(ticket)[1]
        out = out_buffers(B, self.max_det, "cpu")
        _ffi.check(self._lib.y355_pipeline_fetch(self._h, int(ticket), *[t.data_ptr() for t in out]))
        if self.overflow(ticket):
            raise_overflow(self.max_candidates)
        return split_dets(*out, B)

    def counters(self):
        s, g = C.c_int64(), C.c_int64()
        _ffi.check(self._lib.y355_pipeline_counters(self._h, C.byref(s), C.byref(g)))
        return s.value, g.value

    def forward(self, x, find=False, sizes_wh=None, frames=False):
        """Any number of images: chunks of max_batch submitted back to back (up to `depth` in flight), results in order.
        sizes_wh [B,2]: the evaluators' `bboxes *= [[w, h, w, h]]` on the GPU.  find=True: the 2^15 head-room guard."""
        xd = _dev_frames(x, self.device).contiguous() if frames else self._dev_input(x)
        n = int(xd.shape[0])
        wh = None if sizes_wh is None else framelist.wh_tensor(sizes_wh, n, self.device)
        flags = _ffi.F_GUARD if find else 0
        return self._run_chunks(n, lambda i0, i1: self.submit(xd[i0:i1], flags, frames=frames), wh, find)

    def sync(self):
        _ffi.check(self._lib.y355_pipeline_sync(self._h))

