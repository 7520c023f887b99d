"""Drop-in for the reference's models/slim_yolo_v2.py quantized model, backed by the MI355X
engine (include/yolo355.h).

Same constructor, attributes, state_dict layout and eval-mode return as
`SlimYOLOv2_quantize_bnfuse` (models/slim_yolo_v2.py:40-382):

    net = SlimYOLOv2_quantize_bnfuse(device, input_size=[416, 416], num_classes=2,
                                     anchor_size=ANCHOR_SIZE_MASK)
    net.load_state_dict(torch.load(".../slim_yolo_v2_q_bf_retune_quantize_1.pth"), strict=False)
    net.eval()
    bboxes, scores, cls_inds = net(x, quantization=True)      # numpy, image 0, anchor order
    all_images = net.forward_batch(x)                          # new: every image of the batch

What runs where: parameters live in torch modules (checkpoint compatibility only); every
forward goes through the C ABI into the HIP kernels.  There is no PyTorch compute path:
`quantization=True` runs the int8 engine (y355_engine), the default `quantization=False`
(the call of test.py:84 / demo.py:81 / utils/vocapi_evaluator.py:67: trackers are the identity,
fp32 math on whatever weights are loaded) runs the same graph on the bf16 MFMA (y355_net);
`trainable=True` (losses) raises NotImplementedError.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import framelist, prep
from ..engine import Engine, Pipeline
from ..netengine import Net
from ..utils import Conv2d, Conv2d_fuse
from ..utils.modules import folded_f32

_CONVS = ["conv1", "conv2", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv5", "conv6", "conv7"]
_TRACKERS = ["a_tracker_in", "a_tracker1", "a_tracker2", "a_tracker3_1", "a_tracker3_2", "a_tracker4_1",
             "a_tracker4_2", "a_tracker5", "a_tracker6", "a_tracker7", "a_tracker_pred"]


def _cap(model):
    """a model's max_candidates as Engine / Pipeline / Net take it: None = leave the default capacity (4096) alone"""
    cap = getattr(model, "max_candidates", 4096)
    return None if cap == 4096 else cap


def _device(model):
    return model.device if isinstance(model.device, (str, torch.device)) else "cuda:0"


def _cached(slots, slot, key, batch, version, build, load):
    """The handle in slots[slot], kept there as (handle, key, version): build() makes a new one (the old one is closed
    first) when the configuration key changed or its max_batch does not hold `batch`, load(handle) runs when the weight
    version changed.  An empty slot is a missing key."""
    h, k, v = slots.get(slot, (None, None, None))
    if h is None or k != key or h.max_batch < batch:
        if h is not None:
            h.close()
        h, v = build(), None
        slots[slot] = (h, key, None)
    if v != version:
        load(h)
        slots[slot] = (h, key, version)
    return h


class AveragedRangeTracker(nn.Module):
    """Checkpoint-compatible holder of the tracker buffers (models/slim_yolo_v2.py:9-14).
    The max|activation| statistics come from the GPU; the state update is prep.RangeTracker."""

    def __init__(self, momentum=0.1):
        super().__init__()
        self.momentum = momentum
        self.register_buffer("scale", torch.zeros(1))
        self.register_buffer("first_a", torch.zeros(1))


class SlimYOLOv2_quantize_bnfuse(nn.Module):
    def __init__(self, device, input_size=None, num_classes=20, trainable=False, conf_thresh=0.01,
                 nms_thresh=0.5, anchor_size=None, hr=False, max_candidates=4096):
        super().__init__()
        self.max_candidates = int(max_candidates)      # most anchors of an image that may pass conf_thresh (Engine / Net max_candidates)
        self.device = device
        self.input_size = list(input_size)
        self.num_classes = num_classes
        self.trainable = trainable
        self.conf_thresh = conf_thresh
        self.nms_thresh = nms_thresh
        self.anchor_size = torch.tensor(anchor_size)
        self.anchor_number = len(anchor_size)
        self.stride = 16
        self.scale = np.array([[[input_size[1], input_size[0], input_size[1], input_size[0]]]])

        self.a_tracker_in = AveragedRangeTracker()
        self.conv1 = Conv2d_fuse(3, 16, 3, 1, leakyReLU=True)
        self.a_tracker1 = AveragedRangeTracker()
        self.pool1 = nn.MaxPool2d(2, 2)
        self.conv2 = Conv2d_fuse(16, 32, 3, 1, leakyReLU=True)
        self.a_tracker2 = AveragedRangeTracker()
        self.pool2 = nn.MaxPool2d(2, 2)
        self.conv3_1 = Conv2d_fuse(32, 64, 3, 1, leakyReLU=True)
        self.a_tracker3_1 = AveragedRangeTracker()
        self.conv3_2 = Conv2d_fuse(64, 64, 3, 1, leakyReLU=True)
        self.a_tracker3_2 = AveragedRangeTracker()
        self.pool3 = nn.MaxPool2d(2, 2)
        self.conv4_1 = Conv2d_fuse(64, 128, 3, 1, leakyReLU=True)
        self.a_tracker4_1 = AveragedRangeTracker()
        self.conv4_2 = Conv2d_fuse(128, 128, 3, 1, leakyReLU=True)
        self.a_tracker4_2 = AveragedRangeTracker()
        self.pool4 = nn.MaxPool2d(2, 2)
        self.conv5 = Conv2d_fuse(128, 256, 3, 1, leakyReLU=True)
        self.a_tracker5 = AveragedRangeTracker()
        self.conv6 = Conv2d_fuse(256, 256, 3, 1, leakyReLU=True)
        self.a_tracker6 = AveragedRangeTracker()
        self.conv7 = Conv2d_fuse(256, 256, 3, 1, leakyReLU=True)
        self.a_tracker7 = AveragedRangeTracker()
        self.pred = nn.Conv2d(256, self.anchor_number * (1 + 4 + self.num_classes), 3, 1, padding=1)
        self.a_tracker_pred = AveragedRangeTracker()

    PIPELINE_CHUNK = 64                 # images per ticket of the pipeline (BASELINE.json's batch: the kernels' tuned regime)

    @property
    def _engine(self):
        return self.__dict__.get("_engine_state", (None,))[0]

    @property
    def _pipe(self):                    # y355_pipeline: batches larger than PIPELINE_CHUNK and the asynchronous submit / collect
        return self.__dict__.get("_pipe_state", (None,))[0]

    # ------------------------------------------------------------------ reference API
    def set_grid(self, input_size):
        """models/slim_yolo_v2.py:105-109: change the network input size."""
        self.input_size = list(input_size)
        self.scale = np.array([[[input_size[1], input_size[0], input_size[1], input_size[0]]]])

    def forward(self, x, target=None, quantization=False, find=False):
        """Eval-mode return of the reference (:344-358): detections of image 0 as NumPy arrays
        (bboxes float32 [n,4] in [0,1], scores float32 [n], cls_inds int64 [n]), anchor order."""
        return self.forward_batch(x, quantization=quantization, find=find)[0]

    def forward_batch(self, x, quantization=True, find=False, sizes_wh=None):
        """Every image of the batch: element i equals forward(x[i:i+1]) of a frozen model.  sizes_wh ([B,2] original
        (width, height)): boxes come back in pixels of the original images -- the evaluators'
        `bboxes *= scale` (utils/vocapi_evaluator_mask.py:71-72) done on the GPU for the whole batch."""
        if self.trainable:
            raise NotImplementedError("yolo355 is an inference engine: the training branch "
                                      "(models/slim_yolo_v2.py:360-382) is out of scope")
        if not quantization:
            # models/slim_yolo_v2.py:212-358 with the default kwarg: every tracker returns its input (:17-18), so the
            # forward is conv + bias + LeakyReLU(0.125) / max-pool in fp32 on the loaded (possibly dyadic) weights; `find`
            # divides by 2^r weights that were multiplied by 2^r (:222-227), which cancels up to fp32 rounding.
            # Runs as the SlimYOLOv2 graph without BatchNorm on the bf16 MFMA (fp32 accumulation): tolerance parity.
            net = self._get_f32_net(int(x.shape[0]), find)
            net.set_thresholds(self.conf_thresh, self.nms_thresh)
            dets = net.forward(x)
            if sizes_wh is not None:                        # the evaluators' `bboxes *= scale` (utils/vocapi_evaluator.py:69-70)
                wh = np.asarray(sizes_wh, np.float32).reshape(-1, 2)
                dets = [(b * np.array([[w, h, w, h]], np.float32), s, c) for (b, s, c), (w, h) in zip(dets, wh)]
            return dets
        B = int(x.shape[0])
        trackers = self._tracker_states()
        freeze = not self.trainable
        if any(t.first_a == 0 for t in trackers) or not freeze:
            # first call ever (:25-27) calibrates every tracker on this input, layer by layer, on ONE handle holding the whole batch
            eng = self._get_engine(B, find)
            sa = eng.calibrate(x, trackers, freeze=freeze)
            self._store_trackers(trackers)
        else:
            sa = [t.exponent() for t in trackers]
        if B > self.PIPELINE_CHUNK:
            # more than one batch-64 forward: chunks in flight on the pipeline's handles (y355_pipeline), results in order
            return self._primed(self._get_pipeline(find), sa).forward(x, find=find, sizes_wh=sizes_wh)
        eng = self._primed(self._get_engine(B, find), sa)
        if sizes_wh is not None:
            return eng.forward_scaled(x, sizes_wh, find=find)
        return eng.forward(x, find=find)

    def submit_batch(self, x, quantization=True, find=False, sizes_wh=None):
        """Asynchronous forward_batch for callers that have host work per batch (the evaluator loops,
        utils/vocapi_evaluator_mask.py:57-82): enqueue the batch on the pipeline and return a token at once; collect_batch(token)
        gives what forward_batch would have returned.  Up to `pipeline depth` (8) chunks of PIPELINE_CHUNK images may be
        outstanding; the trackers must be calibrated (one forward(x, quantization=True) before)."""
        if not quantization or self.trainable:
            raise NotImplementedError("submit_batch runs the int8 path (quantization=True, eval)")
        sa = self._frozen_exponents()
        pipe = self._primed(self._get_pipeline(find), sa)
        return (pipe,) + pipe.submit_batch(x, sizes_wh)

    def submit_frame_list(self, frames, quantization=True, find=False, sizes_wh=None):
        """submit_batch for a list of camera frames, uint8 [h,w,3] BGR each of its own size (forward_frame_list's input);
        collect_batch(token) gives what forward_frame_list would have returned."""
        if not quantization or self.trainable:
            raise NotImplementedError("submit_frame_list runs the int8 path (quantization=True, eval)")
        sa = self._frozen_exponents()
        pipe = self._primed(self._get_pipeline(find), sa)
        return (pipe,) + pipe.submit_frame_batch(frames, sizes_wh)

    def collect_batch(self, token):
        pipe, tickets, _ = token
        out = []
        for t in tickets:
            out.extend(pipe.fetch(t))
        return out

    def calibrate(self, x, freeze=False, find=False):
        """One calibration step on a batch, the tracker side of the reference's calibration loop
        (retune_bias_quantize.py:357-369: `model(images, target, quantization=True)` in training mode, whose loss branch is
        out of scope here): every AveragedRangeTracker sees max|activation| over the batch -- first call: scale =
        127 / max; later calls: scale = 0.9 scale + 0.1 * 127 / max (models/slim_yolo_v2.py:25-31), or unchanged with
        freeze=True -- layer by layer on the GPU, each layer running with the exponent just updated.  The buffers
        `a_tracker*.scale / first_a` are updated in place (they travel in the state_dict).  Returns the 11 exponents.
        The weights must already be power-of-two quantized (prep.quantize_layers): the reference's loop runs its first
        batch on the un-quantized weights and quantizes afterwards, which moves the first scales by < 2 % (measured,
        tests/test_round2.py) and none of the exponents of the goldens."""
        eng = self._get_engine(int(x.shape[0]), find)
        trackers = self._tracker_states()
        sa = eng.calibrate(x, trackers, freeze=freeze)
        self._store_trackers(trackers)
        return sa

    def forward_frames(self, frames, find=False):
        """New: detections for camera frames, uint8 [B,H,W,3] BGR at the network size --
        BaseTransform + BGR->RGB + HWC->CHW (data/__init__.py:30-56, test.py:79) run inside the first
        layer.  Element i equals forward(x_i) for the tensor the reference's transform makes of frame i.
        The trackers must be calibrated (one forward on a normalised tensor) beforehand."""
        eng = self._get_engine(int(frames.shape[0]), find)
        return self._primed(eng, self._frozen_exponents()).forward_frames(frames, find=find)

    def forward_frame_list(self, frames, quantization=True, find=False, sizes_wh=None):
        """forward_frames for a list of frames, each uint8 [h,w,3] BGR of its own size (numpy, CPU or CUDA torch, mixed) --
        what the reference's callers have: one image at a time, resized per image by BaseTransform (data/__init__.py:30-56,
        test.py:79-90).  Element i equals forward_batch of the tensor the reference's transform makes of frame i, bit for bit.
        sizes_wh: None, an array [n,2], or "own": every image's boxes rescaled by its own (width, height) on the GPU.
        Up to PIPELINE_CHUNK frames run as one list forward on the engine, more as chunks in flight on the pipeline.
        quantization=True needs calibrated trackers (one forward(x, quantization=True) before); quantization=False runs
        the bf16 y355_net of forward_batch(quantization=False)."""
        framelist.check_frame_list(frames)
        if self.trainable:
            raise NotImplementedError("yolo355 is an inference engine: the training branch "
                                      "(models/slim_yolo_v2.py:360-382) is out of scope")
        n = len(frames)
        if not quantization:
            net = self._get_f32_net(n, find)
            net.set_thresholds(self.conf_thresh, self.nms_thresh)
            return net.forward_frame_list(frames, sizes_wh=sizes_wh)
        sa = self._frozen_exponents()
        target = self._get_pipeline(find) if n > self.PIPELINE_CHUNK else self._get_engine(n, find)
        return self._primed(target, sa).forward_frame_list(frames, find=find, sizes_wh=sizes_wh)

    # ------------------------------------------------------------------ engine plumbing
    def _weights_version(self):
        return tuple(int(p._version) for p in self.parameters()) + tuple(p.data_ptr() for p in self.parameters())

    def _frozen_exponents(self):
        """the 11 activation exponents of the calibrated trackers"""
        trackers = self._tracker_states()
        if any(t.first_a == 0 for t in trackers):
            raise RuntimeError("yolo355: calibrate the trackers with one forward(x, quantization=True) first")
        return [t.exponent() for t in trackers]

    def _primed(self, target, sa):
        """an Engine or a Pipeline with these exponents and the model's thresholds"""
        target.set_act_exponents(sa)
        target.set_thresholds(self.conf_thresh, self.nms_thresh)
        return target

    def _config(self):
        """(what a handle is rebuilt for, the arguments Engine / Pipeline / Net share)"""
        anchors = self.anchor_size.tolist()
        return ((tuple(self.input_size), self.num_classes, tuple(map(tuple, anchors))),
                (self.input_size, self.num_classes, anchors, self.conf_thresh, self.nms_thresh))

    def _get_engine(self, batch, find):
        key, args = self._config()
        return _cached(self.__dict__, "_engine_state", key, batch, (self._weights_version(), bool(find)),
                       lambda: Engine(*args, max_batch=max(batch, 1), device=_device(self), max_candidates=_cap(self)),
                       lambda eng: self._load_into(eng, find))

    def _load_into(self, target, find):
        """the ten dyadic layers of this model into an Engine or a Pipeline"""
        mods = [getattr(self, n).convs[0] for n in _CONVS] + [self.pred]
        for i, m in enumerate(mods):
            q_w, e_w = prep.as_dyadic_int8(m.weight)
            q_b, e_b = prep.as_dyadic_int8(m.bias)
            # find=True: the checkpoint holds W * 2^r and the reference divides the conv output
            # by 2^r (:222-227): same values as exponents e + r
            r = prep.RETUNE[i] if find else 0
            target.load_layer(i, q_w, q_b, e_w + r, e_b + r)
        target.set_retune(prep.RETUNE)

    def _get_pipeline(self, find):
        key, args = self._config()

        def load(pipe):
            pipe.sync()
            self._load_into(pipe, find)
        return _cached(self.__dict__, "_pipe_state", key, 0, (self._weights_version(), bool(find)),
                       lambda: Pipeline(*args, max_batch=self.PIPELINE_CHUNK, device=_device(self), max_candidates=_cap(self)), load)

    def _get_f32_net(self, batch, find):
        """y355_net (Y355_ARCH_SLIM_V2, bf16) loaded with this model's conv weights and biases as they are."""
        key, args = self._config()

        def load(net):
            for i, m in enumerate([getattr(self, n).convs[0] for n in _CONVS] + [self.pred]):
                w = m.weight.detach().float().cpu().numpy()
                b = m.bias.detach().float().cpu().numpy()
                if find:                                    # the checkpoint holds W * 2^r, the forward divides by 2^r
                    sc = np.float32(2.0 ** -prep.RETUNE[i])
                    w, b = w * sc, b * sc
                net.load_layer(i, w, b)
        return _cached(self.__dict__, "_f32", key, batch, (self._weights_version(), bool(find)),
                       lambda: Net("slim_yolo_v2", *args, max_batch=max(batch, 1), device=_device(self), dtype="bf16",
                                   max_candidates=_cap(self)), load)

    def _tracker_states(self):
        return [prep.RangeTracker(getattr(self, n).scale, int(getattr(self, n).first_a.item())) for n in _TRACKERS]

    def _store_trackers(self, trackers):
        with torch.no_grad():
            for n, t in zip(_TRACKERS, trackers):
                m = getattr(self, n)
                m.scale.copy_(t.scale.to(m.scale.device))
                m.first_a.fill_(float(t.first_a))


class _NetModel(nn.Module):
    """Shared plumbing of the fp32 model drop-ins: fold BN, load the engine, batched forward."""
    _arch = None

    def _conv_modules(self):
        raise NotImplementedError

    def _flat_anchors(self):
        return [list(map(float, a)) for a in self.anchor_size.view(-1, 2).tolist()]

    def set_grid(self, input_size):
        self.input_size = list(input_size)
        self.scale = np.array([[[input_size[1], input_size[0], input_size[1], input_size[0]]]])

    def _check_inference(self):
        if self.trainable:
            raise NotImplementedError("yolo355 is an inference engine: the training branch is out of scope")
        if self.training and any(isinstance(m, nn.BatchNorm2d) for m in self.modules()):
            raise NotImplementedError("yolo355 folds BatchNorm with its running statistics: call .eval() first")

    def forward_batch(self, x, quantization=False, sizes_wh=None):
        """Every image of the batch.  quantization=True (YOLOv3tiny, YOLOv2, YOLOv3, YOLOv3-SPP) runs the int8 engine:
        weights quantized per tensor (self.channel_level: per output channel) to power-of-two int8 after the BN fold, activation exponents
        frozen at the first quantized call from the bf16 run of that input -- the first-call rule of
        AveragedRangeTracker (models/slim_yolo_v2.py:25-27) applied to this graph.
        sizes_wh: [B,2] original (width, height) per image: the boxes come back in pixels of the original images
        (the evaluators' `bboxes *= [[w, h, w, h]]`, test.py:88-90, on the GPU)."""
        self._check_inference()
        if quantization and self.act_exponents is None:    # (a model calibrate()d on its int8 net never builds the bf16 one)
            self.act_exponents = self._get_net(int(x.shape[0])).calibration_exponents(x)
        return self._ready_net(int(x.shape[0]), quantization).forward(x, sizes_wh=sizes_wh)

    def _ready_net(self, batch, quantization):
        """the bf16 net, or the int8 net with the frozen activation exponents, at the model's thresholds"""
        if quantization and self.act_exponents is None:
            raise RuntimeError("yolo355: the int8 activation exponents are not frozen yet: run one "
                               "forward_batch(x, quantization=True) first")
        net = self._get_net(batch, int8=bool(quantization))
        if quantization:
            net.set_act_exponents(*self.act_exponents)
        net.set_thresholds(self.conf_thresh, self.nms_thresh)
        return net

    def forward_frames(self, frames, quantization=False, sizes_wh=None):
        """New: detections for camera frames as cv2 delivers them, uint8 [B,h,w,3] BGR of any size.
        BaseTransform (data/__init__.py:30-56), BGR->RGB and HWC->CHW (test.py:79-85) run on the GPU inside the op that
        reads the network input; element i equals forward_batch of the tensor the reference's transform makes of frame
        i, bit for bit.  quantization=True needs the frozen activation exponents: run one
        forward_batch(x, quantization=True) first.  sizes_wh as forward_batch."""
        Net.check_frames(frames)
        self._check_inference()
        return self._ready_net(int(frames.shape[0]), quantization).forward_frames(frames, sizes_wh=sizes_wh)

    def forward_frame_list(self, frames, quantization=False, sizes_wh=None):
        """forward_frames for a list of frames, each uint8 [h,w,3] BGR of its own size (numpy, CPU or CUDA torch, mixed) --
        what the reference's callers have: one image at a time, resized per image by BaseTransform.  Element i equals
        forward_frames(frames[i][None])[0], bit for bit.  sizes_wh="own" rescales every image's boxes by its own
        (width, height) on the GPU (test.py:88-90); an array as forward_batch.  quantization=True needs the frozen
        activation exponents, as forward_frames."""
        Net.check_frame_list(frames)
        self._check_inference()
        return self._ready_net(len(frames), quantization).forward_frame_list(frames, sizes_wh=sizes_wh)

    def calibrate_frame_list(self, frames, freeze=False):
        """calibrate() on a list of camera frames of any sizes (Net.calibrate_frame_list)."""
        Net.check_frame_list(frames)
        return self._calibrate_step(lambda net: net.calibrate_frame_list(frames, freeze=freeze), len(frames))

    def calibrate(self, x, freeze=False):
        """One calibration step on the int8 net itself (Net.calibrate): the reference's forward(x, quantization=True)
        with freeze = not trainable (models/slim_yolo_v2.py:212-328; the loop of retune_bias_quantize.py:357-369) on this
        graph -- first call: scale = 127 / max; later calls the EMA, or unchanged with freeze=True.  No bf16 net is built.
        Stores act_exponents for forward_batch(x, quantization=True) / forward_frames and keeps the tracker state in the
        buffers act_tracker_scale / act_tracker_first_a (registered at the first call: they travel in the state_dict).
        Returns (sa_in, [sa per tensor])."""
        return self._calibrate_step(lambda net: net.calibrate(x, freeze=freeze), int(x.shape[0]))

    def calibrate_frames(self, frames, freeze=False):
        """calibrate() on camera frames, uint8 [B,h,w,3] BGR of any size (Net.calibrate_frames)."""
        Net.check_frames(frames)
        return self._calibrate_step(lambda net: net.calibrate_frames(frames, freeze=freeze), int(frames.shape[0]))

    def _calibrate_step(self, step, batch):
        self._check_inference()
        qnet = self._get_net(batch, int8=True)
        if hasattr(self, "act_tracker_scale"):             # the state this model carries (a reloaded state_dict, an earlier net)
            qnet.trackers = (self.act_tracker_scale.cpu().numpy(), self.act_tracker_first_a.cpu().numpy())
        self.act_exponents = step(qnet)
        scale, first = qnet.trackers
        self._register_trackers(len(scale))
        with torch.no_grad():
            self.act_tracker_scale.copy_(torch.from_numpy(scale))
            self.act_tracker_first_a.copy_(torch.from_numpy(first))
        return self.act_exponents

    def _register_trackers(self, n):
        if not hasattr(self, "act_tracker_scale"):
            self.register_buffer("act_tracker_scale", torch.zeros(n, dtype=torch.float32))
            self.register_buffer("act_tracker_first_a", torch.zeros(n, dtype=torch.int32))

    def load_state_dict(self, state_dict, *args, **kwargs):
        """A calibrated model's state_dict carries its tracker buffers: they are registered here before the load, and the
        exponents floor(log2(scale)) (models/slim_yolo_v2.py:33) become act_exponents again -- only when every tracker has
        seen a batch (first_a != 0 everywhere); otherwise act_exponents stays as it was.  A model that has been calibrated
        has the two buffers for good: loading an uncalibrated state_dict into it needs strict=False."""
        if "act_tracker_scale" in state_dict:
            self._register_trackers(int(state_dict["act_tracker_scale"].shape[0]))
        out = super().load_state_dict(state_dict, *args, **kwargs)
        if "act_tracker_scale" in state_dict and bool((self.act_tracker_first_a != 0).all()):
            e = [prep.RangeTracker(s.reshape(1), 1).exponent() for s in self.act_tracker_scale.detach().cpu()]
            self.act_exponents = (e[0], e[1:])
        return out

    def _weights_version(self):
        t = list(self.parameters()) + [b for n, b in self.named_buffers() if not n.startswith("act_tracker_")]
        return tuple(int(p._version) for p in t) + tuple(p.data_ptr() for p in t)

    act_exponents = None      # (sa_in, [sa per tensor]) of the int8 path, frozen at the first quantized call
    # int8 path: one power-of-two weight scale per output channel instead of one per layer (quantize_tensor's
    # channel_level, retune_bias_quantize.py:73-86), exponents at most max_spread apart (None: prep.DEFAULT_MAX_SPREAD).
    # Set before the first quantized call, or any time: the int8 net reloads when they change
    channel_level = False
    max_spread = None

    def _get_net(self, batch, int8=False):
        anchors = self._flat_anchors()
        ver = self._weights_version() + ((bool(self.channel_level), self.max_spread) if int8 else ())

        def load(net):
            folded = [folded_f32(m) for m in self._conv_modules()]
            if int8:
                for i, q in enumerate(prep.quantize_folded(folded, bool(self.channel_level), self.max_spread)):
                    net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
            else:
                for i, (w, b) in enumerate(folded):
                    net.load_layer(i, w, b)
        return _cached(self.__dict__.setdefault("_nets", {}), "q" if int8 else "f", (tuple(self.input_size), self.num_classes, tuple(map(tuple, anchors))), batch, ver,
                       lambda: Net(self._arch, self.input_size, self.num_classes, anchors, self.conf_thresh, self.nms_thresh,
                                   max_batch=max(batch, 1), device=_device(self), dtype="int8" if int8 else "bf16",
                                   max_candidates=_cap(self)), load)


class SlimYOLOv2(_NetModel):
    """Drop-in for the reference's fp32 model (models/slim_yolo_v2.py:385-622): same constructor,
    modules (utils.modules.Conv2d = conv + BN + LeakyReLU(0.125)), state_dict keys and eval-mode
    return.  Inference runs BN-folded on the MI355X with bf16 MFMA and fp32 accumulation
    (include/yolo355.h, y355_net); `quantization` / `find` are accepted and ignored like the
    reference does (:549)."""
    _arch = "slim_yolo_v2"

    def __init__(self, device, input_size=None, num_classes=20, trainable=False, conf_thresh=0.01,
                 nms_thresh=0.5, anchor_size=None, hr=False, max_candidates=4096):
        super().__init__()
        self.max_candidates = int(max_candidates)      # most anchors of an image that may pass conf_thresh (Engine / Net max_candidates)
        self.device = device
        self.input_size = list(input_size)
        self.num_classes = num_classes
        self.trainable = trainable
        self.conf_thresh = conf_thresh
        self.nms_thresh = nms_thresh
        self.anchor_size = torch.tensor(anchor_size)
        self.anchor_number = len(anchor_size)
        self.stride = 16
        self.scale = np.array([[[input_size[1], input_size[0], input_size[1], input_size[0]]]])
        self.conv1 = Conv2d(3, 16, 3, 1, leakyReLU=True)
        self.pool1 = nn.MaxPool2d(2, 2)
        self.conv2 = Conv2d(16, 32, 3, 1, leakyReLU=True)
        self.pool2 = nn.MaxPool2d(2, 2)
        self.conv3_1 = Conv2d(32, 64, 3, 1, leakyReLU=True)
        self.conv3_2 = Conv2d(64, 64, 3, 1, leakyReLU=True)
        self.pool3 = nn.MaxPool2d(2, 2)
        self.conv4_1 = Conv2d(64, 128, 3, 1, leakyReLU=True)
        self.conv4_2 = Conv2d(128, 128, 3, 1, leakyReLU=True)
        self.pool4 = nn.MaxPool2d(2, 2)
        self.conv5 = Conv2d(128, 256, 3, 1, leakyReLU=True)
        self.conv6 = Conv2d(256, 256, 3, 1, leakyReLU=True)
        self.conv7 = Conv2d(256, 256, 3, 1, leakyReLU=True)
        self.pred = nn.Conv2d(256, self.anchor_number * (1 + 4 + self.num_classes), 3, 1, padding=1)

    def _conv_modules(self):
        return [getattr(self, n).convs for n in _CONVS] + [self.pred]

    def forward(self, x, target=None, quantization=False, find=False):
        """Eval-mode return of the reference (:585-601): detections of image 0."""
        return self.forward_batch(x)[0]
