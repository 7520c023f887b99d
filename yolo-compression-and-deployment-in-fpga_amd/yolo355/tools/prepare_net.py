"""Weight preparation of the y355_net families as one command: fp32 checkpoint of SlimYOLOv2, YOLOv3tiny, YOLOv2, YOLOv3
or YOLOv3-SPP -> BN fold -> power-of-two int8 weights (per tensor or per output channel) -> tracker calibration ON THE INT8
NET -> engine package.  It is tools/prepare.py for the general engine:

    utils.modules.folded_f32                  the exact eval-mode fold of conv + BatchNorm
    retune_bias_quantize.py:73-119            prep.quantize_folded (--channel-level, --max-spread)
    retune_bias_quantize.py:357-369           the calibration loop, Net.calibrate / Net.calibrate_frames per batch

    python -m yolo355.tools.prepare_net --version yolo_v2 --weights yolo_v2.pth --out out/yolo_v2_q --num-classes 20 \\
           --size 416 416 [--calib frames.npy] [--calib-batch 32] [--channel-level] [--max-spread 4]

writes  out/yolo_v2_q.npz   integer weights and exponents per layer, the activation exponents, the tracker state, meta;
                            netengine.Net.from_package(path) runs it without any fp32 weights
Calibration runs on the GPU engine (there is no CPU path)."""
import argparse
import json

import numpy as np
import torch

from .. import prep, synth
from ..netengine import Net
from ..utils.modules import folded_f32
from .prepare import calib_batches

VERSIONS = ("slim_yolo_v2", "tiny_yolo_v3", "yolo_v2", "yolo_v3", "yolo_v3_spp")


def model_class(version):
    from .. import models
    from ..models import yolo_v2, yolo_v3
    return {"slim_yolo_v2": lambda: models.SlimYOLOv2, "tiny_yolo_v3": lambda: models.YOLOv3tiny, "yolo_v2": lambda: yolo_v2.myYOLOv2,
            "yolo_v3": lambda: yolo_v3.myYOLOv3, "yolo_v3_spp": lambda: yolo_v3.myYOLOv3Spp}[version]()


def default_anchors(version, num_classes):
    if version == "tiny_yolo_v3":
        return synth.TINY_MULTI_ANCHOR_SIZE
    if version in ("yolo_v3", "yolo_v3_spp"):
        return synth.MULTI_ANCHOR_SIZE
    if version == "slim_yolo_v2" and num_classes == 2:
        return synth.ANCHOR_SIZE_MASK
    return synth.ANCHOR_SIZE


def prepare(version, state_dict, num_classes, anchor_size, input_size, calib, device="cuda:0", conf_thresh=0.01, nms_thresh=0.5,
            calib_batch=0, calib_images=1000, channel_level=False, max_spread=None):
    """Returns (net, package dict): the calibrated int8 Net and what main() writes.  calib: fp32 NCHW tensor / array
    (already normalised) or uint8 [B,h,w,3] BGR frames of any size.  calib_batch = 0: the FIRST image calibrates the trackers,
    frozen (the first-call rule of an eval-mode model, models/slim_yolo_v2.py:25-27); N > 0: the reference's loop over
    batches of N images, first batch sets every scale, every further one moves it by the EMA of :30-31, as many batches as
    prepare.calib_batches gives."""
    fp = model_class(version)(device, input_size=list(input_size), num_classes=num_classes, trainable=False,
                              conf_thresh=conf_thresh, nms_thresh=nms_thresh, anchor_size=anchor_size)
    fp.load_state_dict(state_dict)
    fp.eval()
    anchors = fp._flat_anchors()
    layers = prep.quantize_folded([folded_f32(m) for m in fp._conv_modules()], bool(channel_level), max_spread)
    x = calib.detach().cpu().numpy() if isinstance(calib, torch.Tensor) else np.asarray(calib)
    frames = x.dtype == np.uint8
    if not frames:
        x = np.ascontiguousarray(x, dtype=np.float32)
    n = calib_batch if calib_batch > 0 else 1
    net = Net(version, input_size, num_classes, anchors, conf_thresh, nms_thresh, max_batch=n, device=device, dtype="int8")
    for i, q in enumerate(layers):
        net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
    step = net.calibrate_frames if frames else net.calibrate
    if calib_batch > 0:
        for it in range(calib_batches(x.shape[0], calib_batch, calib_images)):
            step(x[it * calib_batch:(it + 1) * calib_batch], freeze=False)
    else:
        step(x[:1], freeze=True)
    sa_in, sa = net.get_act_exponents()
    scale, first = net.trackers
    meta = dict(arch=version, input_size=[int(v) for v in input_size], num_classes=int(num_classes), anchors=anchors,
                conf_thresh=float(conf_thresh), nms_thresh=float(nms_thresh), channel_level=bool(channel_level),
                num_layers=len(layers))
    package = dict(meta=json.dumps(meta), sa_in=np.int32(sa_in), sa=np.asarray(sa, np.int32), tracker_scale=scale,
                   tracker_first_a=first)
    for i, q in enumerate(layers):
        package["q_w_%d" % i] = np.asarray(q["q_w"]).astype(np.int8)
        package["q_b_%d" % i] = np.asarray(q["q_b"]).astype(np.int32)
        package["e_w_%d" % i] = np.asarray(q["e_w"], np.int32)              # 0-d: one exponent; [cout]: one per output channel
        package["e_b_%d" % i] = np.int32(q["e_b"])
    return net, package


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--version", required=True, choices=VERSIONS)
    ap.add_argument("--weights", required=True, help="fp32 state_dict (.pth) of the --version model")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--num-classes", type=int, default=20)
    ap.add_argument("--size", type=int, nargs=2, default=[416, 416], metavar=("H", "W"))
    ap.add_argument("--calib", help=".npy with uint8 [B,h,w,3] BGR frames or fp32 [B,3,H,W]; default: a synthetic frame")
    ap.add_argument("--calib-batch", type=int, default=0,
                    help="N > 0: the reference's calibration loop (retune_bias_quantize.py:357-369) over the --calib file in "
                         "batches of N (EMA trackers); 0: first image only, frozen")
    ap.add_argument("--calib-images", type=int, default=1000, help="stop the loop once more images than this were seen (:365)")
    ap.add_argument("--channel-level", action="store_true", help="one weight exponent per output channel")
    ap.add_argument("--max-spread", type=int, default=None, help="--channel-level: largest gap between a layer's exponents")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    sd = torch.load(args.weights, map_location="cpu")
    calib = np.load(args.calib) if args.calib else synth.make_frames_u8(1, 1, args.size[0], args.size[1], "blocks")
    net, package = prepare(args.version, sd, args.num_classes, default_anchors(args.version, args.num_classes), args.size, calib,
                           args.device, calib_batch=args.calib_batch, calib_images=args.calib_images,
                           channel_level=args.channel_level, max_spread=args.max_spread)
    np.savez_compressed(args.out + ".npz", **package)
    sa_in, sa = net.get_act_exponents()
    print("activation exponents: input %d, tensors %s" % (sa_in, sa))
    print("wrote", args.out + ".npz")
    net.close()


if __name__ == "__main__":
    main()
