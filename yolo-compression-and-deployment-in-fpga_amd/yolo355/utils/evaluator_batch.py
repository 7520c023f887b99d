"""Evaluator-side batching.  The reference's evaluators call the network one image at a time
(utils/vocapi_evaluator_mask.py:57-82, utils/vocapi_evaluator.py, utils/cocoapi_evaluator.py:70-98) and rescale the
boxes on the host.  These helpers produce the same data structures with batched forwards and the rescale on the GPU
(`forward_batch(..., sizes_wh=...)` -> y355_scale_boxes); the VOC mAP computation that follows them (evaluate_detections:
write_voc_results_file + voc_eval, :140-341) is `voc_map` / `voc_map_from_all_boxes` below, on the GPU (yolo355.apeval); COCO's
(pycocotools' COCOeval, utils/cocoapi_evaluator.py:100-124) is `coco_map` / `coco_stats_from_data_dict`, on the GPU as well.

    # utils/vocapi_evaluator_mask.py:49-95  (evaluate)
    - for i in range(num_images): ... bboxes, scores, cls_inds = net(x, quantization=..., find=...) ...
    + self.all_boxes = voc_all_boxes(net, self.dataset, len(self.labelmap), batch_size=64, quantization=quantization, find=find)

    # utils/cocoapi_evaluator.py:66-98
    + ids, data_dict = coco_data_dict(model, self.dataset, self.transform, batch_size=64)

Both helpers are software-pipelined over the y355_pipeline behind a calibrated q_bf model (`_submit`): batch k + 1 is submitted
before batch k is unpacked, so the GPU runs while the host loads images and builds the evaluator's lists.
"""
import numpy as np
import torch

from .. import _ffi
from .._handle import raise_overflow


def _batches(n, bs):
    for i0 in range(0, n, bs):
        yield i0, min(n, i0 + bs)


def _run(net, x, sizes_wh, **kw):
    """One batched forward with the evaluators' rescale.  Only the keyword arguments the model's forward_batch declares
    are passed (decided from its signature, never by catching TypeError: an exception raised inside a forward must
    surface); asking a model for `quantization=True` / `find=True` that it cannot honour is an error, not a silent
    fp32 evaluation.  A q_bf model whose trackers are still un-calibrated is first run on image 0 alone: the
    reference's per-image loop freezes every tracker on its first image (models/slim_yolo_v2.py:25-27), a batched
    first call would calibrate on the maximum over the whole batch."""
    import inspect
    if not hasattr(net, "forward_batch"):
        raise TypeError("evaluator batching needs a yolo355 model (forward_batch)")
    params = inspect.signature(net.forward_batch).parameters
    for k in ("quantization", "find"):
        if kw.get(k) and k not in params:
            raise TypeError("%s.forward_batch does not take %s=True" % (type(net).__name__, k))
    call = {k: v for k, v in kw.items() if k in params}
    if call.get("quantization") and hasattr(net, "_tracker_states") and any(t.first_a == 0 for t in net._tracker_states()):
        net.forward_batch(x[:1], **call)
    if "sizes_wh" in params:
        return net.forward_batch(x, sizes_wh=sizes_wh, **call)
    # models without the fused rescale (the composed wider families): rescale like the reference, per image
    res = []
    for (b, s, c), (w, h) in zip(net.forward_batch(x, **call), sizes_wh):
        b = b.copy()
        b *= np.array([[w, h, w, h]])
        res.append((b, s, c))
    return res


def _submit(net, x, sizes_wh, **kw):
    """Start one batch and return a zero-argument function that delivers its detections.  A calibrated q_bf model
    (quantization=True, no guard) goes through submit_batch / collect_batch -- the y355_pipeline behind the model: the GPU works
    on this batch while the caller loads the next one and unpacks the previous one; everything else runs synchronously in _run."""
    if (kw.get("quantization") and not kw.get("find") and hasattr(net, "submit_batch") and hasattr(net, "_tracker_states")
            and all(t.first_a != 0 for t in net._tracker_states()) and int(x.shape[0]) <= 2 * _ffi.PIPE_DEFAULT_HANDLES * getattr(net, "PIPELINE_CHUNK", 0)):
        token = net.submit_batch(x, quantization=True, find=False, sizes_wh=sizes_wh)
        return lambda: net.collect_batch(token)
    dets = _run(net, x, sizes_wh, **kw)
    return lambda: dets


def voc_all_boxes(net, dataset, num_classes, batch_size=64, quantization=False, find=False, num_images=None):
    """all_boxes[cls][image] = N x 5 float32 (x1, y1, x2, y2, score) exactly as the loop of
    utils/vocapi_evaluator_mask.py:57-82 builds it; dataset.pull_item(i) -> (im [3,H,W] tensor, gt, h, w)."""
    n = len(dataset) if num_images is None else int(num_images)
    all_boxes = [[[] for _ in range(n)] for _ in range(num_classes)]
    def unpack(i0, dets):
        for k, (bboxes, scores, cls_inds) in enumerate(dets):
            i = i0 + k
            for j in range(num_classes):
                inds = np.where(cls_inds == j)[0]
                if len(inds) == 0:
                    all_boxes[j][i] = np.empty([0, 5], dtype=np.float32)
                    continue
                all_boxes[j][i] = np.hstack((bboxes[inds], scores[inds][:, np.newaxis])).astype(np.float32, copy=False)
    pending = None                                      # (first image, deliver) of the batch the GPU is working on
    for i0, i1 in _batches(n, batch_size):
        ims, sizes = [], []
        for i in range(i0, i1):
            im, gt, h, w = dataset.pull_item(i)
            ims.append(torch.as_tensor(im))
            sizes.append((w, h))
        x = torch.stack(ims).float()
        deliver = _submit(net, x, np.asarray(sizes, np.float32), quantization=quantization, find=find)
        if pending is not None:
            unpack(pending[0], pending[1]())
        pending = (i0, deliver)
    if pending is not None:
        unpack(pending[0], pending[1]())
    return all_boxes


def coco_data_dict(net, dataset, transform, batch_size=64, num_images=None, **kw):
    """(ids, data_dict) exactly as utils/cocoapi_evaluator.py:66-98 builds them: dataset.pull_image(i) -> (img HWC BGR,
    id); transform(img)[0] -> HWC float image at the network size; dataset.class_ids maps class index -> COCO id."""
    n = len(dataset) if num_images is None else int(num_images)
    ids, data_dict = [], []
    def unpack(bids, dets):
        for id_, (bboxes, scores, cls_inds) in zip(bids, dets):
            ids.append(id_)
            for k, box in enumerate(bboxes):
                x1, y1, x2, y2 = float(box[0]), float(box[1]), float(box[2]), float(box[3])
                data_dict.append({"image_id": id_, "category_id": dataset.class_ids[int(cls_inds[k])],
                                  "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(scores[k])})
    pending = None
    for i0, i1 in _batches(n, batch_size):
        xs, sizes, bids = [], [], []
        for i in range(i0, i1):
            img, id_ = dataset.pull_image(i)
            xs.append(torch.from_numpy(np.ascontiguousarray(transform(img)[0][:, :, (2, 1, 0)])).permute(2, 0, 1))
            sizes.append((img.shape[1], img.shape[0]))
            bids.append(int(id_))
        deliver = _submit(net, torch.stack(xs).float(), np.asarray(sizes, np.float32), **kw)
        if pending is not None:
            unpack(pending[0], pending[1]())
        pending = (bids, deliver)
    if pending is not None:
        unpack(pending[0], pending[1]())
    return ids, data_dict


def _frame_batches(net, dataset, n, batch_size, **kw):
    """(first image, ids, detections) per batch of raw frames: dataset.pull_image(i) -> (img uint8 HWC BGR of any size, id),
    forward_frame_list with every image's boxes rescaled by its own (w, h) on the GPU.  No host transform."""
    if not hasattr(net, "forward_frame_list"):
        raise TypeError("%s has no forward_frame_list (the yolo355 model drop-ins have)" % type(net).__name__)
    for i0, i1 in _batches(n, batch_size):
        frames, bids = [], []
        for i in range(i0, i1):
            img, id_ = dataset.pull_image(i)
            frames.append(img)
            bids.append(id_)
        yield i0, bids, net.forward_frame_list(frames, sizes_wh="own", **kw)


def voc_all_boxes_frames(net, dataset, num_classes, batch_size=64, quantization=False, num_images=None):
    """voc_all_boxes from the raw images: all_boxes[cls][image] = N x 5 float32 (x1, y1, x2, y2, score) as the loop of
    utils/vocapi_evaluator_mask.py:57-82 builds it, with BaseTransform's resize and normalisation on the GPU.
    dataset.pull_image(i) -> (img uint8 HWC BGR of any size, id) (data/voc0712.py:148-160); net: a yolo355 model drop-in (the int8 SlimYOLOv2
    or a y355_net family).

        # utils/vocapi_evaluator_mask.py:49-95  (evaluate)
        - for i in range(num_images):
        -     im, gt, h, w = self.dataset.pull_item(i)
        -     x = Variable(im.unsqueeze(0)).to(self.device)
        -     bboxes, scores, cls_inds = net(x, quantization=..., find=...)
        -     scale = np.array([[w, h, w, h]]); bboxes *= scale ...
        + self.all_boxes = voc_all_boxes_frames(net, self.dataset, len(self.labelmap), batch_size=64, quantization=quantization)
    """
    n = len(dataset) if num_images is None else int(num_images)
    all_boxes = [[[] for _ in range(n)] for _ in range(num_classes)]
    for i0, _, dets in _frame_batches(net, dataset, n, batch_size, quantization=quantization):
        for k, (bboxes, scores, cls_inds) in enumerate(dets):
            for j in range(num_classes):
                inds = np.where(cls_inds == j)[0]
                if len(inds) == 0:
                    all_boxes[j][i0 + k] = np.empty([0, 5], dtype=np.float32)
                    continue
                all_boxes[j][i0 + k] = np.hstack((bboxes[inds], scores[inds][:, np.newaxis])).astype(np.float32, copy=False)
    return all_boxes


def coco_data_dict_frames(net, dataset, batch_size=64, num_images=None, **kw):
    """coco_data_dict from the raw images: (ids, data_dict) as utils/cocoapi_evaluator.py:66-98 builds them, without the
    host transform.  dataset.pull_image(i) -> (img uint8 HWC BGR of any size, id); dataset.class_ids maps class index ->
    COCO id; kw: quantization=... of forward_frame_list.

        # utils/cocoapi_evaluator.py:66-98
        - for index in range(num_images):
        -     img, id_ = self.dataset.pull_image(index)
        -     x = torch.from_numpy(self.transform(img)[0][:, :, (2, 1, 0)]).permute(2, 0, 1)
        -     bboxes, scores, cls_inds = model(x.unsqueeze(0).to(self.device)); bboxes *= scale ...
        + ids, data_dict = coco_data_dict_frames(model, self.dataset, batch_size=64)
    """
    n = len(dataset) if num_images is None else int(num_images)
    ids, data_dict = [], []
    for _, bids, dets in _frame_batches(net, dataset, n, batch_size, **kw):
        for id_, (bboxes, scores, cls_inds) in zip(bids, dets):
            id_ = int(id_)
            ids.append(id_)
            for k, box in enumerate(bboxes):
                x1, y1, x2, y2 = float(box[0]), float(box[1]), float(box[2]), float(box[3])
                data_dict.append({"image_id": id_, "category_id": dataset.class_ids[int(cls_inds[k])],
                                  "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(scores[k])})
    return ids, data_dict


# ---------------------------------------------------------------------------------------------------- VOC mAP (yolo355.apeval)
def voc_ground_truth(annopath, image_ids, labelmap):
    """The ground truth voc_eval reads (utils/vocapi_evaluator_mask.py:98-115, :257-268), as ApEval takes it: one array per image
    of rows (cls, xmin, ymin, xmax, ymax, difficult).  annopath: the '%s.xml' pattern of the VOC Annotations directory;
    image_ids: the names of the image-set file, in dataset order; objects whose name is not in labelmap are skipped (voc_eval
    never selects them)."""
    import xml.etree.ElementTree as ET
    index = {name: i for i, name in enumerate(labelmap)}
    gts = []
    for image_id in image_ids:
        rows = []
        for obj in ET.parse(annopath % image_id).findall("object"):
            c = index.get(obj.find("name").text.strip())
            if c is None:
                continue
            d = obj.find("difficult")
            bb = obj.find("bndbox")
            rows.append([c] + [float(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")] + [int(d.text) if d is not None else 0])
        gts.append(np.asarray(rows, np.float64).reshape(-1, 6))
    return gts


def voc_map_from_all_boxes(all_boxes, ground_truth, use_07_metric=True, ovthresh=0.5):
    """The replacement for evaluate_detections(box_list) (utils/vocapi_evaluator_mask.py:339-341): all_boxes[cls][image] = N x 5
    (x1, y1, x2, y2, score) or [] / an empty array -> (aps float64 [C], mean).  The reference's own write_voc_results_file stops
    at `if dets == []` on NumPy >= 2; here nothing is written: the file's rounding is part of ApEval's arithmetic."""
    from ..apeval import ApEval
    C, n = len(all_boxes), len(ground_truth)
    per = [[np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5) for j in range(C)] for i in range(n)]
    ev = ApEval(C, ground_truth, max_dets=max(1, sum(len(a) for p in per for a in p)))
    try:
        for i0, i1 in _batches(n, 1024):
            # per image the classes in ascending order: every class keeps the order of its own results file
            ev.add_detections(i0, [(np.concatenate([a[:, :4] for a in p]), np.concatenate([a[:, 4] for a in p]),
                                    np.concatenate([np.full(len(a), j, np.int32) for j, a in enumerate(p)])) for p in per[i0:i1]])
        return ev.compute(ovthresh=ovthresh, use_07_metric=use_07_metric)
    finally:
        ev.close()


def _pipeline_admits(net, batch, quantization=False, find=False):
    """_submit's rule for the y355_pipeline behind a calibrated q_bf model, restated (the existing helpers stay as they are);
    tests/test_voc_ap_ref.py holds the two together"""
    return bool(quantization and not find and hasattr(net, "submit_batch") and hasattr(net, "_tracker_states")
                and all(t.first_a != 0 for t in net._tracker_states())
                and batch <= 2 * _ffi.PIPE_DEFAULT_HANDLES * getattr(net, "PIPELINE_CHUNK", 0))


def voc_map(net, dataset, num_classes, ground_truth, batch_size=64, quantization=False, find=False, num_images=None,
            use_07_metric=True, max_dets=None):
    """The whole evaluate() of utils/vocapi_evaluator_mask.py:49-95 -> (aps float64 [C], mean): voc_all_boxes' loop with the mAP
    behind it.  A calibrated q_bf model (the rule of _submit) is device-resident end to end: Pipeline.submit -> scale_boxes ->
    ApEval.add on the ticket's stream -> release; no detection is copied to the host and nothing waits for the GPU before
    compute().  Every other model goes through forward_batch(..., sizes_wh=) and ApEval.add_detections.
    dataset.pull_item(i) -> (im [3,H,W] tensor, gt, h, w); ground_truth: voc_ground_truth(...) for the same images."""
    from ..apeval import ApEval
    n = len(dataset) if num_images is None else int(num_images)
    dev = net.device if isinstance(getattr(net, "device", None), (str, torch.device)) else "cuda:0"
    ev = ApEval(num_classes, ground_truth[:n], max_dets=max_dets, device=dev)
    try:
        out = []            # (pipeline, ticket, token) of the batch before: its overflow flag is read one batch late, and the token
                            # keeps what the ticket's launches read (the sizes scale_boxes multiplies by) alive until then
        def settle():
            for pipe, t, _ in out:
                if pipe.overflow(t):                        # as Pipeline.fetch reports it
                    raise_overflow(pipe.max_candidates)
            del out[:]
        for i0, i1 in _batches(n, batch_size):
            ims, sizes = [], []
            for i in range(i0, i1):
                im, gt, h, w = dataset.pull_item(i)
                ims.append(torch.as_tensor(im))
                sizes.append((w, h))
            x = torch.stack(ims).float()
            sizes = np.asarray(sizes, np.float32)
            if _pipeline_admits(net, i1 - i0, quantization=quantization, find=find):
                token = net.submit_batch(x, quantization=True, find=False, sizes_wh=sizes)
                pipe, tickets, wh = token
                settle()
                for k, t in enumerate(tickets):
                    first = i0 + k * pipe.max_batch
                    st = pipe.stream(t)
                    ev.add(first, *pipe.outputs(t), after_stream=st, batch=min(i1 - first, pipe.max_batch))
                    with torch.cuda.stream(st):             # the append just queued there is the last reader of the ticket's outputs
                        pipe.release(t)
                    if wh is not None:
                        wh.record_stream(st)                # the caching allocator must not hand the block on before scale_boxes ran
                    out.append((pipe, t, token))
            else:
                settle()
                ev.add_detections(i0, _run(net, x, sizes, quantization=quantization, find=find))
        settle()
        return ev.compute(use_07_metric=use_07_metric)
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- COCO AP (yolo355.apeval)
def coco_ground_truth(annotations, image_ids, class_ids):
    """The ground truth COCOeval reads from an instances_*.json, as CocoEval takes it: one float64 array per image of rows
    (cls, x, y, w, h, area, iscrowd), annotations in file order.  annotations: the path of the file or its loaded dict; image_ids:
    the ids the evaluator's loop returns, in its order; class_ids: dataset.class_ids (class index -> COCO category id);
    annotations of other categories or other images are skipped."""
    if not isinstance(annotations, dict):
        import json
        with open(annotations) as f:
            annotations = json.load(f)
    index = {int(c): k for k, c in enumerate(class_ids)}
    where = {int(id_): i for i, id_ in enumerate(image_ids)}
    if len(where) != len(image_ids):
        raise ValueError("duplicate image ids")
    rows = [[] for _ in image_ids]
    for ann in annotations["annotations"]:
        i, k = where.get(int(ann["image_id"])), index.get(int(ann["category_id"]))
        if i is None or k is None:
            continue
        x, y, w, h = ann["bbox"]
        rows[i].append([k, x, y, w, h, ann["area"], int(ann.get("iscrowd", 0))])
    return [np.asarray(r, np.float64).reshape(-1, 7) for r in rows]


class CocoStats(tuple):
    """(stats[0], stats[1]) as COCOAPIEvaluator.evaluate returns them; .stats: all twelve; .precision / .recall: COCOeval.eval's"""
    stats = precision = recall = None


def _coco_result(ev):
    stats = ev.compute()
    res = CocoStats((float(stats[0]), float(stats[1])))
    res.stats, res.precision, res.recall = stats, ev.precision, ev.recall
    return res


def coco_stats_from_data_dict(ids, data_dict, ground_truth, class_ids):
    """The consumer of what coco_data_dict / coco_data_dict_frames return -- the replacement for cocoGt.loadRes(data_dict) +
    COCOeval(...).evaluate() / accumulate() / summarize() (utils/cocoapi_evaluator.py:100-124) -> CocoStats.  ground_truth:
    coco_ground_truth(...) for the same ids in the same order."""
    from ..apeval import CocoEval
    index = {int(c): k for k, c in enumerate(class_ids)}
    where = {int(id_): i for i, id_ in enumerate(ids)}
    per = [([], [], []) for _ in ids]
    for d in data_dict:
        b, s, c = per[where[int(d["image_id"])]]
        x, y, w, h = d["bbox"]
        x2, y2 = np.float32(x + w), np.float32(y + h)
        # CocoEval takes the float32 corners the data_dict was made from ([x1, y1, x2 - x1, y2 - y1] on Python floats)
        if np.float32(x) != x or np.float32(y) != y or float(x2) - x != w or float(y2) - y != h:
            raise ValueError("data_dict bbox %r was not built from float32 corners" % (d["bbox"],))
        b.append([x, y, x2, y2])
        s.append(d["score"])
        c.append(index[int(d["category_id"])])
    ev = CocoEval(len(class_ids), ground_truth, image_ids=list(ids), max_dets=max(1, len(data_dict)))
    try:
        for i0, i1 in _batches(len(per), 1024):
            ev.add_detections(i0, [(np.asarray(b, np.float32).reshape(-1, 4), np.asarray(s, np.float32), np.asarray(c, np.int32))
                                   for b, s, c in per[i0:i1]])
        return _coco_result(ev)
    finally:
        ev.close()


def coco_map(net, dataset, ground_truth, batch_size=64, quantization=False, num_images=None, max_dets=None):
    """The whole COCOAPIEvaluator.evaluate (utils/cocoapi_evaluator.py:53-126) from the raw images -> CocoStats, i.e.
    (stats[0], stats[1]) with all twelve in .stats.  A calibrated q_bf model (the rule of _submit) is device-resident end to end:
    Pipeline.submit -> scale_boxes -> CocoEval.add on the ticket's stream -> release, as voc_map; every other model goes through
    forward_frame_list(..., sizes_wh="own") and CocoEval.add_detections.  dataset.pull_image(i) -> (img uint8 HWC BGR of any size,
    id); dataset.class_ids: class index -> COCO id; ground_truth: coco_ground_truth(...) for the same images in the same order."""
    from ..apeval import CocoEval
    n = len(dataset) if num_images is None else int(num_images)
    dev = net.device if isinstance(getattr(net, "device", None), (str, torch.device)) else "cuda:0"
    ev = CocoEval(len(dataset.class_ids), ground_truth[:n], max_dets=max_dets, device=dev)
    ids = []                # learnt from the loop, as the reference's; the order of the ids matters to compute() alone
    try:
        out = []            # as voc_map: the overflow flag of a ticket is read one batch late, its token kept alive until then

        def settle():
            for pipe, t, _ in out:
                if pipe.overflow(t):
                    raise_overflow(pipe.max_candidates)
            del out[:]
        for i0, i1 in _batches(n, batch_size):
            frames = []
            for i in range(i0, i1):
                img, id_ = dataset.pull_image(i)
                frames.append(img)
                ids.append(int(id_))
            if _pipeline_admits(net, i1 - i0, quantization=quantization) and hasattr(net, "submit_frame_list"):
                token = net.submit_frame_list(frames, quantization=True, find=False, sizes_wh="own")
                pipe, tickets, wh = token
                settle()
                for k, t in enumerate(tickets):
                    first = i0 + k * pipe.max_batch
                    st = pipe.stream(t)
                    ev.add(first, *pipe.outputs(t), after_stream=st, batch=min(i1 - first, pipe.max_batch))
                    with torch.cuda.stream(st):
                        pipe.release(t)
                    if wh is not None:
                        wh.record_stream(st)
                    out.append((pipe, t, token))
            else:
                settle()
                ev.add_detections(i0, net.forward_frame_list(frames, sizes_wh="own", quantization=quantization))
        settle()
        ev.set_image_ids(ids)
        return _coco_result(ev)
    finally:
        ev.close()
