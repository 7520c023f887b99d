"""Evaluator helpers on raw images (voc_all_boxes_frames / coco_data_dict_frames): dataset.pull_image(i) hands out uint8 HWC
BGR images of any size, the resize and the normalisation run on the GPU, every image's boxes are rescaled by its own (w, h).
They must build what voc_all_boxes / coco_data_dict build from the host-transformed images (the oracle resize as the
transform)."""
import numpy as np
import pytest

from test_net_frames import SIZE, _model

SIZES_HW = [(375, 500), (480, 640), (375, 500), (333, 500), (224, 320), (480, 640), (97, 131)]     # 7 images, 5 distinct sizes


class _RawSet:
    """pull_image(i) -> (img uint8 HWC BGR, id) like data/voc0712.py:148-160 and data/cocodataset.py:70-81"""
    class_ids = [11, 22, 33]

    def __init__(self):
        from yolo355 import synth
        self.imgs = [synth.make_frames_u8(300 + i, 1, h, w, "blocks")[0] for i, (h, w) in enumerate(SIZES_HW)]

    def __len__(self):
        return len(self.imgs)

    def pull_image(self, i):
        return self.imgs[i], 1000 + 3 * i


def _transformed(img):
    """BaseTransform of one image (data/__init__.py:30-56) with the oracle resize: float32 CHW RGB at the network size"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    return synth.normalize_frames(resize_linear_u8(img, SIZE[0], SIZE[1])[None])[0]


class _VocSet:
    """pull_item(i) -> (im tensor [3,H,W], gt, h, w): the transformed items of the same images"""

    def __init__(self, raw):
        self.raw = raw

    def __len__(self):
        return len(self.raw)

    def pull_item(self, i):
        import torch
        img = self.raw.imgs[i]
        return torch.from_numpy(_transformed(img)), None, img.shape[0], img.shape[1]


def test_frame_helpers_need_a_model_with_forward_frame_list():
    from yolo355.utils.evaluator_batch import coco_data_dict_frames, voc_all_boxes_frames

    class Other:
        def forward_batch(self, x):
            return []
    with pytest.raises(TypeError, match="forward_frame_list"):
        voc_all_boxes_frames(Other(), _RawSet(), 3, batch_size=3)
    with pytest.raises(TypeError, match="forward_frame_list"):
        coco_data_dict_frames(Other(), _RawSet(), batch_size=3)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2"])
def test_frame_evaluators_equal_the_host_transform_evaluators(arch):
    import torch
    from yolo355 import synth
    from yolo355.utils.evaluator_batch import coco_data_dict, coco_data_dict_frames, voc_all_boxes, voc_all_boxes_frames
    m = _model(arch, "cuda:0")
    m.forward_batch(torch.from_numpy(synth.make_images(21, 1, SIZE[0], SIZE[1], "blocks")), quantization=True)      # freezes the exponents
    raw = _RawSet()
    assert len(raw) == 7 and len(set(SIZES_HW)) == 5

    def transform(img):                                    # HWC BGR float at the network size, as BaseTransform returns it
        return [np.ascontiguousarray(_transformed(img).transpose(1, 2, 0)[:, :, ::-1])]
    ids, dd = coco_data_dict_frames(m, raw, batch_size=3)
    wids, wdd = coco_data_dict(m, raw, transform, batch_size=3)
    assert ids == wids == [1000 + 3 * i for i in range(7)]
    assert len(dd) > 0 and dd == wdd
    for q in (False, True):
        got = voc_all_boxes_frames(m, raw, 3, batch_size=3, quantization=q)
        want = voc_all_boxes(m, _VocSet(raw), 3, batch_size=3, quantization=q)
        n = 0
        for j in range(3):
            for i in range(7):
                assert got[j][i].dtype == np.float32 and np.array_equal(got[j][i], want[j][i]), (q, j, i)
                n += len(got[j][i])
        assert n > 0
    part = voc_all_boxes_frames(m, raw, 3, batch_size=2, num_images=4)          # other batch boundaries, a prefix of the set
    want = voc_all_boxes_frames(m, raw, 3, batch_size=3)
    assert all(len(part[j]) == 4 for j in range(3))
    assert all(np.array_equal(part[j][i], want[j][i]) for j in range(3) for i in range(4))
