"""Drop-in name for the reference's `from utils.augmentations import SSDAugmentation`: one sample through yolo355.augment (the
draws on the host from numpy.random's global stream, the pixels on the GPU).  Nothing else of that module is restated."""
import numpy as np

from .. import augment


class SSDAugmentation(object):
    def __init__(self, size=[416, 416], mean=augment.MEAN, std=augment.STD):
        self.mean = mean
        self.size = size
        self.std = std

    def __call__(self, img, boxes, labels):
        """img uint8 [h,w,3] BGR, boxes [n,4] in [0,1], labels [n] -> (float32 [H,W,3] BGR numpy image, boxes, labels); unlike
        the reference, the caller's boxes are left as they are"""
        p, boxes_out, labels_out = augment.draw(img.shape[0], img.shape[1], boxes, labels, mean=self.mean)
        x = augment.apply([img], [p], self.size, mean=self.mean, std=self.std, to_rgb=False)
        return np.ascontiguousarray(x[0].permute(1, 2, 0).cpu().numpy()), boxes_out, labels_out
