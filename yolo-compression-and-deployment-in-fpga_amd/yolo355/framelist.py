"""Lists of camera frames, each uint8 [h,w,3] BGR of its own size (numpy, CPU torch and CUDA torch frames may be mixed): the
checks, the host packing and the y355_frame descriptors that netengine.Net, engine.Engine and engine.Pipeline share
(y355_net_forward_frames / y355_forward_frames / y355_pipeline_submit_frames; include/yolo355.h)."""
import numpy as np
import torch

from . import _ffi


def _is_cuda(f):
    return isinstance(f, torch.Tensor) and f.is_cuda


def check_frame_list(frames):
    """A non-empty list or tuple of uint8 [h,w,3] frames (numpy or torch, h, w >= 1), checked before any device work;
    returns the (h, w) of every frame."""
    if not isinstance(frames, (list, tuple)):
        raise ValueError("frames must be a list or tuple of uint8 [h,w,3] frames, got %s" % type(frames).__name__)
    if len(frames) == 0:
        raise ValueError("empty frame list")
    sizes = []
    for i, f in enumerate(frames):
        if not isinstance(f, (np.ndarray, torch.Tensor)):
            raise ValueError("frame %d must be a numpy array or a torch tensor, got %s" % (i, type(f).__name__))
        if not (f.dtype == np.uint8 if isinstance(f, np.ndarray) else f.dtype == torch.uint8):
            raise ValueError("frame %d must be uint8, got %s" % (i, f.dtype))
        if len(f.shape) != 3 or f.shape[2] != 3:
            raise ValueError("frame %d must be [h,w,3] (HWC BGR), got %s" % (i, tuple(f.shape)))
        if f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("frame %d is empty: %s" % (i, tuple(f.shape)))
        sizes.append((int(f.shape[0]), int(f.shape[1])))
    return sizes


def pack_frames(frames, out=None):
    """Host-only: the host frames of a checked list (numpy, CPU torch) back to back in one uint8 buffer, no padding
    between them -- a frame starts wherever the one before ends, at any byte.  Returns (buffer, offsets, sizes):
    offsets[i] is frame i's first byte in the buffer (None for a CUDA frame, which is not packed), sizes[i] its (h, w).
    out: a uint8 buffer of at least the packed size to fill instead of a new one (the pinned staging buffer)."""
    sizes = check_frame_list(frames)
    offsets, total = [], 0
    for f, (hh, ww) in zip(frames, sizes):
        if _is_cuda(f):
            offsets.append(None)
            continue
        offsets.append(total)
        total += hh * ww * 3
    buf = np.empty(total, np.uint8) if out is None else out
    for f, o, (hh, ww) in zip(frames, offsets, sizes):
        if o is not None:
            buf[o:o + hh * ww * 3].reshape(hh, ww, 3)[...] = f if isinstance(f, np.ndarray) else f.numpy()
    return buf, offsets, sizes


def frame_list(frames, max_batch, device, stream):
    """(y355_frame array, B, sizes, held) of a list for a handle that launches on `stream` (a torch stream): host frames
    through one pinned buffer and one asynchronous copy on that stream, CUDA frames in place (a row-pitched view passes
    its pitch).  held: every tensor the launch reads -- the caller keeps them until the launch cannot be running any more;
    each is marked with record_stream, so that dropping it does not hand its memory out under the launch."""
    sizes = check_frame_list(frames)
    B = len(frames)
    if B > max_batch:
        raise ValueError("%d frames > max_batch %d" % (B, max_batch))
    held, base = [], 0
    nbytes = sum(hh * ww * 3 for f, (hh, ww) in zip(frames, sizes) if not _is_cuda(f))
    if nbytes:
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        _, offsets, _ = pack_frames(frames, out=pinned.numpy())
        with torch.cuda.device(device), torch.cuda.stream(stream):     # allocated on `stream`: its allocator pool, no mark needed
            dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
            dev.copy_(pinned, non_blocking=True)
        held += [pinned, dev]
        base = dev.data_ptr()
    else:
        offsets = [None] * B
    arr = (_ffi.Frame * B)()
    for i, (f, o, (hh, ww)) in enumerate(zip(frames, offsets, sizes)):
        arr[i].height, arr[i].width, arr[i].row_bytes = hh, ww, 0
        if o is not None:
            arr[i].data_dev = base + o
            continue
        if f.device != device:
            f = f.to(device)
        if f.stride(2) == 1 and f.stride(1) == 3 and f.stride(0) >= 3 * ww:
            arr[i].row_bytes = int(f.stride(0))
        else:
            f = f.contiguous()
        f.record_stream(stream)
        held.append(f)
        arr[i].data_dev = f.data_ptr()
    return arr, B, sizes, held


def own_sizes_wh(sizes):
    """the (width, height) rows of sizes_wh="own": every image rescaled by its own source size"""
    return np.asarray([(ww, hh) for hh, ww in sizes], np.float32)


def check_sizes_wh(sizes_wh):
    if isinstance(sizes_wh, str) and sizes_wh != "own":
        raise ValueError('sizes_wh: an array [n,2] or "own", got %r' % (sizes_wh,))


def wh_tensor(sizes_wh, n, device, what="batch"):
    """the (width, height) rows of sizes_wh as a float32 device tensor [n,2]; n None: as many as there are"""
    wh = torch.as_tensor(np.asarray(sizes_wh, np.float32).reshape(-1, 2)).to(device)
    if n is not None and wh.shape[0] != n:
        raise ValueError("sizes_wh has %d rows for a %s of %d" % (wh.shape[0], what, n))
    return wh


def sizes_wh_tensor(sizes_wh, sizes, device):
    """sizes_wh (None, an array [n,2] or "own") of a checked list with these (h, w) as a float32 device tensor [n,2], or None"""
    check_sizes_wh(sizes_wh)
    if sizes_wh is None:
        return None
    return wh_tensor(own_sizes_wh(sizes) if isinstance(sizes_wh, str) else sizes_wh, len(sizes), device, "list")
