"""The image pipeline of the mono3d branch (``configs/gga/gga_pdg.py`` of the reference, :67-105) and the hand-over of an image
batch to the device.

Transforms (mmdet 2.x semantics; mmdet's source is not part of the reference tree, the behaviour is restated here):
``LoadImageFromFileMono3D`` (mmdet3d/datasets/pipelines/loading.py:76-96), ``Resize`` (``keep_ratio=True`` with one
``img_scale``), ``Normalize``, ``Pad`` (``size_divisor``), ``MultiScaleFlipAug`` (one scale factor; ``flip=True`` adds the mirrored view). ``RandomFlip3D``
(gga_amd/pipelines.py) calls ``flip_image`` / ``flip_bboxes`` below when a sample carries an image.

Two ways to the pixels, the same bits:

* eager (``GGA_MONO_IMAGE_DEVICE=0``): every transform works on ``results['img']`` as an array, the sample leaves the worker
  as a normalised, padded float32 image;
* deferred (the default): ``LoadImageFromFileMono3D`` wraps the decoded uint8 image in a ``DeferredImage`` and the four pixel
  transforms only record their decision in it (every other key - ``img_shape``, ``scale_factor``, ``flip``, ``pad_shape``, the
  boxes - is updated exactly as in the eager path). ``loader.pack_collated`` puts the sources of a batch into one uint8
  buffer (``PackedImages``) and ``image_batch`` turns it into the ``[B, 3, Hp, Wp]`` float32 tensor: on a device with one
  upload and one launch of ``gga_image_batch``; without one (``device=None``, the CPU tests) with ``materialize``, the host
  arithmetic of the eager path.

Pixel arithmetic of ``Resize`` is this project's own definition (cv2 is not available to compare with): fixed-point bilinear
with half-pixel centres, integers only, so that host and device agree bit for bit - ``resize_taps`` / ``resize_bilinear``.
``Normalize`` of a uint8 image is a [3, 256] float32 table (``normalize_table``).
"""
import copy
import os

import numpy as np
import torch

from .pipelines import Compose, DataContainer
from .registry import PIPELINES

WEIGHT_BITS = 11                  # tap weights are multiples of 1 / 2048


def device_enabled():
    """``GGA_MONO_IMAGE_DEVICE=0`` makes the loader workers do the pixel work (the eager host path)."""
    return os.environ.get('GGA_MONO_IMAGE_DEVICE', '1') != '0'


# ----------------------------------------------------------------------------- the arithmetic (host side of gga_image_batch)
def resize_taps(dst, src):
    """Taps of the ``dst`` output positions along an axis of ``src`` samples -> (i0, i1, w1) int64 arrays: the output is
    ``((2048 - w1) * p[i0] + w1 * p[i1])``. q = round(fx * 2048) for fx = (x + 0.5) * src / dst - 0.5, in integers."""
    x = np.arange(dst, dtype=np.int64)
    q = ((2 * x + 1) * src * 2048 + dst) // (2 * dst) - 1024
    i0, w1 = q >> WEIGHT_BITS, q & 2047
    low = i0 < 0
    i0[low], w1[low] = 0, 0
    high = i0 >= src - 1
    i0[high] = src - 1
    i1 = np.where(high, src - 1, i0 + 1)
    return i0, i1, w1


def resize_bilinear(img, dst_h, dst_w):
    """uint8 [H, W, C] -> uint8 [dst_h, dst_w, C]: pixel = (sum wy wx p + 2^21) >> 22 (at most 255 * 2^22 + 2^21 < 2^31).
    ``dst == src`` is the identity. Expected to sit within one grey level of cv2's INTER_LINEAR (not measured)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    y0, y1, wy = resize_taps(dst_h, img.shape[0])
    x0, x1, wx = resize_taps(dst_w, img.shape[1])
    p = img.astype(np.int64)
    wx0, wx1 = (2048 - wx)[None, :, None], wx[None, :, None]
    top = wx0 * p[y0][:, x0] + wx1 * p[y0][:, x1]
    bot = wx0 * p[y1][:, x0] + wx1 * p[y1][:, x1]
    out = ((2048 - wy)[:, None, None] * top + wy[:, None, None] * bot + (1 << 21)) >> 22
    return out.astype(np.uint8)


def normalize_table(mean, std):
    """[3, 256] float32: table[c][v] = (float32(v) - float32(mean_c)) * float32(1 / float64(std_c)), the whole function of a
    uint8 input. Whether cv2 (which mmcv's imnormalize calls) rounds the same way cannot be pinned without it; if it ever
    matters, this line is the one to change - host and device both read the table."""
    mean, std = np.asarray(mean, np.float64).reshape(3), np.asarray(std, np.float64).reshape(3)
    v = np.arange(256, dtype=np.float32)[None, :]
    return ((v - mean.astype(np.float32)[:, None]) * (1.0 / std).astype(np.float32)[:, None]).astype(np.float32)


class DeferredImage:
    """A decoded uint8 image [H, W, 3] and what the pixel transforms decided about it: the size after ``Resize``, the
    horizontal flip, the table and channel reversal of ``Normalize``, the size after ``Pad``."""

    def __init__(self, src):
        src = np.ascontiguousarray(src)
        assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3, (src.dtype, src.shape)
        self.src = src
        self.dst_h, self.dst_w = int(src.shape[0]), int(src.shape[1])
        self.flip, self.table, self.reverse = False, None, False
        self.pad_h = self.pad_w = None

    def copy(self):
        """A second record of decisions about the SAME pixels (``src`` is shared, not copied): the other view of a sample under
        ``MultiScaleFlipAug(flip=True)``, which ``flip_image`` may toggle without touching this one."""
        other = DeferredImage(self.src)
        other.dst_h, other.dst_w, other.flip, other.table, other.reverse = self.dst_h, self.dst_w, self.flip, self.table, self.reverse
        other.pad_h, other.pad_w = self.pad_h, self.pad_w
        return other

    @property
    def shape(self):
        """The shape the eager image would have now."""
        return (self.pad_h or self.dst_h, self.pad_w or self.dst_w, 3)

    def materialize(self, out_h=None, out_w=None):
        """The eager pipeline's result, float32 [3, out_h, out_w] (default: the padded size), zero outside dst_h x dst_w."""
        assert self.table is not None, 'Normalize must be part of a deferred image pipeline'
        img = resize_bilinear(self.src, self.dst_h, self.dst_w)
        if self.flip:
            img = img[:, ::-1]
        if self.reverse:
            img = img[..., ::-1]
        out_h, out_w = out_h or self.pad_h or self.dst_h, out_w or self.pad_w or self.dst_w
        out = np.zeros((3, out_h, out_w), np.float32)
        for c in range(3):
            out[c, :self.dst_h, :self.dst_w] = self.table[c][img[..., c]]
        return out


class PackedImages:
    """The deferred images of one chunk as ONE uint8 tensor - the table first, every source at a 16-byte aligned offset -
    plus the small per-image records. Picklable: what crosses the process boundary for a batch of images. Images that share
    their ``src`` array (the views of a frame under ``MultiScaleFlipAug(flip=True)``) share its bytes in the buffer: every
    source is held once. ``n_views``: the images are ``n_views`` views of ``len / n_views`` frames, view-major (all frames
    of view 0 first) - the order of the output rows of ``image_batch``."""

    TABLE_BYTES = 3 * 256 * 4

    def __init__(self, images, n_views=1):
        assert images and all(isinstance(i, DeferredImage) for i in images)
        assert n_views >= 1 and len(images) % n_views == 0, (len(images), n_views)
        first = images[0]
        assert first.table is not None, 'Normalize must be part of a deferred image pipeline'
        for i in images:
            assert i.reverse == first.reverse and np.array_equal(i.table, first.table), 'one img_norm_cfg per batch'
        self.reverse, self.n_views = bool(first.reverse), int(n_views)
        self.records, at, placed, sources = [], self.TABLE_BYTES, {}, []
        for i in images:
            if id(i.src) not in placed:
                placed[id(i.src)] = at
                sources.append((at, i.src))
                at += -(-i.src.size // 16) * 16
            self.records.append((placed[id(i.src)], i.src.shape[0], i.src.shape[1], i.dst_h, i.dst_w, int(i.flip), i.pad_h or i.dst_h,
                                 i.pad_w or i.dst_w))
        self.buffer = torch.zeros(at, dtype=torch.uint8)
        buf = self.buffer.numpy()
        buf[:self.TABLE_BYTES] = np.ascontiguousarray(first.table, np.float32).reshape(-1).view(np.uint8)
        for o, src in sources:
            buf[o:o + src.size] = src.reshape(-1)

    def __len__(self):
        return len(self.records)

    def images(self):
        """The ``DeferredImage`` objects again (views into the buffer)."""
        buf = self.buffer.numpy()
        table = buf[:self.TABLE_BYTES].view(np.float32).reshape(3, 256)
        out = []
        for at, sh, sw, dh, dw, flip, ph, pw in self.records:
            d = DeferredImage(buf[at:at + sh * sw * 3].reshape(sh, sw, 3))
            d.dst_h, d.dst_w, d.flip, d.table, d.reverse, d.pad_h, d.pad_w = dh, dw, bool(flip), table, self.reverse, ph, pw
            out.append(d)
        return out


class PackedView:
    """Stands where view ``index`` > 0 of a chunk was in a collated test-time batch: its images travel in view 0's
    ``PackedImages`` (``n_views`` > 1)."""

    def __init__(self, index):
        self.index = int(index)


def image_batch(images, device=None, channels_last=False):
    """``PackedImages`` or a list of ``DeferredImage`` -> float32 [B, 3, Hp, Wp], Hp / Wp the largest padded sizes of the
    batch; ``channels_last``: in channels-last memory. ``device=None``: the host arithmetic; a device: one upload of the
    byte buffer and one launch of ``gga_image_batch``."""
    packed = images if isinstance(images, PackedImages) else PackedImages(list(images))      # (``n_views`` views: [V * B, ...], view-major)
    hp, wp = max(r[6] for r in packed.records), max(r[7] for r in packed.records)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    if device is None:
        out = torch.from_numpy(np.stack([d.materialize(hp, wp) for d in packed.images()]))
        return out.contiguous(memory_format=fmt)
    import ctypes as C
    from . import _lib
    from . import functional as F
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('gga_amd ops run on the GPU only; there is no CPU fallback in the product path')
    n = len(packed)
    descs = (_lib.ImageDesc * n)()
    for k, (at, sh, sw, dh, dw, flip, _, _) in enumerate(packed.records):
        descs[k].src_offset, descs[k].src_h, descs[k].src_w, descs[k].dst_h, descs[k].dst_w, descs[k].flip = at, sh, sw, dh, dw, flip
    with torch.cuda.device(dev):
        src = packed.buffer.to(dev, non_blocking=True)
        out = torch.empty((n, 3, hp, wp), dtype=torch.float32, device=dev, memory_format=fmt)
        _lib.check(_lib.lib().gga_image_batch(src.data_ptr(), src.numel(), descs, n, src.data_ptr(), int(packed.reverse), hp, wp,
                                              F.LAYOUT_NHWC if channels_last else F.LAYOUT_NCHW, out.data_ptr(), F._stream()),
                   'gga_image_batch')
        src.record_stream(torch.cuda.current_stream(dev))
    return out


# ----------------------------------------------------------------------------- what RandomFlip3D does to an image sample
def flip_image(d):
    """Mirrors every image field of the sample (a deferred image records it)."""
    for key in d.get('img_fields', ['img']):
        if isinstance(d[key], DeferredImage):
            d[key].flip = not d[key].flip
        else:
            d[key] = np.ascontiguousarray(d[key][:, ::-1])


def flip_bboxes(d):
    """mmdet ``RandomFlip.bbox_flip`` (horizontal) for every ``bbox_fields`` array: x1' = w - x2, x2' = w - x1, w from
    ``img_shape``."""
    w = d['img_shape'][1]
    for key in d.get('bbox_fields', []):
        boxes = d[key]
        flipped = boxes.copy()
        flipped[..., 0::4] = w - boxes[..., 2::4]
        flipped[..., 2::4] = w - boxes[..., 0::4]
        d[key] = flipped


# ----------------------------------------------------------------------------- transforms
@PIPELINES.register_module()
class LoadImageFromFileMono3D:
    """loading.py:76-96 over mmdet's ``LoadImageFromFile``: the file ``join(img_prefix, img_info['filename'])`` decoded with
    PIL into uint8 [H, W, 3] in BGR order (mmcv's ``imread`` default; PIL gives RGB), plus ``cam2img``. ``defer``: hand the
    pixels on as a ``DeferredImage`` (default: what ``GGA_MONO_IMAGE_DEVICE`` says)."""

    def __init__(self, to_float32=False, color_type='color', file_client_args=dict(backend='disk'), defer=None):
        if to_float32 or color_type != 'color':
            raise NotImplementedError('LoadImageFromFileMono3D: uint8 colour images only')
        self.defer = defer

    def __call__(self, results):
        from PIL import Image
        info = results['img_info']
        filename = os.path.join(results['img_prefix'], info['filename']) if results.get('img_prefix') is not None else info['filename']
        with Image.open(filename) as im:
            img = np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8)[..., ::-1])
        defer = device_enabled() if self.defer is None else self.defer
        results['filename'], results['ori_filename'] = filename, info['filename']
        results['img'] = DeferredImage(img) if defer else img
        results['img_shape'] = results['ori_shape'] = img.shape
        results['img_fields'] = ['img']
        results['cam2img'] = copy.deepcopy(info['cam_intrinsic'])        # (RandomFlip3D writes into it: not the dataset's own record)
        return results


@PIPELINES.register_module()
class Resize:
    """mmdet 2.x ``Resize`` for ``img_scale=(long, short), keep_ratio=True``: one scale s = min(long / max(h, w), short /
    min(h, w)), new size (int(w s + 0.5), int(h s + 0.5)); ``bbox_fields`` are scaled and clipped to the new image;
    ``centers2d``, ``cam2img`` and the 3D boxes stay as they are (mmdet's transform knows nothing of them and the reference
    adds nothing). Inside ``MultiScaleFlipAug`` the sample's own ``scale_factor`` takes the place of ``img_scale``."""

    def __init__(self, img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True, bbox_clip_border=True,
                 backend='cv2', override=False):
        if isinstance(img_scale, list):
            if len(img_scale) != 1:
                raise NotImplementedError('Resize: one img_scale')
            img_scale = img_scale[0]
        if ratio_range is not None or not keep_ratio or not bbox_clip_border or override:
            raise NotImplementedError('Resize: only img_scale=(w, h), keep_ratio=True, bbox_clip_border=True')
        self.img_scale = tuple(img_scale) if img_scale is not None else None

    def __call__(self, results):
        h, w = results['img'].shape[:2]
        if 'scale' in results:
            scale = results['scale']
        elif 'scale_factor' in results:                  # MultiScaleFlipAug(scale_factor=...): the scaled size as (w, h)
            assert isinstance(results['scale_factor'], float)
            scale = results['scale'] = (int(w * results['scale_factor']), int(h * results['scale_factor']))
        else:
            assert self.img_scale is not None
            scale = results['scale'] = self.img_scale
        s = min(max(scale) / max(h, w), min(scale) / min(h, w))
        new_w, new_h = int(w * float(s) + 0.5), int(h * float(s) + 0.5)
        for key in results.get('img_fields', ['img']):
            img = results[key]
            if isinstance(img, DeferredImage):
                assert img.pad_h is None and not img.flip and img.table is None, 'Resize comes first among the pixel transforms'
                img.dst_h, img.dst_w = new_h, new_w
            else:
                results[key] = resize_bilinear(img, new_h, new_w)
        w_scale, h_scale = new_w / w, new_h / h
        results['scale_factor'] = np.array([w_scale, h_scale, w_scale, h_scale], dtype=np.float32)
        results['img_shape'] = results['pad_shape'] = (new_h, new_w, 3)
        results['keep_ratio'] = True
        for key in results.get('bbox_fields', []):
            boxes = results[key] * results['scale_factor']
            boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, new_w)
            boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, new_h)
            results[key] = boxes
        return results


@PIPELINES.register_module()
class Normalize:
    """mmdet ``Normalize``: the optional BGR -> RGB reversal, then (v - mean) / std per channel, as a table lookup."""

    def __init__(self, mean, std, to_rgb=True):
        self.mean, self.std, self.to_rgb = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32), to_rgb
        self.table = normalize_table(mean, std)

    def __call__(self, results):
        for key in results.get('img_fields', ['img']):
            img = results[key]
            if isinstance(img, DeferredImage):
                assert img.pad_h is None, 'Normalize comes before Pad'
                img.table, img.reverse = self.table, bool(self.to_rgb)
            else:
                assert img.dtype == np.uint8
                if self.to_rgb:
                    img = img[..., ::-1]
                results[key] = np.stack([self.table[c][img[..., c]] for c in range(3)], -1)
        results['img_norm_cfg'] = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)
        return results


@PIPELINES.register_module()
class Pad:
    """mmdet ``Pad`` with ``size_divisor``: zeros at the bottom and right up to the next multiple."""

    def __init__(self, size=None, size_divisor=None, pad_val=0):
        if size is not None or size_divisor is None or pad_val != 0:
            raise NotImplementedError('Pad: only size_divisor with zeros')
        self.size_divisor = int(size_divisor)

    def __call__(self, results):
        shape = None
        for key in results.get('img_fields', ['img']):
            img = results[key]
            h, w = img.shape[:2]
            ph, pw = -(-h // self.size_divisor) * self.size_divisor, -(-w // self.size_divisor) * self.size_divisor
            if isinstance(img, DeferredImage):
                img.pad_h, img.pad_w = ph, pw
            else:
                out = np.zeros((ph, pw) + img.shape[2:], img.dtype)
                out[:h, :w] = img
                results[key] = out
            shape = (ph, pw, 3)
        results['pad_shape'], results['pad_fixed_size'], results['pad_size_divisor'] = shape, None, self.size_divisor
        return results


@PIPELINES.register_module()
class MultiScaleFlipAug:
    """mmdet ``MultiScaleFlipAug`` for one ``scale_factor``: a pass with ``flip=False`` and, with ``flip=True``, a second
    one with the horizontal flip written into the sample (``RandomFlip3D`` among the transforms then mirrors the image and
    sets ``pcd_horizontal_flip``); every output key is a list with one entry per view. The second view works on a
    ``DeferredImage`` record and on lists of its own; the source pixels are shared. Several scales cannot be merged by the
    detector (maps of different sizes) and are refused, as are ``img_scale`` and the vertical flip."""

    def __init__(self, transforms, img_scale=None, scale_factor=None, flip=False, flip_direction='horizontal'):
        if img_scale is not None or isinstance(scale_factor, (list, tuple)) or scale_factor is None:
            raise NotImplementedError('MultiScaleFlipAug: one scale_factor')
        if flip and flip_direction not in ('horizontal', ['horizontal'], ('horizontal', )):
            raise NotImplementedError(f'MultiScaleFlipAug: flip_direction {flip_direction!r} (the horizontal flip is built)')
        if flip and not any((t.get('type') if isinstance(t, dict) else type(t).__name__) == 'RandomFlip3D' for t in transforms):
            # this transform only writes the flag; without the one that reads it the second view would be the first again
            raise NotImplementedError('MultiScaleFlipAug: flip=True needs a RandomFlip3D among the transforms to mirror the second view')
        self.transforms, self.scale_factor, self.flip = Compose(transforms), float(scale_factor), bool(flip)

    def __call__(self, results):
        one = dict(results)
        one['scale_factor'], one['flip'], one['flip_direction'] = self.scale_factor, False, 'horizontal'
        if not self.flip:
            return {key: [value] for key, value in self.transforms(one).items()}
        two = {key: value.copy() if isinstance(value, (DeferredImage, list)) else value for key, value in results.items()}
        two['scale_factor'], two['flip'], two['flip_direction'] = self.scale_factor, True, 'horizontal'
        views = [self.transforms(one), self.transforms(two)]
        return {key: [view[key] for view in views] for key in views[0]}


def format_image(results):
    """``DefaultFormatBundle``'s part for ``img``: an array goes to a C x H x W tensor container that the collate stacks; a
    deferred image travels as it is and becomes part of the batch's ``PackedImages``."""
    img = results['img']
    if isinstance(img, DeferredImage):
        results['img'] = DataContainer(img, stack=False, cpu_only=True)
    else:
        results['img'] = DataContainer(torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))), stack=True)
    return results
