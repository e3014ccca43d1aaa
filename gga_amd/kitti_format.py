"""KITTI result formatting on the device: ``convert_valid_bboxes`` + ``bbox2result_kitti``
(mmdet3d/datasets/kitti_dataset_GGA_train.py:453-566,680-761) for the detections of a whole test run at once.

``format_kitti_dets(net_outputs, data_infos, class_names, pcd_limit_range, device)`` -> the list of KITTI annotation dicts the
host loop of ``KittiDataset_GGA_train.bbox2result_kitti`` builds (same keys, dtypes, shapes and empty-frame placeholders):
one concatenation of the frames' detections, one upload, one launch of ``gga_kitti_format_dets`` (validity tests, compaction
per frame, the label columns), one download. Like the host loop it limits the yaw of the caller's boxes in place."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import functional as F
from ._lib import check

COLS = 20          # GGA_KITTI_FORMAT_COLS: bbox 4, dimensions 3, location 3, rotation_y, alpha, score, LiDAR box 7


def enabled():
    """The environment switch ``GGA_KITTI_FORMAT=0`` sends every caller back to the host loop (A/B runs)."""
    return os.environ.get('GGA_KITTI_FORMAT', '1') != '0'


def _section(sizes):
    """Byte offsets of consecutive 8-byte aligned sections -> (offsets, total)."""
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += (int(s) + 7) // 8 * 8
    return offs, at


def format_columns(boxes, scores, labels, frame_offsets, lidar2cam, p2, image_hw, pcd_limit_range, device):
    """The raw call: host arrays in, host arrays out. boxes [N,7] f32, scores [N] f32, labels [N] i64, frame_offsets [F+1]
    i64, lidar2cam / p2 [F,4,4] f32, image_hw [F,2] i32 -> (columns [N, COLS] f32 and labels [N] i64 whose rows
    frame_offsets[f] .. frame_offsets[f] + counts[f] hold frame f's valid detections in their original order, the limited
    yaw of every detection [N] f32, counts [F] i32)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('gga_amd ops run on the GPU only; there is no CPU fallback in the product path')
    n, f = int(boxes.shape[0]), int(len(frame_offsets) - 1)
    ins = [np.ascontiguousarray(boxes, np.float32).reshape(n, 7), np.ascontiguousarray(scores, np.float32).reshape(n),
           np.ascontiguousarray(labels, np.int64).reshape(n), np.ascontiguousarray(frame_offsets, np.int64).reshape(f + 1),
           np.ascontiguousarray(lidar2cam, np.float32).reshape(f, 16), np.ascontiguousarray(p2, np.float32).reshape(f, 16),
           np.ascontiguousarray(image_hw, np.int32).reshape(f, 2)]
    in_off, in_bytes = _section([a.nbytes for a in ins])
    out_sizes = [n * COLS * 4, n * 8, n * 4, f * 4]
    out_off, out_bytes = _section(out_sizes)
    host = np.zeros(max(in_bytes, 8), np.uint8)
    for a, o in zip(ins, in_off):
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    rng = (C.c_float * 6)(*[float(v) for v in pcd_limit_range])
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(host).to(dev)
        d_out = torch.zeros(max(out_bytes, 8), dtype=torch.uint8, device=dev)
        pi = [C.c_void_p(d_in.data_ptr() + o) for o in in_off]
        po = [C.c_void_p(d_out.data_ptr() + o) for o in out_off]
        check(_lib.lib().gga_kitti_format_dets(pi[0], pi[1], pi[2], n, pi[3], f, pi[4], pi[5], pi[6], C.byref(rng), po[0], po[1],
                                               po[2], po[3], F._stream()), 'gga_kitti_format_dets')
        back = d_out.cpu().numpy()
    cut = lambda k, dt: back[out_off[k]:out_off[k] + out_sizes[k]].view(dt)
    return cut(0, np.float32).reshape(n, COLS), cut(1, np.int64), cut(2, np.float32), cut(3, np.int32)


def _empty_anno():
    return dict(name=np.array([]), truncated=np.array([]), occluded=np.array([]), alpha=np.array([]), bbox=np.zeros([0, 4]),
                dimensions=np.zeros([0, 3]), location=np.zeros([0, 3]), rotation_y=np.array([]), score=np.array([]),
                sample_idx=np.array([], dtype=np.int64))


def format_kitti_dets(net_outputs, data_infos, class_names, pcd_limit_range, device='cuda:0'):
    """-> list of KITTI anno dicts, one per frame (``name``, ``truncated``, ``occluded``, ``alpha``, ``bbox``, ``dimensions``,
    ``location``, ``rotation_y``, ``score``, ``sample_idx``), as ``bbox2result_kitti`` builds them on the host.
    ``net_outputs``: per frame a dict with ``boxes_3d`` (LiDAR boxes), ``scores_3d``, ``labels_3d``. The yaw of every
    ``boxes_3d`` is limited in place (``limit_yaw(offset=0.5, period=2 pi)``), as the host path does."""
    assert len(net_outputs) == len(data_infos), 'invalid list length of network outputs'
    nf = len(net_outputs)
    tensors = [o['boxes_3d'].tensor for o in net_outputs]
    counts = np.array([t.shape[0] for t in tensors], np.int64)
    offsets = np.zeros(nf + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    n = int(offsets[-1])
    if n:
        boxes = torch.cat(tensors, 0)[:, :7].to('cpu', torch.float32).numpy()
        scores = torch.cat([o['scores_3d'].reshape(-1) for o in net_outputs], 0).to('cpu', torch.float32).numpy()
        labels_in = torch.cat([o['labels_3d'].reshape(-1) for o in net_outputs], 0).to('cpu', torch.int64).numpy()
    else:
        boxes, scores, labels_in = np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    lidar2cam, p2, hw = np.zeros((nf, 4, 4), np.float32), np.zeros((nf, 4, 4), np.float32), np.zeros((nf, 2), np.int32)
    for i, info in enumerate(data_infos):
        calib = info['calib']
        lidar2cam[i] = calib['R0_rect'].astype(np.float32) @ calib['Tr_velo_to_cam'].astype(np.float32)
        proj = calib['P2'].astype(np.float32)
        p2[i] = np.eye(4, dtype=np.float32)             # points_cam2img pads a 3 x 4 matrix with the identity's last row
        p2[i, :proj.shape[0], :proj.shape[1]] = proj
        hw[i] = info['image']['image_shape'][:2]
    cols, labels, yaw, valid = format_columns(boxes, scores, labels_in, offsets, lidar2cam, p2, hw, pcd_limit_range, device)
    names = np.asarray(list(class_names))
    name_len = np.array([len(c) for c in class_names], np.int64)
    annos = []
    for i, info in enumerate(data_infos):
        b, k = int(offsets[i]), int(valid[i])
        if counts[i]:
            t = tensors[i]
            t[:, 6] = torch.from_numpy(yaw[b:b + int(counts[i])]).to(t.device)
        if k == 0:
            annos.append(_empty_anno())
            continue
        c, lab = cols[b:b + k], labels[b:b + k]
        annos.append(dict(name=names[lab].astype(f'<U{int(name_len[lab].max())}'), truncated=np.zeros(k),
                          occluded=np.zeros(k, dtype=np.int64), alpha=c[:, 11].copy(), bbox=c[:, 0:4].copy(),
                          dimensions=c[:, 4:7].copy(), location=c[:, 7:10].copy(), rotation_y=c[:, 10].copy(),
                          score=c[:, 12].copy(), sample_idx=np.array([info['image']['image_idx']] * k, dtype=np.int64)))
    return annos


# ----------------------------------------------------------------------------- camera boxes (the image branch)
CAM_COLS = 13      # GGA_KITTI_FORMAT_CAM_COLS: bbox 4, dimensions 3, location 3, rotation_y, alpha, score


def format_columns_cam(boxes, scores, labels, frame_offsets, p2, image_hw, device):
    """The raw call of the camera-box variant: boxes [N,7] f32 camera boxes, scores [N] f32, labels [N] i64, frame_offsets
    [F+1] i64, p2 [F,4,4] f32, image_hw [F,2] i32 -> (columns [N, CAM_COLS] f32, labels [N] i64, counts [F] i32), rows as in
    ``format_columns``. One upload, one launch of ``gga_kitti_format_dets_cam``, one download."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('gga_amd ops run on the GPU only; there is no CPU fallback in the product path')
    n, f = int(boxes.shape[0]), int(len(frame_offsets) - 1)
    ins = [np.ascontiguousarray(boxes, np.float32).reshape(n, 7), np.ascontiguousarray(scores, np.float32).reshape(n),
           np.ascontiguousarray(labels, np.int64).reshape(n), np.ascontiguousarray(frame_offsets, np.int64).reshape(f + 1),
           np.ascontiguousarray(p2, np.float32).reshape(f, 16), np.ascontiguousarray(image_hw, np.int32).reshape(f, 2)]
    in_off, in_bytes = _section([a.nbytes for a in ins])
    out_sizes = [n * CAM_COLS * 4, n * 8, f * 4]
    out_off, out_bytes = _section(out_sizes)
    host = np.zeros(max(in_bytes, 8), np.uint8)
    for a, o in zip(ins, in_off):
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    with torch.cuda.device(dev):
        d_in = torch.from_numpy(host).to(dev)
        d_out = torch.zeros(max(out_bytes, 8), dtype=torch.uint8, device=dev)
        pi = [C.c_void_p(d_in.data_ptr() + o) for o in in_off]
        po = [C.c_void_p(d_out.data_ptr() + o) for o in out_off]
        check(_lib.lib().gga_kitti_format_dets_cam(pi[0], pi[1], pi[2], n, pi[3], f, pi[4], pi[5], po[0], po[1], po[2], F._stream()),
              'gga_kitti_format_dets_cam')
        back = d_out.cpu().numpy()
    cut = lambda k, dt: back[out_off[k]:out_off[k] + out_sizes[k]].view(dt)
    return cut(0, np.float32).reshape(n, CAM_COLS), cut(1, np.int64), cut(2, np.int32)


def format_kitti_dets_cam(net_outputs, anno_infos, class_names, device='cuda:0'):
    """``KittiMonoDataset.bbox2result_kitti`` (mmdet3d/datasets/kitti_mono_dataset.py:271-384) for all frames at once ->
    the list of KITTI anno dicts its host loop builds (same keys, dtypes, shapes, empty-frame placeholders).
    ``net_outputs``: per frame a dict with ``boxes_3d`` (camera boxes), ``scores_3d``, ``labels_3d``."""
    assert len(net_outputs) == len(anno_infos), 'invalid list length of network outputs'
    nf = len(net_outputs)
    tensors = [o['boxes_3d'].tensor for o in net_outputs]
    counts = np.array([t.shape[0] for t in tensors], np.int64)
    offsets = np.zeros(nf + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    if int(offsets[-1]):
        boxes = torch.cat(tensors, 0)[:, :7].to('cpu', torch.float32).numpy()
        scores = torch.cat([o['scores_3d'].reshape(-1) for o in net_outputs], 0).to('cpu', torch.float32).numpy()
        labels_in = torch.cat([o['labels_3d'].reshape(-1) for o in net_outputs], 0).to('cpu', torch.int64).numpy()
    else:
        boxes, scores, labels_in = np.zeros((0, 7), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    p2, hw = np.zeros((nf, 4, 4), np.float32), np.zeros((nf, 2), np.int32)
    for i, info in enumerate(anno_infos):
        proj = info['calib']['P2'].astype(np.float32)
        p2[i] = np.eye(4, dtype=np.float32)             # points_cam2img pads a 3 x 4 matrix with the identity's last row
        p2[i, :proj.shape[0], :proj.shape[1]] = proj
        hw[i] = info['image']['image_shape'][:2]
    cols, labels, valid = format_columns_cam(boxes, scores, labels_in, offsets, p2, hw, device)
    names = np.asarray(list(class_names))
    name_len = np.array([len(c) for c in class_names], np.int64)
    annos = []
    for i, info in enumerate(anno_infos):
        b, k = int(offsets[i]), int(valid[i])
        if k == 0:
            annos.append(_empty_anno())
            continue
        c, lab = cols[b:b + k], labels[b:b + k]
        annos.append(dict(name=names[lab].astype(f'<U{int(name_len[lab].max())}'), truncated=np.zeros(k),
                          occluded=np.zeros(k, dtype=np.int64), alpha=c[:, 11].copy(), bbox=c[:, 0:4].copy(),
                          dimensions=c[:, 4:7].copy(), location=c[:, 7:10].copy(), rotation_y=c[:, 10].copy(),
                          score=c[:, 12].copy(), sample_idx=np.array([info['image']['image_idx']] * k, dtype=np.int64)))
    return annos
