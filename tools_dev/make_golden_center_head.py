#!/usr/bin/env python
"""Golden vectors of the supervised CenterPoint head: tests/golden/center_head.npz.

A sibling of tools_dev/make_golden.py (its stubs for the absent third-party packages are reused): the reference's
``CenterHead`` (mmdet3d/models/dense_heads/centerpoint_head.py) is loaded by path and its ``get_targets`` / ``loss`` run on
the CPU on hand-made frames that hold every edge the device path has to get right. Only inputs and outputs are written.

    python tools_dev/make_golden_center_head.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_golden as mg  # noqa: E402
import _center_head_ref as R  # noqa: E402
from gga_amd.dense_heads import gaussian_radius_np  # noqa: E402
from gga_amd.losses import GaussianFocalLoss, L1Loss  # noqa: E402

CELL = 0.05 * 8
X0, Y0 = 0.0, -9.6


class _Boxes:
    """What ``get_targets_single`` reads of a LiDAR box structure: ``tensor`` and ``gravity_center``."""

    def __init__(self, tensor):
        self.tensor = tensor

    @property
    def gravity_center(self):
        gc = torch.zeros_like(self.tensor[:, :3])
        gc[:, :2] = self.tensor[:, :2]
        gc[:, 2] = self.tensor[:, 2] + self.tensor[:, 5] * 0.5
        return gc


def in_band(v):
    f = abs(v) - np.floor(abs(v))
    return 0.01 <= f <= 0.99


def scaled(v, vs):
    """The reference's f32 ``v / voxel_size / out_size_factor``, as float64."""
    return float(np.float32(np.float32(v) / np.float32(vs)) / np.float32(8))


def radius64(dx, dy):
    return float(gaussian_radius_np(np.float64(scaled(dy, 0.05)), np.float64(scaled(dx, 0.05)), 0.1))


def draw_size(rng, lo, hi):
    """(dx, dy) in metres whose float64 gaussian radius has a fractional part in [0.01, 0.99] (about 2 % of random sizes
    fall outside and are drawn again)."""
    while True:
        dx, dy = np.float32(rng.uniform(lo, hi)), np.float32(rng.uniform(lo, hi))
        if in_band(radius64(dx, dy)):
            return float(dx), float(dy)


def at_cell(rng, cx, cy):
    """A centre inside cell (cx, cy) (or off the map for cells outside it), fractional parts in [0.1, 0.9]."""
    while True:
        x = np.float32(X0 + (cx + rng.uniform(0.1, 0.9)) * CELL)
        y = np.float32(Y0 + (cy + rng.uniform(0.1, 0.9)) * CELL)
        fx = float(np.float32(np.float32(np.float32(x) - np.float32(X0)) / np.float32(0.05)) / np.float32(8))
        fy = float(np.float32(np.float32(np.float32(y) - np.float32(Y0)) / np.float32(0.05)) / np.float32(8))
        if in_band(fx) and in_band(fy):
            return float(x), float(y)


def make_frames(seed=20):
    rng = np.random.RandomState(seed)

    def obj(label, cell, size=None, lo=0.4, hi=4.5, dz=1.6, **over):
        x, y = at_cell(rng, *cell)
        dx, dy = size if size is not None else draw_size(rng, lo, hi)
        o = dict(label=label, x=x, y=y, z=float(np.float32(rng.uniform(-2.5, -0.5))), dx=dx, dy=dy, dz=dz,
                 yaw=float(np.float32(rng.uniform(-3.1, 3.1))))
        o.update(over)
        return o

    frames = [[]]                                                          # frame 0: no objects
    # frame 1: six cars (> K), unknown labels, every side off the map; the classes interleaved
    frames.append([
        obj(2, (5, 7)), obj(0, (-2, 10)), obj(1, (12, -2)), obj(2, (20, 30)), obj(-1, (9, 9)), obj(0, (8, 20), lo=0.4, hi=0.9),
        obj(2, (11, 40)), obj(7, (15, 15)), obj(1, (14, 49)), obj(2, (27, 12)), obj(0, (33, 5)), obj(2, (3, 25)),
        obj(1, (22, 22), lo=0.5, hi=1.9), obj(2, (16, 4))])
    # frame 2: width 0, negative length, dz < 0, two cars in one cell, min_radius clamp, a splat cut by the border
    frames.append([
        obj(2, (10, 10), lo=3.0, hi=4.5), obj(0, (6, 6), size=(0.0, 0.8)), obj(1, (7, 30), size=(1.7, -0.6)),
        obj(2, (10, 10), lo=1.5, hi=2.5), obj(1, (25, 40), lo=0.5, hi=1.9, dz=-1.5), obj(0, (18, 33), lo=0.4, hi=0.6),
        obj(2, (0, 47), lo=5.0, hi=9.0), obj(2, (31, 0), lo=5.0, hi=9.0)])
    return frames


def check_conditions(frames):
    radii = []
    for f in frames:
        for o in f:
            if not (o['dx'] > 0 and o['dy'] > 0):
                continue
            r = radius64(o['dx'], o['dy'])
            fx = float(np.float32(np.float32(np.float32(o['x']) - np.float32(X0)) / np.float32(0.05)) / np.float32(8))
            fy = float(np.float32(np.float32(np.float32(o['y']) - np.float32(Y0)) / np.float32(0.05)) / np.float32(8))
            assert in_band(r) and in_band(fx) and in_band(fy), (o, r, fx, fy)
            assert not (-1 < fx < 0 or -1 < fy < 0), o
            radii.append(r)
    return radii


def slot_objects(frames, layout):
    """[T, B, K] object index inside its frame (or -1): class-major, then index order, the first K."""
    names = R.LAYOUTS[layout]
    T = len(names)
    base = np.concatenate([[0], np.cumsum([len(n) for n in names])])
    out = -np.ones((T, len(frames), R.K), np.int64)
    for b, f in enumerate(frames):
        for t in range(T):
            order = [i for c in range(base[t], base[t + 1]) for i, o in enumerate(f) if o['label'] == c]
            for k, i in enumerate(order[:R.K]):
                out[t, b, k] = i
    return out


def make_ref_head(ref_mod, layout):
    H = ref_mod.CenterHead
    h = H.__new__(H)
    nn.Module.__init__(h)
    h.norm_bbox, h.with_velocity = True, False
    h.class_names = R.LAYOUTS[layout]
    h.task_heads = list(range(len(h.class_names)))
    h.train_cfg = R.TRAIN_CFG
    h.loss_cls = GaussianFocalLoss(reduction='mean', **R.LOSS_CLS[layout])
    h.loss_bbox = L1Loss(reduction='mean', loss_weight=R.LOSS_WEIGHT)
    return h


def main():
    mg.import_reference()
    ref_mod = mg.load('mmdet3d.models.dense_heads.centerpoint_head', 'mmdet3d/models/dense_heads/centerpoint_head.py')
    frames = make_frames()
    radii = check_conditions(frames)
    cols = ('x', 'y', 'z', 'dx', 'dy', 'dz', 'yaw')
    boxes = [torch.tensor([[o[c] for c in cols] for o in f], dtype=torch.float32).reshape(-1, 7) for f in frames]
    labels = [torch.tensor([o['label'] for o in f], dtype=torch.int64) for f in frames]
    out = {'boxes': torch.cat(boxes).numpy(), 'labels': torch.cat(labels).numpy(),
           'frame_offsets': np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)}
    for layout in R.LAYOUTS:
        head = make_ref_head(ref_mod, layout)
        with np.errstate(invalid='ignore'):
            heat, anno, ind, mask = head.get_targets([_Boxes(b) for b in boxes], labels)
        slots = slot_objects(frames, layout)
        for t in range(len(heat)):
            out[f'{layout}.heatmap.{t}'] = heat[t].numpy()
            out[f'{layout}.anno_box.{t}'] = anno[t].numpy()
            out[f'{layout}.ind.{t}'] = ind[t].numpy()
            out[f'{layout}.mask.{t}'] = mask[t].numpy()
            # every live slot is the object the restated slot order names (the others may be skipped objects)
            for b in range(R.B):
                for k in range(R.K):
                    if mask[t][b, k]:
                        o = frames[b][slots[t, b, k]]
                        np.testing.assert_allclose(anno[t][b, k, 3].item(), np.log(np.float32(o['dx'])), rtol=1e-6)
                        np.testing.assert_allclose(anno[t][b, k, 6].item(), np.sin(np.float32(o['yaw'])), atol=1e-6)
        out[f'{layout}.slot_obj'] = slots
        preds = R.synth_preds(layout)
        losses = head.loss([_Boxes(b) for b in boxes], labels, preds)
        for k, v in losses.items():
            out[f'{layout}.{k}'] = np.array(float(v), np.float64)
        print(f'  layout {layout}:', {k: float(v) for k, v in losses.items()},
              'live slots', [int(m.sum()) for m in mask], 'NaN targets', [int(torch.isnan(a).sum()) for a in anno])
    # the cases the file has to hold
    mA = [out[f'A.mask.{t}'] for t in range(3)]
    iA = [out[f'A.ind.{t}'] for t in range(3)]
    assert all(m[0].sum() == 0 for m in mA)                                                        # the empty frame
    assert mA[2][1].sum() == R.K and (np.asarray([o['label'] for o in frames[1]]) == 2).sum() == 6    # six cars, K kept
    assert mA[0][1].tolist() == [0, 1, 0, 0] and mA[1][1].tolist() == [0, 0, 1, 0]                 # off the map: slot used, empty
    assert mA[0][2].tolist() == [0, 1, 0, 0] and mA[1][2].tolist() == [0, 1, 0, 0]                 # width 0 / negative length
    assert np.isnan(out['A.anno_box.1'][2, 1, 5]) and np.isnan(out['A.task1.loss_bbox'])     # dz < 0: NaN * 0 in the reference
    assert iA[2][2, 0] == iA[2][2, 1] and mA[2][2, :2].tolist() == [1, 1]                          # two objects in one cell
    assert min(radii) < R.TRAIN_CFG['min_radius'] < max(radii)                                     # the clamp is exercised
    assert out['B.mask.0'][1].tolist() == [0, 1, 0, 0]                                             # class-major: 3 peds, then cyclist 0
    path = os.path.join(mg.OUT, 'center_head.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path) / 1024:.1f} KiB; radii {min(radii):.2f} .. {max(radii):.2f}')


if __name__ == '__main__':
    main()
