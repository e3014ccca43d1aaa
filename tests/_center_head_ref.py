"""float64 restatements for the supervised CenterPoint head tests (tests/test_center_head_gpu.py) and the shapes the golden
file tests/golden/center_head.npz was generated on (tools_dev/make_golden_center_head.py imports this module, so that the
generator and the tests cannot disagree on a config or on the synthetic head maps)."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)

# voxel 0.05, factor 8, range [0, -9.6, -3, 12.8, 9.6, 1] -> a 32 x 48 map (W x H); K = 4 slots; B = 3 frames
TRAIN_CFG = dict(point_cloud_range=[0, -9.6, -3, 12.8, 9.6, 1], grid_size=[256, 384, 40], voxel_size=[0.05, 0.05, 0.1],
                 out_size_factor=8, dense_reg=1, gaussian_overlap=0.1, max_objs=4, min_radius=2,
                 code_weights=[1.0, 0.5, 2.0, 1.0, 0.25, 1.5, 1.0, 0.75])
B, K, H, W = 3, 4, 48, 32
LAYOUTS = {
    'A': [['Pedestrian'], ['Cyclist'], ['Car']],                 # three one-class tasks
    'B': [['Pedestrian', 'Cyclist'], ['Car']],                   # class-major slot order, a two-channel heat map
}
LOSS_CLS = {'A': dict(alpha=0.0, gamma=4.0), 'B': dict(alpha=2.0, gamma=4.0)}
LOSS_WEIGHT = 0.25
HEADS = (('reg', 2), ('height', 1), ('dim', 3), ('rot', 2))


def synth_map(shape, seed, lo=-2.0, hi=2.0):
    """A head map from integer arithmetic alone (a multiplicative hash of the element index), so that the generator and the
    tests build bit-identical float32 inputs on any machine."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503) + np.uint64(12345)) % np.uint64(1 << 32)
    h = (h * np.uint64(1103515245) + np.uint64(12345)) % np.uint64(1 << 31)
    x = (h >> np.uint64(7)).astype(np.float64) / float(1 << 24)            # 24 bits: exact in float32
    return torch.from_numpy((lo + (hi - lo) * x).astype(np.float32).reshape(shape))


def synth_preds(layout, batch=B):
    """[[{heatmap, reg, height, dim, rot}]] per task, float32, as the head's forward returns them."""
    out = []
    for t, names in enumerate(LAYOUTS[layout]):
        pd = {'heatmap': synth_map((batch, len(names), H, W), 100 * t + 1, -6.0, 2.0)}
        for j, (head, ch) in enumerate(HEADS):
            pd[head] = synth_map((batch, ch, H, W), 100 * t + 10 + j)
        out.append([pd])
    return out


def focal_ref(logits, target, alpha, gamma):
    """clip_sigmoid + GaussianFocalLoss(reduction='mean', avg_factor=max(num_pos, 1)) in the dtype of ``logits``."""
    p = torch.clamp(torch.sigmoid(logits), min=1e-4, max=1 - 1e-4)
    t = target.to(logits.dtype)
    pos = t.eq(1).to(logits.dtype)
    loss = -(p + 1e-12).log() * (1 - p).pow(alpha) * pos - (1 - p + 1e-12).log() * p.pow(alpha) * (1 - t).pow(gamma)
    return loss.sum() / (max(float(pos.sum()), 1.0) + EPS32)


def gather_ref(pd, ind):
    pred = torch.cat([pd['reg'], pd['height'], pd['dim'], pd['rot']], dim=1).permute(0, 2, 3, 1)
    pred = pred.reshape(pred.shape[0], -1, pred.shape[3])
    return pred.gather(1, ind.unsqueeze(2).expand(-1, -1, pred.shape[2]))


def reg_loss_ref(pred, anno, mask, code_weights, loss_weight):
    """The masked, code-weighted L1 with a NaN target weighing nothing - in loss and gradient (``torch.where``: a plain
    ``0 * |pred - NaN|`` is NaN)."""
    a = anno.to(pred.dtype)
    w = mask.to(pred.dtype).unsqueeze(2) * pred.new_tensor(code_weights)
    live = ~torch.isnan(a)
    diff = torch.where(live, (pred - torch.where(live, a, torch.zeros_like(a))).abs(), torch.zeros_like(pred))
    num = np.float32(np.float32(float(mask.sum())) + np.float32(1e-4))
    return loss_weight * (diff * w).sum() / (float(num) + EPS32)


def loss_ref(preds, heatmaps, anno_boxes, inds, masks, code_weights, loss_weight, alpha, gamma):
    """The reference's loss dict (centerpoint_head.py:598-639) on ``preds`` of any float dtype."""
    out = {}
    for t, pd in enumerate(preds):
        pd = pd[0]
        out[f'task{t}.loss_heatmap'] = focal_ref(pd['heatmap'], heatmaps[t], alpha, gamma)
        out[f'task{t}.loss_bbox'] = reg_loss_ref(gather_ref(pd, inds[t]), anno_boxes[t], masks[t], code_weights, loss_weight)
    return out


def anno_ref64(boxes):
    """Columns 3:8 of ``anno_box`` for float32 boxes [n, 7], evaluated in float64: log dx, log dy, log dz, sin yaw, cos yaw."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.stack([np.log(b[:, 3]), np.log(b[:, 4]), np.log(b[:, 5]), np.sin(b[:, 6]), np.cos(b[:, 6])], 1)
