"""The CPU oracle (oracle/) against golden vectors produced by the imported reference
(tools_dev/make_golden.py) and the reference's own known-answer tests. CPU only."""
import numpy as np
import pytest
import torch

from conftest import FMAP, TRAIN_CFG, load_head_case
from gga_amd import synthetic
from oracle import oracle as O


@pytest.mark.parametrize('case', ['second', 'second_coarse', 'pp', 'pp_dense', 'ka'])
def test_hard_voxelize_bit_exact(golden, case):
    d = golden('voxelize')
    if case == 'ka':  # reference tests/test_models/test_voxel_encoder/test_voxel_generator.py:7-22
        vs, rng, mp, mv = [0.5] * 3, [0, -40, -3, 70.4, 40, 1], 1000, 20000
    else:
        cfg = d[f'{case}.cfg']
        vs, rng, mp, mv = cfg[:3], cfg[3:9], int(cfg[9]), int(cfg[10])
    v, c, n = O.hard_voxelize(d[f'{case}.points'], vs, rng, mp, mv)
    assert np.array_equal(c, d[f'{case}.coors'])
    assert np.array_equal(n, d[f'{case}.num_points'])
    assert np.array_equal(v, d[f'{case}.voxels'])
    if case == 'ka':
        assert c.tolist() == [[7, 81, 1], [6, 81, 0], [7, 80, 1], [6, 81, 1],
                              [7, 81, 0], [6, 80, 1], [7, 80, 0], [6, 80, 0]]
        assert n.tolist() == [120, 121, 127, 134, 115, 127, 125, 131]


def test_grid_size():
    assert O.grid_size([0.05, 0.05, 0.1], [0, -40, -3, 70.4, 40, 1]).tolist() == [1408, 1600, 40]
    assert O.grid_size([0.16, 0.16, 4], [0, -39.68, -3, 69.12, 39.68, 1]).tolist() == [432, 496, 1]


def test_voxel_mean(golden):
    d = golden('encoders')
    out = O.voxel_mean(d['vfe.voxels'], d['vfe.num_points'])
    np.testing.assert_allclose(out, d['vfe.out'], rtol=1e-6, atol=1e-6)


def test_pfn_forward(golden):
    d = golden('encoders')
    cfg = d['pfn.cfg']
    out, feats, mean, var = O.pfn_forward(d['pfn.voxels'], d['pfn.num_points'], d['pfn.coors'],
                                          cfg[:3], cfg[3:], d['pfn.linear_w'], d['pfn.bn_w'], d['pfn.bn_b'])
    np.testing.assert_allclose(out, d['pfn.out'], rtol=1e-4, atol=1e-4)  # north_star fp32 tolerance
    rows = feats.shape[0] * feats.shape[1]
    # BatchNorm1d(momentum=0.01): running = 0.99*init + 0.01*batch (unbiased var)
    np.testing.assert_allclose(0.01 * mean, d['pfn.running_mean'], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(0.99 + 0.01 * var * rows / (rows - 1), d['pfn.running_var'], rtol=1e-5)


@pytest.mark.parametrize('case', ['small', 'pp'])
def test_pillar_scatter(golden, case):
    d = golden('scatter')
    B, C, ny, nx = d[f'{case}.shape']
    out = O.pillar_scatter(d[f'{case}.feats'], d[f'{case}.coors'], B, ny, nx)
    assert np.array_equal(out, d[f'{case}.canvas'])


def test_gaussian(golden):
    d = golden('gaussian')
    hm = np.zeros((128, 128), np.float32)
    O.draw_gaussian(hm, 64, 64, 2)
    assert abs(hm.sum() - 4.3505) < 1e-3          # reference tests/test_utils/test_utils.py:12-17
    for (h, w), r in zip(d['radius.sizes'], d['radius.values']):
        assert O.gaussian_radius(h, w, 0.1) == pytest.approx(r, rel=1e-14)
    hm = np.zeros((200, 176), np.float32)
    for (cx, cy), r in zip(d['splat.centers'], d['splat.radii']):
        O.draw_gaussian(hm, cx, cy, r)
    np.testing.assert_allclose(hm, d['splat.heatmap'], rtol=0, atol=1e-7)
    assert np.array_equal(hm == 1, d['splat.heatmap'] == 1)


def _targets(d, c):
    case = load_head_case(d, c)
    torch.manual_seed(1234)
    srl = O.draw_srl(case['B'])
    tg = O.get_targets(case['labels'], case['boxes_img'], case['lidar2img'], case['pseudo'],
                       case['bdry'], case['ibp'], case['meta_l2i'], TRAIN_CFG[c], srl)
    return case, tg


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_get_targets(golden, c):
    d = golden('head')
    case, tg = _targets(d, c)
    for t in range(3):
        hm = np.zeros_like(tg['heatmap'][t])
        idx = d[f'{c}.tgt.{t}.heatmap.idx']
        hm[tuple(idx.T)] = d[f'{c}.tgt.{t}.heatmap.val']
        np.testing.assert_allclose(tg['heatmap'][t], hm, rtol=0, atol=1e-7)
        assert np.array_equal(tg['heatmap'][t] == 1, hm == 1)
        assert np.array_equal(tg['ind'][t], d[f'{c}.tgt.{t}.ind'])
        assert np.array_equal(tg['mask'][t], d[f'{c}.tgt.{t}.mask'])
        assert np.array_equal(tg['bound_mask'][t], d[f'{c}.tgt.{t}.bound_mask'])
        assert np.array_equal(tg['lidar2img'][t], d[f'{c}.tgt.{t}.lidar2img'])
        np.testing.assert_array_equal(tg['anno_box'][t], d[f'{c}.tgt.{t}.anno_box'])
        n_ibp = d[f'{c}.tgt.{t}.n_ibp']
        for b in range(case['B']):
            got = [len(p) for p in tg['ibp'][t][b]]
            assert got == [x for x in n_ibp[b] if x >= 0]


@pytest.mark.parametrize('c', ['second', 'pp'])
def test_head_loss(golden, c):
    d = golden('head')
    case, tg = _targets(d, c)
    H, W = FMAP[c]
    preds = [{k: v.numpy() for k, v in p.items()}
             for p in synthetic.make_head_preds(case['B'], H, W, seed=int(d[f'{c}.pred_seed']))]
    losses, mids = O.head_loss(preds, tg, TRAIN_CFG[c])
    for t in range(3):
        for k in ('pred', 'rot', 'pred_ratio', 'pred_box_bev'):
            np.testing.assert_allclose(mids[t][k], d[f'{c}.mid.{t}.{k}'], rtol=2e-6, atol=2e-6, err_msg=k)
        # pixel coordinates reach ~1e3: relative tolerance
        np.testing.assert_allclose(mids[t]['pred_iou'], d[f'{c}.mid.{t}.pred_iou'], rtol=1e-5, atol=1e-3)
        for k in ('p2c_min', 'p2c_x', 'p2c_y'):
            np.testing.assert_allclose(mids[t][k], d[f'{c}.mid.{t}.{k}'], rtol=1e-5, atol=1e-4, err_msg=k)
    assert len(losses) == 18
    for k, v in losses.items():
        ref = float(d[f'{c}.loss.{k}'])
        assert float(v) == pytest.approx(ref, rel=1e-5, abs=1e-4), k   # north_star: fp32 losses within 1e-4


def test_focal_grad_matches_reference(golden):
    d = golden('head')
    c = 'second'
    case, tg = _targets(d, c)
    H, W = FMAP[c]
    preds = synthetic.make_head_preds(case['B'], H, W, seed=int(d[f'{c}.pred_seed']))
    for t in range(3):
        _, g, _ = O.focal_loss(preds[t]['heatmap'].numpy(), tg['heatmap'][t], with_grad=True)
        sel = d[f'{c}.gradA.{t}.heatmap.flatidx']
        np.testing.assert_allclose(5.0 * g[sel], d[f'{c}.gradA.{t}.heatmap.val'], rtol=1e-4, atol=1e-7)


def test_rotation_known_answer(golden):
    # reference tests/test_utils/test_box3d.py:1598-1607 through the oracle's PAL rotation:
    # rotating clockwise by -a equals the counter-clockwise rotation by a.
    d = golden('rotation')
    p, a, out = d['ka2d.points'][0], float(d['ka2d.angles'][0]), d['ka2d.out'][0]
    c, s = np.cos(a), np.sin(a)
    got = np.stack([p[:, 0] * c - p[:, 1] * s, p[:, 0] * s + p[:, 1] * c], 1)
    np.testing.assert_allclose(got, out, atol=1e-7)


# ---- §8(f) rank 1 ops: the reference's own known-answer tests ---------------------------------
KA_PTS = np.array([[1.0, 4.3, 0.1], [1.0, 4.4, 0.1], [1.1, 4.3, 0.1], [0.9, 4.3, 0.1], [1.0, -0.3, 0.1],
                   [1.0, -0.4, 0.1], [2.9, 0.1, 6.0], [-0.9, 3.9, 6.0]], np.float32)
KA_BOXES = np.array([[1.0, 2.0, 0.0, 4.0, 4.0, 6.0, np.pi / 6], [1.0, 2.0, 0.0, 4.0, 4.0, 6.0, np.pi / 2],
                     [1.0, 2.0, 0.0, 4.0, 4.0, 6.0, 7 * np.pi / 6], [1.0, 2.0, 0.0, 4.0, 4.0, 6.0, -np.pi / 6]], np.float32)
KA_ALL = [[1, 0, 1, 1], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1], [1, 0, 1, 1], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]]
KA_PART = [0, -1, 0, 3, 0, -1, 1, 1]
KA_DEPTH_BOXES = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.3], [-10.0, 23.0, 16.0, 10, 20, 20, 0.5]], np.float32)
KA_DEPTH_PTS = np.array([[1, 2, 3.3], [1.2, 2.5, 3.0], [0.8, 2.1, 3.5], [1.6, 2.6, 3.6], [0.8, 1.2, 3.9],
                         [-9.2, 21.0, 18.2], [3.8, 7.9, 6.3], [4.7, 3.5, -12.2], [3.8, 7.6, -2], [-10.6, -12.9, -20],
                         [-16, -18, 9], [-21.3, -52, -5], [0, 0, 0], [6, 7, 8], [-2, -3, -4]], np.float32)
KA_DEPTH_PART = [0, 0, 0, 0, 0, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1]
KA_NMS_BOXES = np.array([[6.0, 3.0, 8.0, 7.0, 2.0], [3.0, 6.0, 9.0, 11.0, 1.0], [3.0, 7.0, 10.0, 12.0, 1.0],
                         [1.0, 4.0, 13.0, 7.0, 3.0]], np.float32)
KA_NMS_SCORES = np.array([0.6, 0.9, 0.7, 0.2], np.float32)
KA_OV1 = np.array([[1.8, -2.5, -1.8, 1.75, 3.39, 1.65, -1.6615927], [8.9, -2.5, -1.6, 1.54, 4.01, 1.57, -1.5215927],
                   [28.3, 0.5, -1.3, 1.47, 2.23, 1.48, -4.7115927], [31.3, -8.2, -1.6, 1.74, 3.77, 1.48, -0.35]], np.float32)
KA_OV2 = np.array([[1.2, -3.0, -1.9, 1.8, 3.4, 1.7, -1.9], [8.1, -2.9, -1.8, 1.5, 4.1, 1.6, -1.8],
                   [31.3, -8.2, -1.6, 1.74, 3.77, 1.48, -0.35], [20.1, -28.5, -1.9, 1.6, 3.5, 1.4, -5.1]], np.float32)
KA_IOU3D = np.array([[0.3710, 0, 0, 0], [0, 0.3322, 0, 0], [0, 0, 0, 0], [0, 0, 1.0, 0]], np.float32)
KA_IOF3D = np.array([[0.5582, 0, 0, 0], [0, 0.5025, 0, 0], [0, 0, 0, 0], [0, 0, 1.0, 0]], np.float32)


def overlaps_3d_from_bev(iou2d_fn, b1, b2, mode):
    """BaseInstance3DBoxes.overlaps (base_box3d.py:440-500) around a BEV rotated-IoU function."""
    top1, bot1 = b1[:, 2] + b1[:, 5], b1[:, 2]
    top2, bot2 = b2[:, 2] + b2[:, 5], b2[:, 2]
    oh = np.clip(np.minimum(top1[:, None], top2[None]) - np.maximum(bot1[:, None], bot2[None]), 0, None)
    bev1, bev2 = b1[:, [0, 1, 3, 4, 6]], b2[:, [0, 1, 3, 4, 6]]
    iou2d = iou2d_fn(bev1, bev2)
    a1, a2 = (bev1[:, 2] * bev1[:, 3])[:, None], (bev2[:, 2] * bev2[:, 3])[None]
    ov = iou2d * (a1 + a2) / (1 + iou2d) * oh
    v1, v2 = (b1[:, 3] * b1[:, 4] * b1[:, 5])[:, None], (b2[:, 3] * b2[:, 4] * b2[:, 5])[None]
    return ov / np.clip(v1 + v2 - ov, 1e-8, None) if mode == 'iou' else ov / np.clip(v1, 1e-8, None)


def test_points_in_boxes_known_answers():    # reference tests/test_utils/test_box3d.py:1683-1745
    assert O.points_in_boxes(KA_PTS, KA_BOXES, all_boxes=True).tolist() == KA_ALL
    assert O.points_in_boxes(KA_PTS, KA_BOXES).tolist() == KA_PART
    assert O.points_in_boxes(KA_DEPTH_PTS, KA_DEPTH_BOXES).tolist() == KA_DEPTH_PART


def test_nms_bev_known_answer():              # reference tests/test_utils/test_nms.py:82-98
    assert O.nms_bev(KA_NMS_BOXES, KA_NMS_SCORES, 0.3).tolist() == [1, 0, 3]


def test_boxes3d_overlaps_known_answer():     # reference tests/test_utils/test_box3d.py:1122-1158
    np.testing.assert_allclose(overlaps_3d_from_bev(O.box_iou_rotated, KA_OV1, KA_OV2, 'iou'), KA_IOU3D,
                               rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(overlaps_3d_from_bev(O.box_iou_rotated, KA_OV1, KA_OV2, 'iof'), KA_IOF3D,
                               rtol=1e-3, atol=1e-4)


# ----------------------------------------------------------------------------- sparse conv restatements
@pytest.mark.parametrize('cfg', [
    dict(subm=True, cin=4, cout=16, k=3, s=1, p=1),
    dict(subm=False, cin=16, cout=32, k=3, s=2, p=1),
    dict(subm=False, cin=8, cout=8, k=3, s=2, p=(0, 1, 1)),
    dict(subm=False, cin=8, cout=12, k=(3, 1, 1), s=(2, 1, 1), p=0),
    dict(subm=False, cin=5, cout=6, k=3, s=1, p=0),
])
def test_sparse_pair_list_restatement_equals_dense_restatement(cfg):
    """oracle/sparse_ref.conv_ref_pairs (runs at the real grid size) against conv_ref (dense conv3d,
    the published definition) on a small grid: same site set, same order, same values and gradients."""
    import torch
    from gga_amd.sparse import SparseConv3d, SubMConv3d
    from oracle import sparse_ref as SR
    torch.manual_seed(0)
    shape, B = (9, 14, 12), 2
    g = torch.Generator().manual_seed(4)
    coors = []
    for b in range(B):
        pts = torch.stack([torch.randint(0, shape[0], (150,), generator=g), torch.randint(0, shape[1], (150,), generator=g),
                           torch.randint(0, shape[2], (150,), generator=g)], 1)
        pts = torch.unique(pts, dim=0)
        pts = pts[torch.randperm(len(pts), generator=g)]
        coors.append(torch.cat([torch.full((len(pts), 1), b), pts], 1))
    coors = torch.cat(coors).int()
    cls = SubMConv3d if cfg['subm'] else SparseConv3d
    conv = cls(cfg['cin'], cfg['cout'], cfg['k'], stride=cfg['s'], padding=cfg['p'], bias=False)
    x1 = torch.randn(len(coors), cfg['cin'], requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)
    y1, c1, s1 = SR.conv_ref(conv, x1, coors, B, shape)
    w_grad_dense = torch.autograd.grad(y1.square().sum(), [x1, conv.weight])
    y2, c2, s2 = SR.conv_ref_pairs(conv, x2, coors, B, shape)
    w_grad_pairs = torch.autograd.grad(y2.square().sum(), [x2, conv.weight])
    assert tuple(s1) == tuple(s2) and torch.equal(c1.long(), c2.long())
    torch.testing.assert_close(y1, y2, rtol=1e-5, atol=1e-5)
    for a, b in zip(w_grad_dense, w_grad_pairs):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


def test_circle_nms_reference_known_answer():
    # reference tests/test_utils/test_nms.py:63-79
    boxes = np.array([[-11.1100, 2.1300, 0.8823], [-11.2810, 2.2422, 0.8914], [-10.3966, -0.3198, 0.8643],
                      [-10.2906, -13.3159, 0.8401], [5.6518, 9.9791, 0.8271], [-11.2652, 13.3637, 0.8267],
                      [4.7768, -13.0409, 0.7810], [5.6621, 9.0422, 0.7753], [-10.5561, 18.9627, 0.7518],
                      [-10.5643, 13.2293, 0.7200]], np.float32)
    keep = O.circle_nms(boxes, 0.175)
    assert sorted(keep) == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert keep[0] == 1          # highest score first
