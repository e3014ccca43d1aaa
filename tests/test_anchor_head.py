"""Anchor3DHead and VoxelNet on the CPU: generators, coder, assigner, the eager targets against the float32 restatement of the
reference's loop (tests/_anchor_head_ref.py), and the two retrain configs."""
import os

import numpy as np
import pytest
import torch

import _anchor_head_ref as R
from conftest import REPO
from gga_amd import Config, build_model
from gga_amd.anchor_head import MaxIoUAssigner, bbox_overlaps
from gga_amd.registry import build_bbox_coder, build_head, build_prior_generator

KITTI_MAPS = {      # model config -> (feature map, ranges, generator type): the two KITTI layouts
    'second': ((200, 176), [[0, -40.0, -0.6, 70.4, 40.0, -0.6]] * 2 + [[0, -40.0, -1.78, 70.4, 40.0, -1.78]], False),
    'pointpillars': ((248, 216), [[0, -39.68, -0.6, 69.12, 39.68, -0.6]] * 2 + [[0, -39.68, -1.78, 69.12, 39.68, -1.78]], True),
}


# ----------------------------------------------------------------------------- generators
def test_range_generator_repr_and_shape():
    # tests/test_utils/test_anchors.py:13-43 of the reference
    gen = build_prior_generator(dict(
        type='Anchor3DRangeGenerator',
        ranges=[[0, -39.68, -0.6, 70.4, 39.68, -0.6], [0, -39.68, -0.6, 70.4, 39.68, -0.6], [0, -39.68, -1.78, 70.4, 39.68, -1.78]],
        sizes=[[0.8, 0.6, 1.73], [1.76, 0.6, 1.73], [3.9, 1.6, 1.56]], rotations=[0, 1.57], reshape_out=False))
    assert repr(gen) == ('Anchor3DRangeGenerator(anchor_range=[[0, -39.68, -0.6, 70.4, 39.68, -0.6], '
                         '[0, -39.68, -0.6, 70.4, 39.68, -0.6], [0, -39.68, -1.78, 70.4, 39.68, -1.78]],'
                         '\nscales=[1],\nsizes=[[0.8, 0.6, 1.73], [1.76, 0.6, 1.73], [3.9, 1.6, 1.56]],'
                         '\nrotations=[0, 1.57],\nreshape_out=False,\nsize_per_range=True)')
    assert gen.single_level_grid_anchors((256, 256), 1.1, device='cpu').shape == torch.Size([1, 256, 256, 3, 2, 7])
    assert gen.num_base_anchors == 6 and gen.num_levels == 1


def test_aligned_generator_known_answers():
    # tests/test_utils/test_anchors.py:46-186 of the reference: rows [:56:7] of every level
    gen = build_prior_generator(dict(
        type='AlignedAnchor3DRangeGenerator', ranges=[[-51.2, -51.2, -1.80, 51.2, 51.2, -1.80]], scales=[1, 2, 4],
        sizes=[[2.5981, 0.8660, 1.], [1.7321, 0.5774, 1.], [1., 1., 1.], [0.4, 0.4, 1]], custom_values=[0, 0],
        rotations=[0, 1.57], size_per_range=False, reshape_out=True))
    assert gen.num_base_anchors == 8
    levels = gen.grid_anchors([(256, 256), (128, 128), (64, 64)], device='cpu')
    assert [tuple(a.shape) for a in levels] == [(524288, 9), (131072, 9), (32768, 9)]
    base = [[2.5981, 0.8660, 1.0, 0.0], [0.4, 0.4, 1.0, 1.57], [0.4, 0.4, 1.0, 0.0], [1.0, 1.0, 1.0, 1.57], [1.0, 1.0, 1.0, 0.0],
            [1.7321, 0.5774, 1.0, 1.57], [1.7321, 0.5774, 1.0, 0.0], [2.5981, 0.8660, 1.0, 1.57]]
    first_x = [(-51.0, 0.4), (-50.8, 0.8), (-50.4, 1.6)]
    for lvl, (anchors, scale, (x0, step)) in enumerate(zip(levels, (1, 2, 4), first_x)):
        xs = [x0, x0] + [x0 + step * k for k in range(1, 7)]
        want = torch.tensor([[x, x0, -1.8, b[0] * scale, b[1] * scale, b[2] * scale, b[3], 0.0, 0.0] for x, b in zip(xs, base)])
        assert anchors[:56:7].allclose(want), lvl
    assert gen.grid_anchors([(256, 256), (128, 128), (64, 64)], device='cpu')[0] is levels[0]       # built once, then kept


@pytest.mark.parametrize('name', sorted(KITTI_MAPS))
def test_generators_equal_the_restatement_bit_for_bit(name):
    feat, ranges, aligned = KITTI_MAPS[name]
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', f'gga_kitti_retrain_{name}.py'))
    gcfg = dict(cfg.model['bbox_head']['anchor_generator'])
    assert gcfg['type'] == ('AlignedAnchor3DRangeGenerator' if aligned else 'Anchor3DRangeGenerator')
    assert [list(r) for r in gcfg['ranges']] == ranges
    got = build_prior_generator(gcfg).grid_anchors([feat], device='cpu')[0]
    want = R.ref_anchors(feat, ranges, R.SIZES, R.ROTATIONS, aligned)
    assert got.shape == (1, feat[0], feat[1], 3, 2, 7) and got.dtype == torch.float32
    assert torch.equal(got, want)


def test_fixture_generators_equal_the_restatement():
    for aligned in (True, False):
        got = build_prior_generator(R.generator_cfg(aligned)).grid_anchors([R.FEAT], device='cpu')[0]
        assert got.numel() == 864 * 7 and torch.equal(got, R.fixture_anchors(aligned))


# ----------------------------------------------------------------------------- coder, assigner
def test_coder_round_trip():
    coder = build_bbox_coder(dict(type='DeltaXYZWLHRBBoxCoder'))
    assert coder.code_size == 7
    anchors = R.fixture_anchors().reshape(-1, 7)[::37][:20]
    boxes, _ = R.random_boxes(20, 3)
    enc = coder.encode(anchors, boxes)
    assert torch.equal(enc, R.ref_encode(anchors, boxes))
    np.testing.assert_allclose(coder.decode(anchors, enc).numpy(), boxes.numpy(), rtol=1e-5, atol=1e-5)


def test_assigner_known_answer():
    # tests/test_utils/test_assigners.py:13-34 of the reference
    bboxes = torch.FloatTensor([[0, 0, 10, 10], [10, 10, 20, 20], [5, 5, 15, 15], [32, 32, 38, 42]])
    gt_bboxes = torch.FloatTensor([[0, 0, 10, 9], [0, 10, 10, 19]])
    res = MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5).assign(bboxes, gt_bboxes, gt_labels=torch.LongTensor([2, 3]))
    assert res.gt_inds.tolist() == [1, 0, 2, 0] and len(res.labels) == 4
    assert res.labels.tolist() == [2, -1, 3, -1]
    assert R.ref_assign(R.ref_overlaps(gt_bboxes, bboxes), 0.5, 0.5, 0.0).tolist() == [1, 0, 2, 0]
    assert torch.equal(bbox_overlaps(gt_bboxes, bboxes), R.ref_overlaps(gt_bboxes, bboxes))


@pytest.mark.parametrize('key, value', [('neg_iou_thr', (0.1, 0.3)), ('gt_max_assign_all', False), ('match_low_quality', False),
                                        ('ignore_iof_thr', 0.5), ('gpu_assign_thr', 100)])
def test_assigner_refuses_what_it_does_not_implement(key, value):
    kw = dict(pos_iou_thr=0.5, neg_iou_thr=0.4)
    kw[key] = value
    with pytest.raises(NotImplementedError, match=key):
        MaxIoUAssigner(**kw)


# ----------------------------------------------------------------------------- the fixture and the eager targets
def test_the_fixture_holds_its_cases():
    anchors = R.fixture_anchors(True)
    t = R.ref_targets_batch(anchors, R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, True, R.NUM_CLASSES)
    ped, cyc, car = t['groups'][0]
    # two Cars: IoUs 1.0 and 0.82, five positives by threshold, four ignored anchors between 0.45 and 0.6
    np.testing.assert_allclose(car['iou'].max(dim=1)[0].numpy(), [1.0, 0.82], atol=5e-3)
    assert int((car['iou'].max(dim=0)[0] >= 0.6).sum()) == 5 and int((car['gt_inds'] > 0).sum()) == 5
    assert int((car['gt_inds'] < 0).sum()) == 4
    mid = car['iou'].max(dim=0)[0][car['gt_inds'] < 0]
    assert bool(((mid >= 0.45) & (mid < 0.6)).all())
    # the Pedestrian's yaw takes the pi/4 swap: the two anchors of its cell are positive, the turned one (1.57) at IoU 1.0
    assert abs(float(R.ref_limit_period(R.GT_BOXES[0][2, 6]))) > np.pi / 4
    ped_pos = (ped['gt_inds'] > 0).nonzero().reshape(-1)
    assert len(ped_pos) == 2 and int(ped_pos[0]) + 1 == int(ped_pos[1]) and int(ped_pos[0]) % 2 == 0
    assert float(ped['iou'][0][ped_pos[1]]) > 0.999 and abs(float(ped['iou'][0][ped_pos[0]]) - 0.6) < 1e-3
    # the Cyclist (yaw 3.5, outside [-pi, pi]): positive only by the low-quality rule
    assert float(R.GT_BOXES[0][3, 6]) > np.pi
    best = float(cyc['iou'].max())
    assert 0.35 <= best < 0.5 and abs(best - 0.361) < 1e-3 and int((cyc['gt_inds'] > 0).sum()) == 1
    # frame 1 is empty; frame 2: the Pedestrian matches nothing, the duplicate Cars tie and the anchor goes to the second
    assert int(t['pos_count'][1]) == 0 and bool((t['label_weights'][1] == 1).all())
    ped2, _, car2 = t['groups'][2]
    assert float(ped2['iou'].max()) < 0.35 and abs(float(ped2['iou'].max()) - 0.083) < 1e-3 and int((ped2['gt_inds'] > 0).sum()) == 0
    assert torch.equal(car2['iou'][0], car2['iou'][1]) and abs(float(car2['iou'].max()) - 0.729) < 1e-3
    a = int(car2['iou'][0].argmax())
    assert int(car2['iou'][:, a].argmax()) == 0 and int(car2['gt_inds'][a]) == 2
    # assign_per_class=False: a Cyclist anchor becomes positive for the Pedestrian box by the low-quality rule
    t2 = R.ref_targets_batch(anchors, R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, False, R.NUM_CLASSES)
    cyc_all = t2['groups'][0][1]
    hit = (cyc_all['gt_inds'] == 3).nonzero().reshape(-1)           # ground truth 2 of the frame = the Pedestrian
    assert len(hit) == 1 and abs(float(cyc_all['iou'][2, hit[0]]) - 0.455) < 1e-3 and int(cyc_all['labels'][hit[0]]) == R.PED
    assert t['pos_count'].tolist() != t2['pos_count'].tolist()
    # both direction bins and all three classes occur among the positives
    pos = t['pos'].bool()
    assert set(t['dir_targets'][pos].tolist()) == {0, 1} and set(t['labels'][pos].tolist()) == {0, 1, 2}


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('assign_per_class', [True, False])
def test_eager_targets_equal_the_restatement(aligned, assign_per_class):
    head = build_head(R.head_cfg(aligned, assign_per_class))
    anchors = head.anchor_generator.grid_anchors([R.FEAT], device='cpu')[0]
    want = R.ref_targets_batch(R.fixture_anchors(aligned), R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, assign_per_class, R.NUM_CLASSES)
    got = head.get_targets(anchors, R.GT_BOXES, R.GT_LABELS, bbox_weights=True)
    for key in ('labels', 'label_weights', 'bbox_targets', 'pos', 'dir_targets', 'dir_weights', 'pos_count'):
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert torch.equal(got['bbox_weights'], want['pos'].float()[..., None].expand(-1, -1, 7))


def test_eager_loss_equals_the_float64_restatement():
    head = build_head(R.head_cfg(True, True, train_cfg_extra=dict(code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5])))
    H, W = R.FEAT
    maps = [R.synth_map((3, 6 * c, H, W), 11 + c, 0.5) for c in (3, 7, 2)]
    metas = [dict() for _ in range(3)]
    losses = head.loss([maps[0]], [maps[1]], [maps[2]], R.GT_BOXES, R.GT_LABELS, metas)
    assert list(losses) == ['loss_cls', 'loss_bbox', 'loss_dir'] and all(len(v) == 1 for v in losses.values())
    t = R.ref_targets_batch(R.fixture_anchors(True), R.GT_BOXES, R.GT_LABELS, R.THRESHOLDS, True, R.NUM_CLASSES)
    want = R.ref_losses(*[m.double() for m in maps], t, R.NUM_CLASSES, code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5])
    for key, w in zip(losses, want):
        np.testing.assert_allclose(float(losses[key][0]), float(w), rtol=2e-5)
    # no ground truth at all: loss_bbox and loss_dir are exactly zero (tests/test_models/test_heads.py:214-221 of the reference)
    empty = head.loss([maps[0]], [maps[1]], [maps[2]], [torch.zeros(0, 7)] * 3, [torch.zeros(0, dtype=torch.long)] * 3, metas)
    assert float(empty['loss_cls'][0]) > 0 and float(empty['loss_bbox'][0]) == 0 and float(empty['loss_dir'][0]) == 0


# ----------------------------------------------------------------------------- configs
@pytest.mark.parametrize('name', ['second', 'pointpillars'])
def test_retrain_configs_build(name):
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', f'gga_kitti_retrain_{name}.py'))
    model = build_model(cfg.model)
    assert type(model).__name__ == 'VoxelNet' and type(model.bbox_head).__name__ == 'Anchor3DHead'
    prefixes = ('voxel_encoder.', 'middle_encoder.', 'backbone.', 'neck.', 'bbox_head.')
    names = list(model.state_dict())
    assert names and all(n.startswith(prefixes) for n in names)
    assert {n.split('.')[0] for n in names} >= {'backbone', 'neck', 'bbox_head'}
    head = model.bbox_head
    # tests/test_models/test_heads.py:181-185 of the reference
    assert (head.conv_cls.out_channels, head.conv_reg.out_channels, head.conv_dir_cls.out_channels) == (18, 42, 12)
    assert head.conv_cls.in_channels == cfg.model['bbox_head']['feat_channels'] and head.conv_cls.kernel_size == (1, 1)
    assert head.assign_per_class == (name == 'pointpillars') and len(head.bbox_assigner) == 3
    assert model.pts_bbox_head is head and model.pts_backbone is model.backbone        # the shared machinery's names
    assert cfg.data['train']['dataset']['ann_file'].endswith('kitti_infos_trainval_GGA_pseudo.pkl')
    assert cfg.data['val']['ann_file'].endswith('kitti_infos_val_GGA.pkl') and cfg.data['val']['type'] == 'KittiDataset'
    kinds = [t['type'] for t in cfg.data['train']['dataset']['pipeline']]
    assert 'ObjectSample' not in kinds and 'ObjectNoise' not in kinds and 'ObjectNameFilter' in kinds
    assert cfg.runner['max_epochs'] == (40 if name == 'second' else 80) and cfg.data['train']['times'] == 2
