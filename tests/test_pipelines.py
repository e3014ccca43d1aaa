"""GGA train data pipeline: this repo's ObjectSample_GGA /
DataBaseSampler_GGA / BatchSampler / ObjectRangeFilter_GGA / point filters against vectors produced
by the reference's classes (mmdet3d/datasets/pipelines/gga_processing.py) with equal numpy / torch
seeds (tools_dev/make_golden.py::golden_pipeline) - every array of every frame, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import pipelines as P
from gga_amd import synthetic
from gga_amd.box3d import LiDARInstance3DBoxes
from gga_amd.points import LiDARPoints
from oracle import oracle as O

sys.path.insert(0, os.path.join(REPO, 'tools_dev'))
import make_golden as MG  # noqa: E402  (run_pipeline_case / case tables only; no reference access at import)

GOLD = np.load(os.path.join(REPO, 'tests', 'golden', 'pipeline.npz'))


def _make_sampler(db, loader):
    return P.DataBaseSampler_GGA(info_path=db, data_root=None, rate=1.0,
                                 prepare=dict(filter_by_difficulty=[-1],
                                              filter_by_min_points=dict(Car=5, Pedestrian=10, Cyclist=10)),
                                 sample_groups=MG.PIPELINE_GROUPS, classes=synthetic.PIPELINE_CLASSES, points_loader=loader)


@pytest.mark.parametrize('seed,nf', MG.PIPELINE_CASES)
def test_pipeline_matches_reference(seed, nf):
    res = MG.run_pipeline_case(seed, nf, LiDARPoints, LiDARInstance3DBoxes, _make_sampler,
                               lambda s: P.ObjectSample_GGA(min_distance=5.0, db_sampler=s), P.ObjectRangeFilter_GGA)
    n_sampled = 0
    for f, o in enumerate(res):
        for k, got in o.items():
            want = GOLD[f'{seed}.{f}.{k}']
            got = np.asarray(got)
            assert got.shape == want.shape, (seed, f, k, got.shape, want.shape)
            assert got.dtype == want.dtype, (seed, f, k, got.dtype, want.dtype)
            assert np.array_equal(got, want), (seed, f, k)
        n_sampled += int(o['n_obj_after_sample'])
    assert n_sampled > 50


def test_collision_free_rule():
    anchors = np.array([[0.0, 0.0], [20.0, 0.0]])
    cand = np.array([[3.0, 0.0],      # 3 m from anchor 0                        -> dropped
                     [10.0, 0.0],     # 3 m from the LATER candidate 2            -> dropped (not yet visited counts)
                     [13.0, 0.0],     # its only conflict (candidate 1) is gone   -> kept
                     [6.5, 0.0],      # conflicts (candidates 0, 1) are gone      -> kept
                     [40.0, 0.0],     # 4.999 m from the later candidate 5        -> dropped
                     [40.0, 4.999]])  # its conflict is gone                      -> kept
    assert P.collision_free(anchors, cand, 5.0).tolist() == [False, False, True, True, False, True]
    assert P.collision_free(anchors, np.array([[30.0, 0.0], [35.0, 0.0]]), 5.0).tolist() == [True, True]   # exactly 5 m: not < 5
    assert P.collision_free(np.zeros((0, 2)), np.zeros((0, 2)), 5.0).tolist() == []


def test_batch_sampler_wraps_and_reshuffles():
    np.random.seed(3)
    s = P.BatchSampler(list(range(10)), 'x', shuffle=True)
    first = s.sample(4) + s.sample(4)
    tail = s.sample(4)                 # only 2 left: handed out short, then a new shuffled pass starts
    assert len(tail) == 2 and sorted(first + tail) == list(range(10))
    assert len(s.sample(3)) == 3


def test_points_range_filter_and_shuffle_modules():
    raw = synthetic.make_pipeline_frame(7)
    rng = [0, -40, -3, 70.4, 40, 1]
    d = dict(points=LiDARPoints(raw['points'], points_dim=4))
    d = P.PointsRangeFilter(rng)(d)
    t = d['points'].tensor
    r = np.array(rng, np.float32)
    assert bool(((t[:, 0] > r[0]) & (t[:, 0] < r[3]) & (t[:, 1] > r[1]) & (t[:, 1] < r[4]) & (t[:, 2] > r[2]) & (t[:, 2] < r[5])).all())
    assert len(t) < len(raw['points'])          # the points placed exactly on the faces are rejected (strict)
    before = t.clone()
    torch.manual_seed(5)
    d = P.PointShuffle()(d)
    torch.manual_seed(5)
    assert torch.equal(d['points'].tensor, before[torch.randperm(len(before))])


def test_compose_and_formatting():
    db, db_pts = synthetic.make_gt_database(9)
    loader = lambda res: dict(points=LiDARPoints(db_pts[res['pts_filename']], points_dim=4))
    np.random.seed(1); torch.manual_seed(1)
    pipe = P.Compose([
        P.ObjectSample_GGA(min_distance=5.0, db_sampler=_make_sampler(db, loader)),
        dict(type='PointsRangeFilter', point_cloud_range=[0, -40, -3, 70.4, 40, 1]),
        dict(type='ObjectRangeFilter_GGA', point_cloud_range=[0, -40, -3, 70.4, 40, 1], num_points_range=15),
        dict(type='PointShuffle'),
        dict(type='DefaultFormatBundle3D_GGA', class_names=synthetic.PIPELINE_CLASSES),
        dict(type='Collect3D_GGA', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d', 'GGA_boxes_img', 'GGA_lidar2img',
                                         'GGA_init_pseudo_labels', 'GGA_bdry_masks', 'GGA_in_box_points'])])
    raw = synthetic.make_pipeline_frame(11)
    out = pipe(dict(raw, points=LiDARPoints(raw['points'], points_dim=4), gt_bboxes_3d=LiDARInstance3DBoxes(raw['gt_bboxes_3d']),
                    sample_idx=11, pts_filename='x.bin'))
    assert set(out) == {'img_metas', 'points', 'gt_bboxes_3d', 'gt_labels_3d', 'GGA_boxes_img', 'GGA_lidar2img',
                        'GGA_init_pseudo_labels', 'GGA_bdry_masks', 'GGA_in_box_points'}
    n = len(out['gt_labels_3d'].data)
    assert out['points'].data.dtype == torch.float32 and out['points'].data.shape[1] == 4
    assert isinstance(out['gt_bboxes_3d'].data, LiDARInstance3DBoxes) and out['gt_bboxes_3d'].cpu_only
    assert len(out['gt_bboxes_3d'].data) == n == len(out['GGA_in_box_points'].data) == len(out['GGA_boxes_img'].data)
    assert out['GGA_lidar2img'].data.shape == (n, 4, 4) and out['GGA_init_pseudo_labels'].data.dtype == torch.float64
    assert out['img_metas'].data == dict(sample_idx=11, pts_filename='x.bin')
    yaw = out['gt_bboxes_3d'].data.tensor[:, 6]
    assert bool(((yaw >= -np.pi) & (yaw < np.pi)).all())


# ----------------------------------------------------------------------------- device tail
def _deferred_frames(seed, nf):
    """The repo's pipeline with defer_points=True: what DevicePointPrep receives, frame by frame."""
    db, db_pts = synthetic.make_gt_database(seed)
    loader = lambda res: dict(points=LiDARPoints(db_pts[res['pts_filename']], points_dim=4))
    np.random.seed(seed)
    torch.manual_seed(seed)
    osample = P.ObjectSample_GGA(min_distance=5.0, db_sampler=_make_sampler(db, loader), defer_points=True)
    rfilt = P.PointsRangeFilter(MG.PIPELINE_RANGE, defer_points=True)
    frames = []
    for f in range(nf):
        raw = synthetic.make_pipeline_frame(1000 * seed + f)
        d = dict(raw, points=LiDARPoints(raw['points'], points_dim=4), gt_bboxes_3d=LiDARInstance3DBoxes(raw['gt_bboxes_3d']))
        frames.append(rfilt(osample(d)))
    return frames


@pytest.mark.parametrize('seed,nf', MG.PIPELINE_CASES)
def test_oracle_point_tail_matches_reference(seed, nf):
    # the C restatement of remove-near-centres + cat + range filter == the reference's points, row for row
    for f, d in enumerate(_deferred_frames(seed, nf)):
        samp = d['sampled_points'].tensor.numpy() if 'sampled_points' in d else np.zeros((0, 4), np.float32)
        got = O.points_prepare(d['points'].tensor.numpy(), samp, d.get('sampled_centers', np.zeros((0, 2))), 5.0,
                               MG.PIPELINE_RANGE)
        assert np.array_equal(got, GOLD[f'{seed}.{f}.points_after_range']), (seed, f)


def _boundary_case():
    """Distances exactly at / one ulp around min_distance, points on the range faces."""
    c = np.array([[30.0, 0.0]])
    xs = np.array([35.0, np.nextafter(np.float32(35.0), np.float32(0)), np.nextafter(np.float32(35.0), np.float32(99)),
                   33.0, 34.0, 30.0, 25.0, np.nextafter(np.float32(25.0), np.float32(99))], np.float32)
    pts = np.stack([xs, np.zeros_like(xs), np.full_like(xs, -1.0), np.ones_like(xs)], 1)
    pts = np.concatenate([pts, np.array([[33.0, 4.0, -1, 1], [27.0, -4.0, -1, 1], [33.0, np.nextafter(np.float32(4.0), np.float32(9)), -1, 1],
                                         [0.0, 0, -1, 1], [70.4, 0, -1, 1], [1, -40, -1, 1], [1, 40, -1, 1], [1, 0, -3, 1], [1, 0, 1, 1]],
                                        np.float32)])
    return pts, np.zeros((0, 4), np.float32), c


def test_oracle_point_tail_boundaries():
    pts, samp, c = _boundary_case()
    got = O.points_prepare(pts, samp, c, 5.0, MG.PIPELINE_RANGE)
    keep_x = {float(v) for v in got[:, 0]}
    assert 35.0 in keep_x and 25.0 in keep_x                     # distance exactly 5.0 is NOT < 5.0
    assert float(np.nextafter(np.float32(35.0), np.float32(0))) not in keep_x
    # kept: 35, 35+ulp, 25, the two exact 3-4-5 points and (33, 4+ulp); 25+ulp, 33, 34, 30 are inside 5 m
    assert len(got) == 6
    assert not any(v in keep_x for v in (0.0, 1.0)) and not np.any(got[:, 0] > 70.0)   # points on the range faces (strict) are out



@pytest.mark.gpu
@pytest.mark.parametrize('seed,nf', MG.PIPELINE_CASES)
def test_device_point_tail_matches_reference(seed, nf):
    from gga_amd import functional as F
    frames = _deferred_frames(seed, nf)
    prep = P.DevicePointPrep(min_distance=5.0)(frames)            # seeds absent -> order kept
    got = prep.to_list()
    for f in range(nf):
        assert np.array_equal(got[f].cpu().numpy(), GOLD[f'{seed}.{f}.points_after_range']), (seed, f)
    # shuffled: same rows, a different order, reproducible per seed
    for f, d in enumerate(frames):
        d['deferred_shuffle_seed'] = 1234567 + f
    a = P.DevicePointPrep(5.0)(frames).to_list()
    b = P.DevicePointPrep(5.0)(frames).to_list()
    for f, d in enumerate(frames):
        d['deferred_shuffle_seed'] = 7654321 + f
    c = P.DevicePointPrep(5.0)(frames).to_list()
    srt = lambda t: t[np.lexsort(t.T[::-1])]
    for f in range(nf):
        x, y, z, g = a[f].cpu().numpy(), b[f].cpu().numpy(), c[f].cpu().numpy(), got[f].cpu().numpy()
        assert np.array_equal(x, y) and x.shape == g.shape == z.shape
        assert np.array_equal(srt(x), srt(g)) and np.array_equal(srt(z), srt(g))       # permutations of the kept rows
        assert not np.array_equal(x, g) and not np.array_equal(x, z)
        moved = np.mean(np.any(x != g, axis=1))
        assert moved > 0.9                                                              # not a near-identity permutation


@pytest.mark.gpu
def test_device_point_tail_boundaries_and_voxelizer_handover():
    from gga_amd import functional as F
    pts, samp, c = _boundary_case()
    rng = MG.PIPELINE_RANGE
    # frame 0: boundary case; frame 1: empty scene + pasted points only; frame 2: plain frame, nothing pasted
    raw = synthetic.make_pipeline_frame(77, n_points=20000)['points']
    scene = [torch.from_numpy(pts), torch.zeros((0, 4)), torch.from_numpy(raw)]
    sampled = [torch.zeros((0, 4)), torch.tensor([[10.0, 0, -1, 0.5], [100.0, 0, -1, 0.5]]), torch.zeros((0, 4))]
    centers = [c, np.array([[10.0, 0.0]]), np.zeros((0, 2))]
    prep = F.points_prepare_batch(scene, sampled, centers, 5.0, rng, [0, 0, 0], 'cuda:0')
    got = prep.to_list()
    for f in range(3):
        want = O.points_prepare(scene[f].numpy(), sampled[f].numpy(), centers[f], 5.0, rng)
        assert np.array_equal(got[f].cpu().numpy(), want), f
    assert len(got[1]) == 1                                       # pasted points are range-filtered but never removed
    # voxelizer hand-over without a host round trip == voxelizing the materialised frames
    vs, mp, mv = [0.05, 0.05, 0.1], 5, 16000
    a = F.hard_voxelize_prepared(prep, vs, rng, mp, mv)
    b = F.hard_voxelize_batch([g.contiguous() for g in got], vs, rng, mp, mv)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[3][-1]) > 1000


@pytest.mark.gpu
def test_device_point_tail_scan_carries_across_rounds():
    """262 145 virtual rows = 1025 chunks of 256: pp_scan_kernel (1024 chunk counts per round) needs a second round, so its
    carry is live - rows and count bit for bit against the C oracle; then the same frame followed by an empty one."""
    from gga_amd import functional as F
    rng, g = MG.PIPELINE_RANGE, np.random.default_rng(262145)
    margin = np.array([2, 2, 0.25], np.float32)
    lo, hi = np.array(rng[:3], np.float32) - margin, np.array(rng[3:], np.float32) + margin
    n_samp = 145
    n_scene = 1024 * 256 + 1 - n_samp
    scene = np.concatenate([g.uniform(lo, hi, (n_scene, 3)), g.uniform(0, 1, (n_scene, 1))], 1).astype(np.float32)
    scene[-1, :3] = [40.0, 30.0, -1.0]                           # the one row of chunk 1024: in range, far from the centres
    samp = np.concatenate([g.uniform(lo, hi, (n_samp, 3)), g.uniform(0, 1, (n_samp, 1))], 1).astype(np.float32)
    ctr = np.array([[20.0, 5.0], [50.0, -20.0], [8.0, -3.0]])
    want = O.points_prepare(scene, samp, ctr, 5.0, rng)
    assert 0.5 * n_scene < len(want) < n_scene and np.array_equal(want[-1], scene[-1])
    none4 = torch.zeros((0, 4))
    prep = F.points_prepare_batch([torch.from_numpy(scene)], [torch.from_numpy(samp)], [ctr], 5.0, rng, [0], 'cuda:0')
    assert prep.counts.cpu().tolist() == [len(want)]
    assert np.array_equal(prep.to_list()[0].cpu().numpy(), want)
    prep = F.points_prepare_batch([torch.from_numpy(scene), none4], [torch.from_numpy(samp), none4], [ctr, np.zeros((0, 2))], 5.0,
                                  rng, [0, 0], 'cuda:0')
    assert prep.counts.cpu().tolist() == [len(want), 0]
    got = prep.to_list()
    assert np.array_equal(got[0].cpu().numpy(), want) and got[1].shape == (0, 4)
