"""The image branch on the host: the coco converter (``gga_amd.kitti_converter_mono``), ``KittiMonoDataset``
(``gga_amd.kitti_mono``), the image pipeline (``gga_amd.image_pipelines``, ``RandomFlip3D``, ``LoadAnnotations3D``) and the
resize definition.

* The converter's 2D boxes are held to an independent float64 restatement kept here: the extent of (convex hull of the
  projected in-front corners) intersected with the canvas as four linear programs over ``scipy.spatial.ConvexHull``'s facet
  equations plus the canvas bounds. shapely / nuscenes are absent, so there is no golden of the reference's converter.
* The dataset is held to vectors of the reference's own method bodies (tests/golden/kitti_mono.npz,
  tools_dev/make_golden.py::golden_kitti_mono).
* The pipeline: hand-computed expectations for a resized, flipped frame, and the device-deferred record materialised on the
  host equals the eager host result bit for bit."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import Config, synthetic
from gga_amd import image_pipelines as IP
from gga_amd import kitti_converter_mono as KC
from gga_amd import loader as LD
from gga_amd.kitti_mono import KittiMonoDataset

GOLDEN = os.path.join(REPO, 'tests', 'golden')
CLASSES = ('Pedestrian', 'Cyclist', 'Car')
P2 = synthetic.KITTI_CALIB['P2']


# ------------------------------------------------------------------------------------------------------------ converter
def hull_canvas_extent(points, canvas=(1600, 900)):
    """min / max of x and y over hull(points) intersected with the canvas, by linear programming; None when empty."""
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(points, np.float64)).equations            # a x + b y + c <= 0 inside
    bounds = [(0, canvas[0]), (0, canvas[1])]
    out = []
    for cost in ([1, 0], [0, 1], [-1, 0], [0, -1]):
        res = linprog(cost, A_ub=eq[:, :2], b_ub=-eq[:, 2], bounds=bounds, method='highs')
        if res.status == 2:
            return None
        assert res.status == 0, res.message
        out.append(res.fun)
    return out[0], out[1], -out[2], -out[3]


def _info(objects, image_idx=3, names=None):
    """An info dict with the given camera-frame objects (x, y_bottom, z, l, h, w, ry)."""
    o = np.asarray(objects, np.float64).reshape(-1, 7)
    n = len(o)
    p0 = P2.copy()
    p0[:3, 3] = 0.0
    return dict(image=dict(image_idx=image_idx, image_path=f'training/image_2/{image_idx:06d}.png', image_shape=np.array([375, 1242], np.int32)),
                calib=dict(P0=p0, P2=P2.copy(), R0_rect=np.eye(4), Tr_velo_to_cam=np.eye(4), Tr_imu_to_velo=np.eye(4)),
                annos=dict(name=np.array(names if names is not None else ['Car'] * n), occluded=np.zeros(n, np.int64), location=o[:, :3],
                           dimensions=o[:, 3:6], rotation_y=o[:, 6]))


def _projected_front_corners(obj):
    loc = np.array(obj[:3]) + np.array(obj[3:6]) * np.array([0.0, -0.5, 0.0])
    box = np.concatenate([loc, obj[3:6], obj[6:7]]).astype(np.float32)
    corners = KC._corners(box[:3], box[3:6], box[6]).T.astype(np.float64)
    corners = corners[:, corners[2] > 0]
    return KC.view_points(corners, P2, True).T[:, :2], corners.shape[1]


CONVERTER_CASES = {            # (x, y_bottom, z, l, h, w, ry) -> number of corners in front of the camera
    'inside': ([1.0, 1.6, 20.0, 3.9, 1.56, 1.6, 0.3], 8),
    'inside_far': ([-6.0, 1.7, 45.0, 0.8, 1.73, 0.6, -1.2], 8),
    'left_edge': ([-9.5, 1.6, 12.0, 3.9, 1.56, 1.6, 0.1], 8),
    'right_edge': ([16.5, 1.6, 12.0, 3.9, 1.56, 1.6, 1.4], 8),
    'top_edge': ([0.5, -1.0, 8.0, 3.9, 1.56, 1.6, 0.7], 8),
    'bottom_edge': ([0.5, 10.8, 10.0, 3.9, 1.56, 1.6, 0.7], 8),
    'straddles_4': ([0.3, 1.0, 0.02, 3.9, 1.56, 1.6, 0.0], 4),
    'straddles_6': ([0.9, 1.0, 1.2, 3.9, 1.56, 1.6, 0.785398], 6),
}


@pytest.mark.parametrize('case', sorted(CONVERTER_CASES))
def test_converter_boxes_against_linear_programs(case):
    obj, n_front = CONVERTER_CASES[case]
    pts, n = _projected_front_corners(np.array(obj))
    assert n == n_front, (case, n)
    want = hull_canvas_extent(pts)
    recs = KC.get_2d_boxes(_info([obj]), occluded=[0, 1, 2, 3])
    assert want is not None and len(recs) == 1
    x, y, w, h = recs[0]['bbox']
    got = np.array([x, y, x + w, y + h])
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * 1600), (case, got, want)
    assert 0 <= got[0] < got[2] <= 1600 and 0 <= got[1] < got[3] <= 900
    if case.endswith('_edge'):          # the box crosses that edge of the canvas: the extent ends on it
        k, bound = dict(left_edge=(0, 0), top_edge=(1, 0), right_edge=(2, 1600), bottom_edge=(3, 900))[case]
        assert got[k] == bound and abs(want[k] - bound) < 1e-9
    assert np.isclose(recs[0]['area'], w * h)
    # the 3D part: gravity centre, the P2 - P0 offset on x only in bbox_cam3d, the projected unshifted centre with its depth
    centre = np.array(obj[:3]) - [0, obj[4] / 2, 0]
    offset = (P2[0, 3] - 0.0) / P2[0, 0]
    assert np.allclose(recs[0]['bbox_cam3d'], np.concatenate([centre + [offset, 0, 0], obj[3:]]).astype(np.float32))
    q = P2 @ np.append(centre, 1.0)
    assert np.allclose(recs[0]['center2d'], [q[0] / q[2], q[1] / q[2], q[2]], rtol=1e-12)
    assert recs[0]['velo_cam3d'] == recs[0]['attribute_name'] == recs[0]['attribute_id'] == -1
    assert recs[0]['category_id'] == 2 and recs[0]['iscrowd'] == 0


def test_converter_drops_what_the_reference_drops():
    behind = [1.0, 1.6, -20.0, 3.9, 1.56, 1.6, 0.3]                # wholly behind the camera: no corner in front
    beyond = [60.0, 1.6, 10.0, 3.9, 1.56, 1.6, 0.3]                # projects to the right of the 1600-wide canvas
    centre_behind = [0.0, 1.0, -0.4, 3.9, 1.56, 1.6, 0.0]          # four corners in front, centre depth <= 0
    for obj in (behind, beyond, centre_behind):
        assert KC.get_2d_boxes(_info([obj]), occluded=[0, 1, 2, 3]) == [], obj
    pts, n = _projected_front_corners(np.array(beyond))
    assert n == 8 and hull_canvas_extent(pts) is None
    pts, n = _projected_front_corners(np.array(centre_behind))
    assert n == 4 and hull_canvas_extent(pts) is not None          # (the 2D box exists: it is the depth test that drops it)
    # the canvas is the reference's default (1600, 900), not the image: a box right of the 1242-wide image is kept
    right_of_image = [12.0, 1.6, 12.0, 0.8, 1.73, 0.6, 0.0]
    rec = KC.get_2d_boxes(_info([right_of_image]), occluded=[0, 1, 2, 3])
    assert len(rec) == 1 and rec[0]['bbox'][0] > 1242
    # unknown categories give None (left out of the file), an occlusion state outside the list drops the object
    assert KC.get_2d_boxes(_info([CONVERTER_CASES['inside'][0]], names=['Van']), occluded=[0, 1, 2, 3]) == [None]
    info = _info([CONVERTER_CASES['inside'][0]])
    info['annos']['occluded'][:] = -1
    assert KC.get_2d_boxes(info, occluded=[0, 1, 2, 3]) == []
    # degenerate hulls are skipped
    assert KC.hull_clip_bounds([[10.0, 10.0], [20.0, 20.0]]) is None and KC.hull_clip_bounds([]) is None
    assert KC.hull_clip_bounds([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]) is None


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('kitti_mono'))
    info_path, test_path = synthetic.write_kitti_mono_tree(root, 6, img_hw=(96, 320))
    return dict(root=root, info=info_path, test=test_path, json=KC.export_2d_annotation(root, info_path),
                json_test=KC.export_2d_annotation(root, test_path))


def test_written_tree_and_coco_files(tree):
    from PIL import Image
    infos, tests = pickle.load(open(tree['info'], 'rb')), pickle.load(open(tree['test'], 'rb'))
    assert len(infos) == len(tests) == 6 and all('annos' not in t for t in tests)
    assert all(list(i['annos']['name']).count('DontCare') == 1 for i in infos)
    shapes = {tuple(i['image']['image_shape']) for i in infos}
    assert len(shapes) > 1 and all(90 <= h <= 96 and 312 <= w <= 320 for h, w in shapes)
    with Image.open(os.path.join(tree['root'], infos[0]['image']['image_path'])) as im:
        assert im.size == (infos[0]['image']['image_shape'][1], infos[0]['image']['image_shape'][0]) and im.mode == 'RGB'
    assert synthetic.write_kitti_mono_tree(tree['root'], 6, img_hw=(96, 320)) == (tree['info'], tree['test'])          # left alone
    assert tree['json'].endswith('kitti_infos_trainval_GGA_pseudo_mono3d.coco.json') and tree['json_test'].endswith('kitti_infos_test_mono3d.coco.json')
    coco, coco_test = json.load(open(tree['json'])), json.load(open(tree['json_test']))
    assert [c['name'] for c in coco['categories']] == list(CLASSES) and [c['id'] for c in coco['categories']] == [0, 1, 2]
    assert [a['id'] for a in coco['annotations']] == list(range(len(coco['annotations']))) and len(coco['annotations']) > 6
    assert all(a['category_name'] in CLASSES and a['category_id'] == CLASSES.index(a['category_name']) for a in coco['annotations'])
    assert len(coco['images']) == 6 and coco_test['annotations'] == [] and len(coco_test['images']) == 6
    for im, info in zip(coco['images'], infos):
        assert (im['height'], im['width']) == tuple(info['image']['image_shape']) and im['id'] == info['image']['image_idx']
        for k in ('Tri2v', 'Trv2c', 'rect', 'cam_intrinsic'):
            assert isinstance(im[k], list) and np.array(im[k]).shape == (4, 4)
    # the infos are not modified by the converter
    again = pickle.load(open(tree['info'], 'rb'))
    KC.get_2d_boxes(again[0], occluded=[0, 1, 2, 3])
    assert all(np.array_equal(again[0]['annos'][k], infos[0]['annos'][k]) for k in infos[0]['annos'])


# -------------------------------------------------------------------------------------------------------------- dataset
@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'kitti_mono.npz'))
    coco = json.loads(str(z['inputs.coco']))
    calib = {k: z[f'inputs.calib.{k}'] for k in ('P2', 'R0_rect', 'Tr_velo_to_cam')}
    infos = [dict(image=dict(image_idx=int(z[f'inputs.{f}.image_idx']), image_shape=z[f'inputs.{f}.image_shape']), calib=calib) for f in range(4)]
    return z, coco, infos


def _same(got, want, exact=True):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if exact or got.dtype.kind not in 'f':
        assert np.array_equal(got, want)
    else:
        assert np.allclose(got, want, rtol=1e-6, atol=1e-6)


def test_parse_ann_info_against_the_reference(golden):
    z, coco, infos = golden
    ds = KittiMonoDataset('/nonexistent', infos, coco, None, classes=CLASSES, test_mode=True)
    assert ds.cat_ids == [0, 1, 2] and ds.cat2label == {0: 0, 1: 1, 2: 2} and ds.bbox_code_size == 7 and len(ds) == 4
    assert [d['filename'] for d in ds.data_infos] == [d['file_name'] for d in ds.data_infos]
    counts = []
    for f in range(4):
        a = ds.get_ann_info(f)
        for k in ('bboxes', 'labels', 'gt_labels_3d', 'centers2d', 'depths', 'bboxes_ignore'):
            _same(a[k], z[f'parse.{f}.{k}'])
        _same(a['gt_bboxes_3d'].tensor.numpy(), z[f'parse.{f}.gt_bboxes_3d'])
        assert a['seg_map'] == str(z[f'parse.{f}.seg_map']) and len(a['masks']) == int(z[f'parse.{f}.n_masks'])
        counts.append(len(a['bboxes']))
    assert counts[1] == counts[2] == 0 and min(counts[0], counts[3]) > 2          # the empty frames have the empty shapes / dtypes
    assert len(ds.get_ann_info(0)['bboxes_ignore']) == 1


def test_result_formatting_against_the_reference(golden, tmp_path):
    from gga_amd.box3d import CameraInstance3DBoxes
    z, coco, infos = golden
    ds = KittiMonoDataset('/nonexistent', infos, coco, None, classes=CLASSES, test_mode=True)
    outs = [dict(boxes_3d=CameraInstance3DBoxes(torch.from_numpy(z[f'inputs.{f}.boxes'].copy())), scores_3d=torch.from_numpy(z[f'inputs.{f}.scores'].copy()),
                 labels_3d=torch.from_numpy(z[f'inputs.{f}.labels'].copy())) for f in range(4)]
    for f in range(4):
        conv = ds.convert_valid_bboxes(copy.deepcopy(outs[f]), infos[f])
        assert sorted(conv) == list(z[f'convert.{f}.keys'])
        for k, v in conv.items():
            _same(v, z[f'convert.{f}.{k}'], exact=k != 'box3d_lidar')
    annos = ds.bbox2result_kitti(copy.deepcopy(outs), CLASSES, pklfile_prefix=str(tmp_path / 'res'), submission_prefix=str(tmp_path / 'sub'))
    assert [len(a['score']) for a in annos] == [len(z[f'anno.{f}.score']) for f in range(4)] and len(annos[1]['score']) == len(annos[2]['score']) == 0
    for f, anno in enumerate(annos):
        assert set(anno) == {k.split('.', 2)[2] for k in z.files if k.startswith(f'anno.{f}.')}
        for k, v in anno.items():
            want = z[f'anno.{f}.{k}']
            if k == 'name':
                assert list(v) == list(want)
            else:
                _same(v, want, exact=k != 'alpha')
        assert open(tmp_path / 'sub' / f'{int(z[f"inputs.{f}.image_idx"]):06d}.txt').read() == str(z[f'submission.{f}'])
    assert [len(a['score']) for a in pickle.load(open(tmp_path / 'res.pkl', 'rb'))] == [len(a['score']) for a in annos]
    # 2D results: per class arrays [n, 5]
    two_d = [[np.array([[1.0, 2.0, 30.0, 40.0, 0.9]], np.float32), np.zeros((0, 5), np.float32), np.array([[5.0, 6.0, 7.0, 8.0, 0.5]] * 2, np.float32)]] + \
            [[np.zeros((0, 5), np.float32)] * 3] * 3
    res, _ = ds.format_results([dict(img_bbox=o, img_bbox2d=t) for o, t in zip(copy.deepcopy(outs), two_d)], submission_prefix=str(tmp_path / 's_'))
    assert set(res) == {'img_bbox', 'img_bbox2d'} and list(res['img_bbox2d'][0]['name']) == ['Pedestrian', 'Car', 'Car']
    assert (res['img_bbox2d'][0]['alpha'] == -10).all() and (res['img_bbox2d'][0]['location'] == -1000).all() and len(res['img_bbox2d'][1]['score']) == 0
    assert len(os.listdir(str(tmp_path / 's_img_bbox2d'))) == 4 and len(os.listdir(str(tmp_path / 's_img_bbox'))) == 4


def test_filter_group_flags_and_retry(tree):
    coco = json.load(open(tree['json']))
    coco['images'][1].update(width=31)                                               # too small
    coco['annotations'] = [a for a in coco['annotations'] if a['image_id'] != 2]     # no annotation
    for a in coco['annotations']:
        if a['image_id'] == 3:
            a['category_id'] = 9                                                     # only annotations of an unknown category
    coco['images'][4].update(width=50, height=80)                                    # taller than wide
    coco['images'] = coco['images'][::-1]                                            # (order in the file does not matter)
    infos = pickle.load(open(tree['info'], 'rb'))
    ds = KittiMonoDataset(tree['root'], infos, coco, None, classes=CLASSES, img_prefix=tree['root'])
    assert [d['id'] for d in ds.data_infos] == ds.img_ids == [0, 4, 5] and ds.flag.tolist() == [1, 0, 1] and ds.flag.dtype == np.uint8
    test = KittiMonoDataset(tree['root'], infos, coco, None, classes=CLASSES, test_mode=True)
    assert [d['id'] for d in test.data_infos] == [0, 1, 2, 3, 4, 5] and not hasattr(test, 'flag')
    keep_all = KittiMonoDataset(tree['root'], infos, coco, None, classes=CLASSES, filter_empty_gt=False)
    assert [d['id'] for d in keep_all.data_infos] == [0, 2, 3, 4, 5]
    # a pipeline that gives None: another index of the SAME group is drawn until one works
    seen = []

    def pipeline(results):
        seen.append(results['img_info']['id'])
        return None if results['img_info']['id'] == 0 else results
    ds.pipeline = pipeline
    np.random.seed(0)
    out = ds[0]
    assert seen[0] == 0 and seen[-1] == 5 and set(seen) <= {0, 5} and out['img_info']['id'] == 5
    assert out['img_prefix'] == tree['root'] and out['bbox_fields'] == [] and out['box_type_3d'].__name__ == 'CameraInstance3DBoxes'
    assert out['box_mode_3d'] == 1 and set(out['ann_info']) >= {'bboxes', 'labels', 'gt_bboxes_3d', 'centers2d', 'depths'}


def test_config_data_section_equals_the_reference():
    mine = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg.py'))
    ref = json.load(open(os.path.join(GOLDEN, 'reference_configs.json')))['configs/gga/gga_pdg.py']['data']
    assert json.loads(json.dumps(dict(mine.data))) == ref


# ------------------------------------------------------------------------------------------------------------- pipeline
def _cfg(tree):
    cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', 'gga_pdg.py'))
    for split in ('train', 'val', 'test'):
        cfg.data[split].update(data_root=tree['root'] + '/', img_prefix=tree['root'] + '/', ann_file=tree['json_test' if split == 'test' else 'json'],
                               info_file=tree['test' if split == 'test' else 'info'])
    return cfg


def _unwrap(v):
    return v.data if isinstance(v, LD.DataContainer) else v


@pytest.mark.parametrize('flip', [True, False])
def test_train_pipeline_of_one_frame_by_hand(tree, monkeypatch, flip):
    """Frame 0 through the config's train pipeline with the flip decided: every key against arithmetic done here."""
    monkeypatch.setenv('GGA_MONO_IMAGE_DEVICE', '0')
    cfg = _cfg(tree)
    ds = LD.build_dataset(copy.deepcopy(cfg.data['train']))
    raw = ds.get_ann_info(0)
    info = ds.data_infos[0]
    h, w = info['height'], info['width']
    monkeypatch.setattr(np.random, 'choice', lambda a, p=None: (a[0] if flip else a[1]))
    sample = ds[0]
    meta = _unwrap(sample['img_metas'])
    s = min(1242 / max(h, w), 375 / min(h, w))
    new_w, new_h = int(w * s + 0.5), int(h * s + 0.5)
    assert meta['img_shape'] == (new_h, new_w, 3) and meta['ori_shape'] == (h, w, 3) and meta['flip'] is flip
    assert meta['pad_shape'] == (-(-new_h // 32) * 32, -(-new_w // 32) * 32, 3)
    sf = np.array([new_w / w, new_h / h, new_w / w, new_h / h], np.float32)
    assert meta['scale_factor'].dtype == np.float32 and np.array_equal(meta['scale_factor'], sf)
    boxes = raw['bboxes'] * sf
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, new_w)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, new_h)
    cam = raw['gt_bboxes_3d'].tensor.clone()
    c2d = raw['centers2d'].copy()
    cu = info['cam_intrinsic'][0][2]
    if flip:
        boxes = np.stack([new_w - boxes[:, 2], boxes[:, 1], new_w - boxes[:, 0], boxes[:, 3]], 1)
        cam[:, 0] = -cam[:, 0]
        cam[:, 6] = -cam[:, 6] + np.pi
        c2d[:, 0] = w - c2d[:, 0]                     # the ORIGINAL width, as the reference has it
        cu = w - cu
    assert np.array_equal(_unwrap(sample['gt_bboxes']).numpy(), boxes) and _unwrap(sample['gt_bboxes']).dtype == torch.float32
    assert torch.equal(_unwrap(sample['gt_bboxes_3d']).tensor, cam)
    assert np.array_equal(_unwrap(sample['centers2d']).numpy(), c2d)          # (not resized: mmdet's Resize does not know them)
    assert np.array_equal(_unwrap(sample['depths']).numpy(), raw['depths']) and np.array_equal(_unwrap(sample['gt_labels']).numpy(), raw['labels'])
    assert meta['cam2img'][0][2] == cu and ds.data_infos[0]['cam_intrinsic'][0][2] == info['cam_intrinsic'][0][2]
    assert set(meta) >= {'filename', 'ori_shape', 'img_shape', 'cam2img', 'pad_shape', 'scale_factor', 'flip', 'pcd_horizontal_flip',
                         'pcd_vertical_flip', 'box_mode_3d', 'box_type_3d', 'img_norm_cfg', 'transformation_3d_flow'}
    # the pixels: BGR from the file, resized by the definition, mirrored, mean-subtracted, padded with zeros
    from PIL import Image
    bgr = np.asarray(Image.open(meta['filename']).convert('RGB'))[..., ::-1]
    want = IP.resize_bilinear(np.ascontiguousarray(bgr), new_h, new_w)
    want = (want[:, ::-1] if flip else want).astype(np.float32) - np.array([103.530, 116.280, 123.675], np.float32)
    img = _unwrap(sample['img'])
    assert img.dtype == torch.float32 and tuple(img.shape) == (3,) + meta['pad_shape'][:2]
    assert np.array_equal(img[:, :new_h, :new_w].numpy(), want.transpose(2, 0, 1))
    assert (img[:, new_h:] == 0).all() and (img[:, :, new_w:] == 0).all()


def test_deferred_record_equals_the_eager_host_result(tree, monkeypatch):
    cfg = _cfg(tree)

    def batches(mode, split, n):
        monkeypatch.setenv('GGA_MONO_IMAGE_DEVICE', mode)
        ds = LD.build_dataset(copy.deepcopy(cfg.data[split]))
        np.random.seed(3)
        samples = [ds[i] for i in range(n)]
        return samples, LD.to_step_inputs(LD.collate(samples, n, packed=True))
    for split, n in (('train', 4), ('val', 3)):
        s1, on = batches('1', split, n)
        s0, off = batches('0', split, n)
        first = s1[0]['img'][0] if split == 'val' else s1[0]['img']
        assert isinstance(_unwrap(first), IP.DeferredImage) and _unwrap(first).src.dtype == np.uint8
        img_on, img_off = (on['img'][0], off['img'][0]) if split == 'val' else (on['img'], off['img'])
        assert img_on.dtype == torch.float32 and img_on.shape == img_off.shape and img_on.shape[0] == n
        assert torch.equal(img_on.view(torch.int32), img_off.view(torch.int32))
        metas_on, metas_off = (on['img_metas'][0], off['img_metas'][0]) if split == 'val' else (on['img_metas'], off['img_metas'])
        for a, b in zip(metas_on, metas_off):
            assert a['img_shape'] == b['img_shape'] and a['pad_shape'] == b['pad_shape'] and a['flip'] == b['flip']
            assert np.array_equal(a['scale_factor'], b['scale_factor'])
        if split == 'train':
            assert any(m['flip'] for m in metas_on) and not all(m['flip'] for m in metas_on)
            for k in ('gt_bboxes', 'centers2d', 'depths', 'gt_labels', 'gt_labels_3d'):
                assert all(torch.equal(a, b) for a, b in zip(on[k], off[k]))
        else:
            assert metas_on[0]['scale_factor'] == 1.0 and metas_on[0]['flip'] is False and img_on.shape[2] == 96 and img_on.shape[3] == 320
    # what crosses the process boundary for a batch: one uint8 buffer
    monkeypatch.setenv('GGA_MONO_IMAGE_DEVICE', '1')
    ds = LD.build_dataset(copy.deepcopy(cfg.data['train']))
    packed = LD.collate([ds[i] for i in range(3)], 3, packed=True)['img'].data[0]
    assert isinstance(packed, IP.PackedImages) and packed.buffer.dtype == torch.uint8 and len(packed) == 3
    assert packed.buffer.numel() < 3072 + 3 * (96 * 320 * 3 + 16)
    assert len(pickle.loads(pickle.dumps(packed)).images()) == 3


def test_pipeline_argument_combinations_that_are_not_built_raise():
    for bad in (dict(img_scale=(100, 50), keep_ratio=False), dict(img_scale=[(100, 50), (200, 100)]), dict(img_scale=(100, 50), ratio_range=(0.5, 1.5))):
        with pytest.raises(NotImplementedError):
            IP.Resize(**bad)
    with pytest.raises(NotImplementedError):
        IP.Pad(size=(10, 10))
    with pytest.raises(NotImplementedError):
        IP.MultiScaleFlipAug(transforms=[], scale_factor=1.0, flip=True)


# ---------------------------------------------------------------------------------------------------- resize definition
def _bilinear64(img, dst_h, dst_w):
    """float64 bilinear with half-pixel centres and edge replication."""
    def taps(dst, src):
        f = (np.arange(dst) + 0.5) * src / dst - 0.5
        i0 = np.floor(f)
        return np.clip(i0, 0, src - 1).astype(int), np.clip(i0 + 1, 0, src - 1).astype(int), f - i0
    y0, y1, wy = taps(dst_h, img.shape[0])
    x0, x1, wx = taps(dst_w, img.shape[1])
    p = img.astype(np.float64)
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = (1 - wx) * p[y0][:, x0] + wx * p[y0][:, x1]
    bot = (1 - wx) * p[y1][:, x0] + wx * p[y1][:, x1]
    return (1 - wy) * top + wy * bot


@pytest.mark.parametrize('src,dst', [((37, 53), (37, 53)), ((37, 53), (30, 42)), ((37, 53), (38, 54)), ((96, 320), (375, 1242)),
                                     ((40, 64), (17, 200)), ((1, 700), (1, 709)), ((5, 1), (9, 3))])
def test_resize_definition(src, dst):
    """Identity at dst == src; everywhere within one grey level of float64 bilinear: the two weights are quantised to 1 / 2048
    (error of the weighted mean <= 255 * (2 * 2^-12 + 2^-24) < 0.13) and the result is rounded (<= 0.5), so the integer result is
    within 0.63 of the real one and an image rounded from the real one differs by at most one level."""
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    out = IP.resize_bilinear(img, *dst)
    assert out.dtype == np.uint8 and out.shape == dst + (3,)
    if src == dst:
        assert np.array_equal(out, img)
    exact = _bilinear64(img, *dst)
    assert np.abs(out.astype(np.float64) - exact).max() <= 0.63
    assert np.abs(out.astype(np.int64) - np.rint(exact).astype(np.int64)).max() <= 1
    # the taps are what the kernel computes: q = round(fx * 2048) in integers
    i0, i1, w1 = IP.resize_taps(dst[1], src[1])
    fx = (np.arange(dst[1]) + 0.5) * src[1] / dst[1] - 0.5
    q = np.floor(fx * 2048 + 0.5).astype(np.int64)
    inner = (q >= 0) & ((q >> 11) < src[1] - 1)
    assert np.array_equal(i0[inner], q[inner] >> 11) and np.array_equal(w1[inner], q[inner] & 2047) and np.array_equal(i1[inner], i0[inner] + 1)
    assert (i0 >= 0).all() and (i1 <= src[1] - 1).all() and (w1[q < 0] == 0).all()


def test_normalize_table_is_the_whole_function():
    mean, std = [103.530, 116.280, 123.675], [57.375, 1.0, 0.017]
    table = IP.normalize_table(mean, std)
    assert table.dtype == np.float32 and table.shape == (3, 256)
    v = np.arange(256, dtype=np.float32)
    for c in range(3):
        assert np.array_equal(table[c], (v - np.float32(mean[c])) * np.float32(1 / np.float64(std[c])))
    img = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    out = IP.Normalize(mean, std, to_rgb=True)(dict(img=img, img_fields=['img']))
    assert np.array_equal(out['img'][..., 0], table[0][img[..., 2]]) and out['img_norm_cfg']['to_rgb'] is True
