"""Step 1 of the recipe without a GPU: the raw-file parsing against a run of the reference's own functions
(tests/golden/kitti_raw.npz, tools_dev/make_golden.py::golden_kitti_raw), the argument validation of
``gga_frame_point_tests``, and the numpy statement of its face test against the C oracle."""
import os
import sys

import numpy as np
import pytest

from _frame_points_ref import face_test
from conftest import REPO
from gga_amd import _lib, synthetic
from gga_amd import kitti_data_utils as DU

sys.path.insert(0, os.path.join(REPO, 'tools_dev'))


@pytest.fixture(scope='module')
def raw_tree(tmp_path_factory):
    from make_golden import KITTI_RAW_TREE
    root = str(tmp_path_factory.mktemp('kitti_raw'))
    return root, synthetic.write_kitti_raw_tree(root, **KITTI_RAW_TREE)


def _same(got, g, prefix):
    """``got`` (dict, array, scalar or string) equals what the golden holds under ``prefix``: keys in order, dtype, shape, bits."""
    if isinstance(got, dict):
        assert list(got) == g[prefix + '.keys'].tolist(), prefix
        for k, v in got.items():
            _same(v, g, f'{prefix}.{k}')
        return
    want = g[prefix]
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (prefix, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), prefix


def test_tree_layout(raw_tree):
    root, ids = raw_tree
    assert ids == dict(train=[0, 2, 3], val=[1, 4], test=[0, 1])
    assert DU._extend_matrix(np.zeros((3, 4))).shape == (4, 4)
    for i in ids['train'] + ids['val']:
        for sub, ext in (('calib', 'txt'), ('image_2', 'png'), ('label_2', 'txt'), ('velodyne', 'bin'), ('planes', 'txt')):
            assert os.path.exists(os.path.join(root, 'training', sub, f'{i:06d}.{ext}'))
        labels = open(os.path.join(root, 'training', 'label_2', f'{i:06d}.txt')).read().splitlines()
        assert labels[-1].startswith('DontCare ') and all(len(line.split(' ')) == 15 for line in labels)
        assert (len(labels) == 1) == (i == 1)             # frame 1: no object lines but its DontCare
        assert len(open(os.path.join(root, 'training', 'calib', f'{i:06d}.txt')).read().splitlines()) == 7
    assert not os.path.exists(os.path.join(root, 'testing', 'label_2'))
    from gga_amd.kitti_converter import _read_imageset_file
    assert _read_imageset_file(os.path.join(root, 'ImageSets', 'val.txt')) == [1, 4]


def test_get_kitti_image_info_matches_reference(golden, raw_tree):
    g = golden('kitti_raw')
    root, ids = raw_tree
    for split in ('train', 'val', 'test'):
        training = split != 'test'
        infos = DU.get_kitti_image_info(root, training=training, label_info=training, velodyne=True, calib=True,
                                        with_plane=training, image_ids=ids[split], relative_path=True, num_worker=2)
        assert [i['image']['image_idx'] for i in infos] == g[f'{split}.ids'].tolist()
        for i, info in zip(ids[split], infos):
            _same(info, g, f'{split}.{i}')
            assert ('annos' in info) == training and ('plane' in info) == training
            for k in ('P0', 'P1', 'P2', 'P3', 'R0_rect', 'Tr_velo_to_cam', 'Tr_imu_to_velo'):
                assert info['calib'][k].shape == (4, 4) and info['calib'][k].dtype == np.float64
            assert info['image']['image_shape'].dtype == np.int32
    a = DU.get_kitti_image_info(root, image_ids=[1], relative_path=True)[0]['annos']      # DontCare only
    assert a['name'].tolist() == ['DontCare'] and a['index'].tolist() == [-1] and a['difficulty'].tolist() == [-1]
    # 3x4 matrices, absolute paths, no image shape
    plain = DU.get_kitti_image_info(root, training=True, calib=True, image_ids=ids['train'][:1], extend_matrix=False,
                                    relative_path=False, with_imageshape=False)[0]
    assert plain['image']['image_path'] == os.path.join(root, 'training', 'image_2', '000000.png')
    plain['image']['image_path'] = os.path.relpath(plain['image']['image_path'], root)
    _same(plain, g, 'plain')
    # a count in place of a list of ids means 0 .. count-1
    assert [i['image']['image_idx'] for i in DU.get_kitti_image_info(root, label_info=False, image_ids=3)] == [0, 1, 2]
    with pytest.raises(ValueError, match='file not exist'):
        DU.get_kitti_image_info(root, image_ids=[99])


def test_label_anno_and_difficulty_match_reference(golden, raw_tree, tmp_path):
    g = golden('kitti_raw')
    root, ids = raw_tree
    label = DU.get_label_path(ids['train'][0], root, relative_path=False)
    anno = DU.get_label_anno(label)
    _same(anno, g, 'label_anno')
    diff = DU.add_difficulty_to_annos(dict(annos=anno))
    assert diff == g['difficulty_return'].tolist() == anno['difficulty'].tolist() and anno['difficulty'].dtype == np.int32
    n = len(anno['name'])
    assert anno['name'][-1] == 'DontCare' and anno['index'].tolist() == list(range(n - 1)) + [-1]
    assert anno['group_ids'].tolist() == list(range(n)) and anno['index'].dtype == anno['group_ids'].dtype == np.int32
    scored = tmp_path / 'scored.txt'
    scored.write_text(''.join(line.rstrip('\n') + ' %.2f\n' % (0.25 * (k + 1)) for k, line in enumerate(open(label))))
    _same(DU.get_label_anno(str(scored)), g, 'label_anno_scored')


# ------------------------------------------------------------------------------------------ gga_frame_point_tests: the ABI
def test_frame_point_tests_validates_without_gpu():
    L = _lib.lib()
    p = 4096                 # a non-null stand-in for a device pointer: nothing here dereferences it
    ws = L.gga_frame_point_tests_workspace_bytes(1000)
    assert ws >= 4 * 4 and L.gga_frame_point_tests_workspace_bytes(-1) == 0
    assert L.gga_frame_point_tests_workspace_bytes((1 << 21) + 1) == 0 < L.gga_frame_point_tests_workspace_bytes(1 << 21)

    def call(n=1000, stride=4, P=3, S=6, reduce_poly=0, points=p, normal=p, d=p, member=p, counts=p, counts_reduced=p, reduced=p,
             n_reduced=p, workspace=p, ws_bytes=ws):
        return L.gga_frame_point_tests(points, n, stride, normal, d, P, S, reduce_poly, member, counts, counts_reduced, reduced,
                                       n_reduced, workspace, ws_bytes, None)

    def refused(rc, status, word):
        msg = L.gga_last_error().decode()
        return rc == status and msg.startswith('gga_frame_point_tests:') and word in msg

    for bad in (dict(stride=2), dict(P=0), dict(P=257), dict(reduce_poly=3), dict(reduce_poly=-2), dict(n=-1), dict(n=(1 << 21) + 1),
                dict(S=0), dict(P=256, S=8), dict(stride=65)):
        assert refused(call(**bad), -1, 'bad sizes'), bad
    for name in ('points', 'normal', 'd', 'member', 'counts', 'counts_reduced', 'reduced', 'n_reduced', 'workspace'):
        assert refused(call(**{name: None}), -1, 'null pointer'), name
    assert refused(call(ws_bytes=ws - 1), -2, 'workspace')
    assert refused(call(ws_bytes=0), -2, 'workspace')
    # N == 0 is fine whatever else is null: nothing is read or written
    assert call(n=0, points=None, member=None, counts=None, counts_reduced=None, reduced=None, n_reduced=None, workspace=None,
                ws_bytes=0) == 0
    assert call(n=0, P=257) == -1           # but the sizes are still checked


def test_numpy_face_test_matches_the_oracle():
    from gga_amd import label_gen as LG
    from oracle import oracle as O
    inside = 0
    for seed in (1, 2):
        pts, boxes = synthetic.make_frustum_case(seed)
        c = synthetic.KITTI_CALIB
        for box in boxes:
            surf = LG.frustum_surfaces(c['R0_rect'], c['Tr_velo_to_cam'], c['P2'], box)
            normal, d = LG.surface_equ_3d(surf[:, :, :3, :])
            want = O.points_in_frustm_indices(pts, c['R0_rect'], c['Tr_velo_to_cam'], c['P2'], box)
            assert np.array_equal(face_test(pts, normal, d), want)
            inside += int(want.sum())
            # float32 points, as a velodyne file holds them, widen exactly
            p32 = pts.astype(np.float32)
            assert np.array_equal(face_test(p32, normal, d), O.points_in_polyhedra(p32[:, :3].astype(np.float64), normal, d))
    assert inside > 1000          # the cases are not all-outside
