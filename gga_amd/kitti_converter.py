"""Step 1 of the recipe from a raw KITTI root - SURVEY.md §8(f) rank 3
(tools/data_converter/kitti_converter_gga.py:32-212, 521-673 of the reference; ``tools/create_data_gga.py kitti``).

The reference fans ``_calculate_rga`` out over a 60-process pool (hours of CPU per dataset,
README.md:159), every worker dumping ``GGA_kitti_scene_<idx>.pkl``, and then merges the per-frame
files in ImageSets order. Here one process drives the device (``label_gen.calculate_rga``: a frame
is a handful of launches), with the same on-disk protocol: per-frame pickles (so an interrupted
run resumes), merged ``<prefix>_infos_<split>_GGA.pkl``. The stock info dicts come from
``kitti_data_utils.get_kitti_image_info``.

* ``create_kitti_info_file`` - the four splits in the reference's order (train, val, trainval, test).
* ``create_reduced_point_cloud`` - ``<split>/velodyne_reduced/*.bin``, the points inside the image frustum.
* ``export_2d_annotation`` - ``<info>_mono3d.coco.json``. The reference's step-1 function
  (kitti_converter_gga.py:628-844) and its step-3 one (kitti_converter_mono.py:626-842) are the same text, so this is
  ``kitti_converter_mono.export_2d_annotation``.

The per-frame point stage. A frame's cloud is asked: which points lie in the image frustum (``num_points_in_gt`` counts
only those; they are also the reduced cloud), how many of them in each ground-truth box, and which points lie in each
object's 2D-box frustum (the seeds of the region growing). By default (``prepare_frame_points``) the velodyne file is read
once and all of it is ONE ``label_gen.frame_point_tests`` call with polyhedra [image frustum, boxes..., object frusta...]
and ``reduce_poly=0``; the reduced cloud is written to ``velodyne_reduced`` from the same result.
``GGA_PREP_ONE_PASS=0`` keeps the per-call form: one float64 upload, launch and download per question.

Different from the reference: a frame without objects (only DontCare lines) gets empty GGA fields - there the reference
raises (``np.concatenate`` of an empty list) inside a pool worker, the frame's pickle is never written and the merge fails.
The per-frame files go to ``split_save_path`` (default ``<data_path>/kitti_GGA_split_file``), not to a path relative to the
working directory.
"""
import os
import pickle
from pathlib import Path

import numpy as np

from . import label_gen as LG
from .gt_database import points_in_rbbox, rbbox_surfaces
from .kitti_converter_mono import export_2d_annotation      # noqa: F401  (the step-1 function: see the module docstring)
from .kitti_data_utils import get_kitti_image_info


def limit_period(val, offset=0.5, period=np.pi):
    return val - np.floor(val / period + offset) * period


def box_camera_to_lidar(data, r_rect, velo2cam):
    """box_np_ops.box_camera_to_lidar (core/bbox/box_np_ops.py:45-67)."""
    xyz = data[:, 0:3]
    x_size, y_size, z_size = data[:, 3:4], data[:, 4:5], data[:, 5:6]
    r = data[:, 6:7]
    xyz_lidar = LG.camera_to_lidar(xyz, r_rect, velo2cam)
    r_new = limit_period(-r - np.pi / 2, period=np.pi * 2)
    return np.concatenate([xyz_lidar, x_size, z_size, y_size, r_new], axis=1)


def remove_outside_points(points, rect, Trv2c, P2, image_shape):
    """box_np_ops.remove_outside_points (:745-771): keep the points inside the camera frustum."""
    inside = LG.points_in_frustm_indices(points, rect, Trv2c, P2, [0, 0, image_shape[1], image_shape[0]])
    return points[inside.reshape([-1])]


def _read_imageset_file(path):
    with open(path, 'r') as f:
        lines = f.readlines()
    return [int(line) for line in lines]


def _velodyne_path(data_path, info, relative_path):
    p = info['point_cloud']['velodyne_path']
    return str(Path(data_path) / p) if relative_path else p


def _read_velodyne(data_path, info, relative_path, num_features=4):
    return np.fromfile(_velodyne_path(data_path, info, relative_path), dtype=np.float32, count=-1).reshape([-1, num_features])


def _gt_boxes_lidar(info):
    annos, calib = info['annos'], info['calib']
    num_obj = len([n for n in annos['name'] if n != 'DontCare'])
    gt_boxes_camera = np.concatenate([annos['location'][:num_obj], annos['dimensions'][:num_obj],
                                      annos['rotation_y'][:num_obj][..., np.newaxis]], axis=1)
    return box_camera_to_lidar(gt_boxes_camera, calib['R0_rect'], calib['Tr_velo_to_cam']), num_obj


def calculate_num_points_in_gt(data_path, infos, relative_path, remove_outside=True, num_features=4):
    """``_calculate_num_points_in_gt`` (kitti_converter_gga.py:153-192): annos['num_points_in_gt']."""
    for info in infos:
        calib = info['calib']
        points_v = _read_velodyne(data_path, info, relative_path, num_features)
        rect, Trv2c, P2 = calib['R0_rect'], calib['Tr_velo_to_cam'], calib['P2']
        if remove_outside:
            points_v = remove_outside_points(points_v, rect, Trv2c, P2, info['image']['image_shape'])
        annos = info['annos']
        gt_boxes_lidar, num_obj = _gt_boxes_lidar(info)
        indices = points_in_rbbox(points_v[:, :3], gt_boxes_lidar)
        num_ignored = len(annos['dimensions']) - num_obj
        annos['num_points_in_gt'] = np.concatenate([indices.sum(0), -np.ones([num_ignored])]).astype(np.int32)
    return infos


def _image_frustum(info):
    calib, shape = info['calib'], info['image']['image_shape']
    return LG.frustum_surfaces(calib['R0_rect'], calib['Tr_velo_to_cam'], calib['P2'], [0, 0, shape[1], shape[0]])


def _image_shape(info):
    return tuple(int(v) for v in info['image']['image_shape'][:2])


def prepare_frame_points(info, points_v):
    """The point stage of one frame in one pass: sets ``annos['num_points_in_gt']`` and
    -> (the objects' frustum masks, one bool [N] per object, for ``calculate_rga(frusta=)``; the reduced cloud)."""
    annos, calib = info['annos'], info['calib']
    gt_boxes_lidar, num_obj = _gt_boxes_lidar(info)
    boxes_img = LG.box2d_labels(annos, calib['P2'], _image_shape(info))[0] if num_obj else np.zeros((0, 4))
    surfaces = [_image_frustum(info)]
    if num_obj:
        surfaces.append(rbbox_surfaces(gt_boxes_lidar))
        surfaces += [LG.frustum_surfaces(calib['R0_rect'], calib['Tr_velo_to_cam'], calib['P2'], b) for b in boxes_img]
    member, _, counts_reduced, reduced, _ = LG.frame_point_tests(points_v, surfaces, reduce_poly=0)
    num_ignored = len(annos['dimensions']) - num_obj
    annos['num_points_in_gt'] = np.concatenate([counts_reduced[1:1 + num_obj], -np.ones([num_ignored])]).astype(np.int32)
    return [member[:, 1 + num_obj + j] for j in range(num_obj)], reduced


def _rga_without_objects(annos):
    """The GGA fields of a frame that has only DontCare entries, laid out as ``calculate_rga`` pads them."""
    n_ign = len(annos['dimensions'])
    annos['GGA_boxes_img'] = -np.zeros([n_ign, 4])
    for key in ('GGA_mask2d', 'GGA_mask_depth', 'GGA_mask_boundary', 'GGA_mask_valid'):
        annos[key] = np.zeros([n_ign]).astype(bool)
    annos['GGA_bdry_masks'] = np.zeros([n_ign, 4]).astype(bool)
    annos['GGA_in_box_points'] = [np.array([]) for _ in range(n_ign)]
    annos['GGA_init_pseudo_label'] = np.zeros([n_ign, 7])
    annos['GGA_num_points_in_box2d'] = np.zeros([n_ign])
    return annos


def _reduced_path(data_path, info, save_path=None, back=False):
    """Where ``_create_reduced_point_cloud`` (:566-577) puts a frame's reduced cloud."""
    v_path = Path(data_path) / info['point_cloud']['velodyne_path']
    if save_path is None:
        save_dir = v_path.parent.parent / (v_path.parent.stem + '_reduced')
        save_dir.mkdir(exist_ok=True)
        name = str(save_dir / v_path.name)
    else:
        name = str(Path(save_path) / v_path.name)
    return name + '_back' if back else name


# reduced clouds this process has already written from a frame's one pass: create_reduced_point_cloud skips them
_REDUCED_WRITTEN = set()


def _write_reduced(filename, points):
    with open(filename, 'w') as f:
        points.tofile(f)


def calculate_rga_file(data_path, info, relative_path, save_path, num_features=4, resume=False, frame_points=False):
    """One frame of ``_calculate_rga`` including its file handling (:214-245, :517-518): read the
    velodyne file, run the label generation, dump ``GGA_kitti_scene_<idx>.pkl`` under ``save_path``.
    ``frame_points``: the whole point stage belongs to this call (``prepare_frame_points``: num_points_in_gt, the object
    frusta and the frame's ``velodyne_reduced`` file from one pass over the file as read)."""
    filename = os.path.join(save_path, 'GGA_kitti_scene_{}.pkl'.format(info['image']['image_idx']))
    if resume and os.path.exists(filename):
        return filename
    points_v = _read_velodyne(data_path, info, relative_path, num_features)
    frusta = None
    if frame_points:
        frusta, reduced = prepare_frame_points(info, points_v)
        if relative_path:
            out = _reduced_path(data_path, info)
            _write_reduced(out, reduced)
            _REDUCED_WRITTEN.add(os.path.abspath(out))
    if len([n for n in info['annos']['name'] if n != 'DontCare']) == 0:
        _rga_without_objects(info['annos'])
    else:
        LG.calculate_rga(points_v, info['calib'], info['annos'], _image_shape(info), frusta=frusta)
    os.makedirs(save_path, exist_ok=True)
    with open(filename, 'wb') as f:
        pickle.dump(info, f)
    return filename


def create_gga_info_file(data_path, infos, image_ids, out_file, relative_path=True, save_path='./data/kitti_GGA_split_file',
                         resume=False, seed=None, logger=print, compute_num_points=True):
    """The GGA part of ``create_kitti_info_file`` for one split (:70-99): num_points_in_gt, the
    per-frame label generation, then the merge of the per-frame files in ``image_ids`` order into
    ``out_file``. ``seed``: re-seed ``np.random`` per frame with ``seed + image_idx`` (the RANSAC
    ground fit draws from it; the reference's pool workers inherit an arbitrary state)."""
    frame_points = compute_num_points and LG.one_pass()
    if compute_num_points and not frame_points:      # False: the infos already carry annos['num_points_in_gt']
        calculate_num_points_in_gt(data_path, infos, relative_path)
    for info in infos:
        if seed is not None:
            np.random.seed(seed + int(info['image']['image_idx']))
        calculate_rga_file(data_path, info, relative_path, save_path, resume=resume, frame_points=frame_points)
        logger('Finish Processing Sample {}'.format(info['image']['image_idx']))
    merged = []
    for idx in image_ids:
        with open(os.path.join(save_path, 'GGA_kitti_scene_{}.pkl'.format(int(idx))), 'rb') as f:
            merged.append(pickle.load(f))
    with open(out_file, 'wb') as f:
        pickle.dump(merged, f)
    logger(f'Kitti info file is saved to {out_file}')
    return merged


def create_kitti_info_file(data_path, pkl_prefix='kitti', with_plane=False, save_path=None, relative_path=True,
                           split_save_path=None, seed=None, resume=False, num_worker=8, logger=print):
    """``create_kitti_info_file`` (kitti_converter_gga.py:32-150): ``<prefix>_infos_{train,val,trainval}_GGA.pkl`` and
    ``<prefix>_infos_test.pkl`` under ``save_path`` (default ``data_path``) from ``ImageSets/{train,val,test}.txt``.
    The test split has no labels. ``split_save_path``: the per-frame pickles (default
    ``<data_path>/kitti_GGA_split_file``); ``seed`` / ``resume``: see ``create_gga_info_file``."""
    imageset_folder = Path(data_path) / 'ImageSets'
    train_img_ids = _read_imageset_file(str(imageset_folder / 'train.txt'))
    val_img_ids = _read_imageset_file(str(imageset_folder / 'val.txt'))
    test_img_ids = _read_imageset_file(str(imageset_folder / 'test.txt'))
    logger('Generate info. this may take several minutes.')
    save_path = Path(data_path) if save_path is None else Path(save_path)
    split_save_path = str(Path(data_path) / 'kitti_GGA_split_file') if split_save_path is None else str(split_save_path)
    merged = {}
    for split, ids in (('train', train_img_ids), ('val', val_img_ids)):
        infos = get_kitti_image_info(data_path, training=True, velodyne=True, calib=True, with_plane=with_plane, image_ids=ids,
                                     relative_path=relative_path, num_worker=num_worker)
        merged[split] = create_gga_info_file(data_path, infos, ids, str(save_path / f'{pkl_prefix}_infos_{split}_GGA.pkl'),
                                             relative_path=relative_path, save_path=split_save_path, resume=resume, seed=seed,
                                             logger=logger)
    filename = save_path / f'{pkl_prefix}_infos_trainval_GGA.pkl'
    logger(f'Kitti info trainval file is saved to {filename}')
    with open(filename, 'wb') as f:
        pickle.dump(merged['train'] + merged['val'], f)
    kitti_infos_test = get_kitti_image_info(data_path, training=False, label_info=False, velodyne=True, calib=True, with_plane=False,
                                            image_ids=test_img_ids, relative_path=relative_path, num_worker=num_worker)
    filename = save_path / f'{pkl_prefix}_infos_test.pkl'
    logger(f'Kitti info test file is saved to {filename}')
    with open(filename, 'wb') as f:
        pickle.dump(kitti_infos_test, f)


def _create_reduced_point_cloud(data_path, info_path, save_path=None, back=False, num_features=4, front_camera_id=2):
    """``_create_reduced_point_cloud`` (:521-579): for every info of ``info_path`` the points inside the image frustum of
    camera ``front_camera_id``, in file order, to ``<split>/velodyne_reduced/<idx>.bin`` (or under ``save_path``)."""
    with open(info_path, 'rb') as f:
        kitti_infos = pickle.load(f)
    for info in kitti_infos:
        filename = _reduced_path(data_path, info, save_path, back)
        if os.path.abspath(filename) in _REDUCED_WRITTEN:      # written from the frame's one pass by this run
            continue
        calib = info['calib']
        points_v = _read_velodyne(data_path, info, True, num_features)
        rect, Trv2c = calib['R0_rect'], calib['Tr_velo_to_cam']
        P2 = calib['P2'] if front_camera_id == 2 else calib[f'P{str(front_camera_id)}']
        shape = info['image']['image_shape']
        if back:
            points_v[:, 0] = -points_v[:, 0]
        if LG.one_pass():
            surf = LG.frustum_surfaces(rect, Trv2c, P2, [0, 0, shape[1], shape[0]])
            points_v = LG.frame_point_tests(points_v, surf, reduce_poly=0)[3]
        else:
            points_v = remove_outside_points(points_v, rect, Trv2c, P2, shape)
        _write_reduced(filename, points_v)


def create_reduced_point_cloud(data_path, pkl_prefix, train_info_path=None, val_info_path=None, test_info_path=None,
                               save_path=None, with_back=False):
    """``create_reduced_point_cloud`` (:583-625) for the train, val and test infos of ``pkl_prefix``."""
    if train_info_path is None:
        train_info_path = Path(data_path) / f'{pkl_prefix}_infos_train_GGA.pkl'
    if val_info_path is None:
        val_info_path = Path(data_path) / f'{pkl_prefix}_infos_val_GGA.pkl'
    if test_info_path is None:
        test_info_path = Path(data_path) / f'{pkl_prefix}_infos_test.pkl'
    for path in (train_info_path, val_info_path, test_info_path):
        _create_reduced_point_cloud(data_path, path, save_path)
    if with_back:
        for path in (train_info_path, val_info_path, test_info_path):
            _create_reduced_point_cloud(data_path, path, save_path, back=True)


def kitti_data_prep(root_path, info_prefix, version='v1.0', out_dir=None, with_plane=False, workers=4, seed=None, resume=False,
                    logger=print):
    """``kitti_data_prep`` of tools/create_data_gga.py:18-55, in its order: the info files, the reduced clouds, the four
    mono3d coco files, the ground-truth database (from ``<out_dir>/<prefix>_infos_train_GGA.pkl``). ``version='mask'``
    (instance masks in the database) is not built."""
    from .gt_database import create_groundtruth_database
    if version == 'mask':
        raise NotImplementedError('kitti_data_prep: the mask version (with_mask) of the ground-truth database')
    out_dir = root_path if out_dir is None else out_dir
    create_kitti_info_file(root_path, info_prefix, with_plane, seed=seed, resume=resume, num_worker=workers, logger=logger)
    create_reduced_point_cloud(root_path, info_prefix)
    for name in (f'{info_prefix}_infos_train_GGA.pkl', f'{info_prefix}_infos_val_GGA.pkl', f'{info_prefix}_infos_trainval_GGA.pkl',
                 f'{info_prefix}_infos_test.pkl'):
        export_2d_annotation(root_path, os.path.join(root_path, name))
    create_groundtruth_database('KittiDataset_GGA', root_path, info_prefix,
                                info_path=os.path.join(out_dir, f'{info_prefix}_infos_train_GGA.pkl'), logger=logger)
