"""Raw KITTI files -> the stock info dicts: the parsing half of step 1 of the recipe (``tools/create_data_gga.py kitti``),
``tools/data_converter/kitti_data_utils.py:13-295,534-576`` of the reference. Host code; same names, arguments, dict keys,
dtypes and array shapes, because the info pickles are the on-disk protocol every later step reads.

Different: ``image_shape`` comes from the image header (PIL opens a file without decoding its pixels) where the reference
decodes the whole image for its ``.shape``; the plane file is read with plain file I/O. ``score`` is read only where the
label file has a 16th column (a detection file) and is zeros otherwise, as in the reference.
"""
from concurrent import futures
from pathlib import Path

import numpy as np


def get_image_index_str(img_idx, use_prefix_id=False):
    return '{:07d}'.format(img_idx) if use_prefix_id else '{:06d}'.format(img_idx)


def get_kitti_info_path(idx, prefix, info_type='image_2', file_tail='.png', training=True, relative_path=True, exist_check=True,
                        use_prefix_id=False):
    name = get_image_index_str(idx, use_prefix_id) + file_tail
    prefix = Path(prefix)
    file_path = Path('training' if training else 'testing') / info_type / name
    if exist_check and not (prefix / file_path).exists():
        raise ValueError('file not exist: {}'.format(file_path))
    return str(file_path) if relative_path else str(prefix / file_path)


def get_image_path(idx, prefix, training=True, relative_path=True, exist_check=True, info_type='image_2', file_tail='.png',
                   use_prefix_id=False):
    return get_kitti_info_path(idx, prefix, info_type, file_tail, training, relative_path, exist_check, use_prefix_id)


def get_label_path(idx, prefix, training=True, relative_path=True, exist_check=True, info_type='label_2', use_prefix_id=False):
    return get_kitti_info_path(idx, prefix, info_type, '.txt', training, relative_path, exist_check, use_prefix_id)


def get_plane_path(idx, prefix, training=True, relative_path=True, exist_check=True, info_type='planes', use_prefix_id=False):
    return get_kitti_info_path(idx, prefix, info_type, '.txt', training, relative_path, exist_check, use_prefix_id)


def get_velodyne_path(idx, prefix, training=True, relative_path=True, exist_check=True, use_prefix_id=False):
    return get_kitti_info_path(idx, prefix, 'velodyne', '.bin', training, relative_path, exist_check, use_prefix_id)


def get_calib_path(idx, prefix, training=True, relative_path=True, exist_check=True, use_prefix_id=False):
    return get_kitti_info_path(idx, prefix, 'calib', '.txt', training, relative_path, exist_check, use_prefix_id)


def get_label_anno(label_path):
    """One ``label_2`` file -> the annotation dict. Lines keep the file's order (KITTI lists DontCare regions last);
    ``index`` numbers the objects and is -1 for DontCare; ``dimensions`` go from the file's (h, w, l) to (l, h, w)."""
    with open(label_path, 'r') as f:
        content = [line.strip().split(' ') for line in f.readlines()]
    num_objects = len([x[0] for x in content if x[0] != 'DontCare'])
    annotations = {}
    annotations['name'] = np.array([x[0] for x in content])
    num_gt = len(annotations['name'])
    annotations['truncated'] = np.array([float(x[1]) for x in content])
    annotations['occluded'] = np.array([int(x[2]) for x in content])
    annotations['alpha'] = np.array([float(x[3]) for x in content])
    annotations['bbox'] = np.array([[float(v) for v in x[4:8]] for x in content]).reshape(-1, 4)
    annotations['dimensions'] = np.array([[float(v) for v in x[8:11]] for x in content]).reshape(-1, 3)[:, [2, 0, 1]]
    annotations['location'] = np.array([[float(v) for v in x[11:14]] for x in content]).reshape(-1, 3)
    annotations['rotation_y'] = np.array([float(x[14]) for x in content]).reshape(-1)
    if len(content) != 0 and len(content[0]) == 16:          # a detection file
        annotations['score'] = np.array([float(x[15]) for x in content])
    else:
        annotations['score'] = np.zeros((annotations['bbox'].shape[0], ))
    annotations['index'] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
    annotations['group_ids'] = np.arange(num_gt, dtype=np.int32)
    return annotations


def _extend_matrix(mat):
    return np.concatenate([mat, np.array([[0., 0., 0., 1.]])], axis=0)


def _calib_row(line, count, shape):
    return np.array([float(v) for v in line.split(' ')[1:1 + count]]).reshape(shape)


def get_kitti_image_info(path, training=True, label_info=True, velodyne=False, calib=False, with_plane=False, image_ids=7481,
                         extend_matrix=True, num_worker=8, relative_path=True, with_imageshape=True):
    """The info dicts of ``image_ids`` (a list, or a count meaning 0..count-1), in that order:
    ``image`` {image_idx, image_path, image_shape int32 (H, W)}, ``point_cloud`` {num_features: 4, velodyne_path},
    ``calib`` {P0..P3, R0_rect, Tr_velo_to_cam, Tr_imu_to_velo; 4x4 with ``extend_matrix``}, ``plane`` (``with_plane``),
    ``annos`` (``label_info``; with ``difficulty``). ``num_worker`` threads read the files."""
    from PIL import Image
    root_path = Path(path)
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))

    def map_func(idx):
        info = {}
        pc_info = {'num_features': 4}
        image_info = {'image_idx': idx}
        annotations = None
        if velodyne:
            pc_info['velodyne_path'] = get_velodyne_path(idx, path, training, relative_path)
        image_info['image_path'] = get_image_path(idx, path, training, relative_path)
        if with_imageshape:
            img_path = image_info['image_path']
            if relative_path:
                img_path = str(root_path / img_path)
            with Image.open(img_path) as im:          # the header only
                w, h = im.size
            image_info['image_shape'] = np.array((h, w), dtype=np.int32)
        if label_info:
            label_path = get_label_path(idx, path, training, relative_path)
            if relative_path:
                label_path = str(root_path / label_path)
            annotations = get_label_anno(label_path)
        info['image'] = image_info
        info['point_cloud'] = pc_info
        if calib:
            with open(get_calib_path(idx, path, training, relative_path=False), 'r') as f:
                lines = f.readlines()
            P = [_calib_row(lines[i], 12, [3, 4]) for i in range(4)]
            R0_rect = _calib_row(lines[4], 9, [3, 3])
            Tr_velo_to_cam = _calib_row(lines[5], 12, [3, 4])
            Tr_imu_to_velo = _calib_row(lines[6], 12, [3, 4])
            if extend_matrix:
                P = [_extend_matrix(m) for m in P]
                rect_4x4 = np.zeros([4, 4], dtype=R0_rect.dtype)
                rect_4x4[3, 3] = 1.
                rect_4x4[:3, :3] = R0_rect
                Tr_velo_to_cam = _extend_matrix(Tr_velo_to_cam)
                Tr_imu_to_velo = _extend_matrix(Tr_imu_to_velo)
            else:
                rect_4x4 = R0_rect
            info['calib'] = {'P0': P[0], 'P1': P[1], 'P2': P[2], 'P3': P[3], 'R0_rect': rect_4x4,
                             'Tr_velo_to_cam': Tr_velo_to_cam, 'Tr_imu_to_velo': Tr_imu_to_velo}
        if with_plane:
            plane_path = get_plane_path(idx, path, training, relative_path)
            if relative_path:
                plane_path = str(root_path / plane_path)
            with open(plane_path, 'r') as f:
                lines = [line.rstrip('\n\r') for line in f]
            info['plane'] = np.array([float(i) for i in lines[3].split()])
        if annotations is not None:
            info['annos'] = annotations
            add_difficulty_to_annos(info)
        return info

    with futures.ThreadPoolExecutor(num_worker) as executor:
        image_infos = executor.map(map_func, image_ids)
    return list(image_infos)


def add_difficulty_to_annos(info):
    """KITTI's easy / moderate / hard (0 / 1 / 2, else -1) from the 2D box height, occlusion and truncation ->
    ``annos['difficulty']`` int32; returns the list."""
    min_height = [40, 25, 25]
    max_occlusion = [0, 1, 2]
    max_trunc = [0.15, 0.3, 0.5]
    annos = info['annos']
    dims = annos['dimensions']
    bbox = annos['bbox']
    height = bbox[:, 3] - bbox[:, 1]
    masks = [np.ones((len(dims), ), dtype=bool) for _ in range(3)]
    for i, (h, o, t) in enumerate(zip(height, annos['occluded'], annos['truncated'])):
        for level in range(3):
            if o > max_occlusion[level] or h <= min_height[level] or t > max_trunc[level]:
                masks[level][i] = False
    is_easy = masks[0]
    is_moderate = np.logical_xor(masks[0], masks[1])
    is_hard = np.logical_xor(masks[2], masks[1])
    diff = []
    for i in range(len(dims)):
        diff.append(0 if is_easy[i] else 1 if is_moderate[i] else 2 if is_hard[i] else -1)
    annos['difficulty'] = np.array(diff, np.int32)
    return diff
