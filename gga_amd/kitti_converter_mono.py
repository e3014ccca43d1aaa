"""The hand-over on disk between the pseudo-label file and PGD's dataset: KITTI info pickle -> ``<info>_mono3d.coco.json``
(``images``, ``annotations``, ``categories``), step 3 of the reference's workflow (tools/create_data_gga_retrain_mono.py:9-31).

Mirrors tools/data_converter/kitti_converter_mono.py:626-842 (``export_2d_annotation``, ``get_2d_boxes``,
``generate_record``) and tools/data_converter/nuscenes_converter.py:534-564 (``post_process_coords``). The reference takes the
convex hull and its intersection with the canvas from shapely and the projection from the nuScenes devkit; neither is needed:
``hull_clip_bounds`` is a monotone-chain hull and a Sutherland-Hodgman clip in float64, ``view_points`` three lines.

Kept as the reference has it: the canvas of ``post_process_coords`` is its default (1600, 900), not the image size; the centre
moves from the bottom to the middle of the box; ``bbox_cam3d`` carries the P2 - P0 x offset while ``center2d`` is projected
from the unshifted centre; records whose centre has depth <= 0 are dropped; ``velo_cam3d`` / ``attribute_*`` are -1.
Different: the infos are not modified in place, and a box whose in-front corners have a hull of fewer than three distinct
points (one or two corners in front of the camera) is skipped - there the reference raises, a Point or LineString having no
``exterior``. Image sizes come from the file header (PIL)."""
import json
import os
import pickle

import numpy as np

kitti_categories = ('Pedestrian', 'Cyclist', 'Car')
CANVAS = (1600, 900)            # post_process_coords' default imsize, which get_2d_boxes never overrides


def convex_hull(points):
    """Andrew's monotone chain -> hull vertices counter-clockwise, collinear points dropped; float64 [k, 2]."""
    pts = sorted(set((float(x), float(y)) for x, y in points))
    if len(pts) <= 2:
        return np.array(pts, np.float64).reshape(-1, 2)
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1], np.float64).reshape(-1, 2)


def clip_to_rectangle(polygon, x_max, y_max):
    """Sutherland-Hodgman: a convex polygon [k, 2] clipped to [0, x_max] x [0, y_max] -> its vertices (possibly none)."""
    poly = [tuple(p) for p in np.asarray(polygon, np.float64)]
    for axis, bound, keep_below in ((0, 0.0, False), (0, float(x_max), True), (1, 0.0, False), (1, float(y_max), True)):
        inside = (lambda p: p[axis] <= bound) if keep_below else (lambda p: p[axis] >= bound)
        out = []
        for i, cur in enumerate(poly):
            prev = poly[i - 1]
            if inside(cur) != inside(prev):
                t = (bound - prev[axis]) / (cur[axis] - prev[axis])
                cut = [prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])]
                cut[axis] = bound
                out.append(tuple(cut))
            if inside(cur):
                out.append(cur)
        poly = out
        if not poly:
            break
    return np.array(poly, np.float64).reshape(-1, 2)


def hull_clip_bounds(corner_coords, imsize=CANVAS):
    """``post_process_coords``: (min_x, min_y, max_x, max_y) of (convex hull of the points) intersected with the canvas, or
    None when they do not meet - or when the hull has fewer than three distinct vertices (see the module docstring)."""
    hull = convex_hull(corner_coords)
    if len(hull) < 3:
        return None
    inter = clip_to_rectangle(hull, imsize[0], imsize[1])
    if len(inter) == 0:
        return None
    return float(inter[:, 0].min()), float(inter[:, 1].min()), float(inter[:, 0].max()), float(inter[:, 1].max())


def view_points(points, view, normalize):
    """nuscenes.utils.geometry_utils.view_points: points [3, n] through the (up to 4 x 4) matrix ``view``, optionally
    divided by their depth."""
    viewpad = np.eye(4)
    viewpad[:view.shape[0], :view.shape[1]] = view
    points = (viewpad @ np.concatenate((points, np.ones((1, points.shape[1])))))[:3, :]
    return points / points[2:3, :].repeat(3, 0).reshape(3, points.shape[1]) if normalize else points


def _corners(center, dims, angle):
    """box_np_ops.center_to_corner_box3d(..., origin (0.5, 0.5, 0.5), axis=1) for one box -> [8, 3], in the arrays' dtype."""
    norm = np.stack(np.unravel_index(np.arange(8), [2] * 3), axis=1).astype(dims.dtype)[[0, 1, 3, 2, 4, 5, 7, 6]]
    corners = dims.reshape(1, 3) * (norm - np.array([0.5, 0.5, 0.5], dtype=dims.dtype))
    c, s = np.cos(angle), np.sin(angle)
    rot_t = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], dtype=dims.dtype)
    return corners @ rot_t + center.reshape(1, 3)


def generate_record(ann_rec, x1, y1, x2, y2, sample_data_token, filename):
    """kitti_converter_mono.py:788-842 -> the coco record, or None for a category outside ``kitti_categories``."""
    if ann_rec['name'] not in kitti_categories:
        return None
    coco_rec = dict()
    coco_rec['file_name'] = filename
    coco_rec['image_id'] = sample_data_token
    coco_rec['area'] = (y2 - y1) * (x2 - x1)
    coco_rec['category_name'] = str(ann_rec['name'])
    coco_rec['category_id'] = kitti_categories.index(ann_rec['name'])
    coco_rec['bbox'] = [x1, y1, x2 - x1, y2 - y1]
    coco_rec['iscrowd'] = 0
    return coco_rec


def get_2d_boxes(info, occluded, mono3d=True):
    """kitti_converter_mono.py:674-785: the 2D (and mono3d) annotation records of one info; entries may be None (unknown
    category), which ``export_2d_annotation`` leaves out."""
    P2 = info['calib']['P2']
    repro_recs = []
    if 'annos' not in info:         # test infos
        return repro_recs
    annos = info['annos']
    keep = [i for i, ocld in enumerate(annos['occluded']) if ocld in occluded]
    for ann_idx, i in enumerate(keep):
        ann_rec = {k: annos[k][i] for k in ('name', 'location', 'dimensions', 'rotation_y')}
        sample_data_token = info['image']['image_idx']
        loc = np.asarray(ann_rec['location'])[np.newaxis, :]
        dim = np.asarray(ann_rec['dimensions'])[np.newaxis, :]
        rot = np.asarray(ann_rec['rotation_y'])[np.newaxis, np.newaxis]
        loc = loc + dim * (np.array([0.5, 0.5, 0.5]) - np.array([0.5, 1.0, 0.5]))          # bottom centre -> gravity centre
        offset = (info['calib']['P2'][0, 3] - info['calib']['P0'][0, 3]) / info['calib']['P2'][0, 0]
        loc_3d = np.copy(loc)
        loc_3d[0, 0] += offset
        gt_bbox_3d = np.concatenate([loc, dim, rot], axis=1).astype(np.float32)
        corners_3d = _corners(gt_bbox_3d[0, :3], gt_bbox_3d[0, 3:6], gt_bbox_3d[0, 6]).T          # [3, 8]
        in_front = np.argwhere(corners_3d[2, :] > 0).flatten()
        corners_3d = corners_3d[:, in_front]
        corner_coords = view_points(corners_3d, P2, True).T[:, :2].tolist()
        final_coords = hull_clip_bounds(corner_coords)
        if final_coords is None:
            continue
        min_x, min_y, max_x, max_y = final_coords
        repro_rec = generate_record(ann_rec, min_x, min_y, max_x, max_y, sample_data_token, info['image']['image_path'])
        if mono3d and repro_rec is not None:
            repro_rec['bbox_cam3d'] = np.concatenate([loc_3d, dim, rot], axis=1).astype(np.float32).squeeze().tolist()
            repro_rec['velo_cam3d'] = -1
            center3d = np.concatenate([np.array(loc, np.float64).reshape(1, 3), np.ones((1, 1))], 1)
            proj = np.eye(4)
            proj[:P2.shape[0], :P2.shape[1]] = P2
            p = center3d @ proj.T
            repro_rec['center2d'] = np.concatenate([p[:, :2] / p[:, 2:3], p[:, 2:3]], 1).squeeze().tolist()
            if repro_rec['center2d'][2] <= 0:          # samples with depth <= 0 are removed
                continue
            repro_rec['attribute_name'] = -1
            repro_rec['attribute_id'] = -1
        repro_recs.append(repro_rec)
    return repro_recs


def _listed(value):
    return value.tolist() if isinstance(value, np.ndarray) else value


def export_2d_annotation(root_path, info_path, mono3d=True):
    """kitti_converter_mono.py:626-671: ``info_path`` (an info pickle) -> ``<info>_mono3d.coco.json`` beside it (without
    ``mono3d``: ``<info>.coco.json``). Annotation ids are consecutive over the file; matrices go out as nested lists.
    -> the json's path."""
    from PIL import Image
    with open(info_path, 'rb') as f:
        kitti_infos = pickle.load(f)
    cat2Ids = [dict(id=kitti_categories.index(cat_name), name=cat_name) for cat_name in kitti_categories]
    coco_ann_id = 0
    coco_2d_dict = dict(annotations=[], images=[], categories=cat2Ids)
    for info in kitti_infos:
        coco_infos = get_2d_boxes(info, occluded=[0, 1, 2, 3], mono3d=mono3d)
        with Image.open(os.path.join(root_path, info['image']['image_path'])) as im:
            width, height = im.size
        calib = info['calib']
        coco_2d_dict['images'].append(dict(file_name=info['image']['image_path'], id=int(info['image']['image_idx']),
                                           Tri2v=_listed(calib['Tr_imu_to_velo']), Trv2c=_listed(calib['Tr_velo_to_cam']),
                                           rect=_listed(calib['R0_rect']), cam_intrinsic=_listed(calib['P2']), width=width,
                                           height=height))
        for coco_info in coco_infos:
            if coco_info is None:
                continue
            coco_info['image_id'] = int(coco_info['image_id'])
            coco_info['segmentation'] = []
            coco_info['id'] = coco_ann_id
            coco_2d_dict['annotations'].append(coco_info)
            coco_ann_id += 1
    json_prefix = f'{info_path[:-4]}_mono3d' if mono3d else f'{info_path[:-4]}'
    with open(f'{json_prefix}.coco.json', 'w') as f:
        json.dump(coco_2d_dict, f)
    return f'{json_prefix}.coco.json'


def kitti_data_prep(root_path, info_prefix, version=None, out_dir=None, with_plane=False):
    """tools/create_data_gga_retrain_mono.py:9-31: the coco files of the pseudo-labelled trainval infos and the test infos."""
    out = [export_2d_annotation(root_path, os.path.join(root_path, f'{info_prefix}_infos_trainval_GGA_pseudo.pkl'))]
    test = os.path.join(root_path, f'{info_prefix}_infos_test.pkl')
    out.append(export_2d_annotation(root_path, test))
    return out
