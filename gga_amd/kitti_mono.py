"""``KittiMonoDataset``: the image-branch dataset of configs/gga/gga_pdg.py - PGD retrained on the GGA pseudo labels.

Mirrors mmdet3d/datasets/kitti_mono_dataset.py:17-570 and what it inherits from ``NuScenesMonoDataset``
(nuscenes_mono_dataset.py:78-175) and mmdet's ``CocoDataset`` / ``CustomDataset`` (third-party, not in the tree; pycocotools
is not needed - the coco json written by ``kitti_converter_mono`` is read directly):

* load: ``cat_ids`` follow ``CLASSES`` by name, ``data_infos`` are the image records in ascending id order with
  ``filename = file_name``, ``get_ann_info`` hands an image's annotations (in file order) to ``_parse_ann_info``;
* train mode: ``_filter_imgs`` (no annotation of a known class, or a side below 32 px), ``_set_group_flag`` (aspect ratio),
  ``__getitem__`` retries another index of the same group when the pipeline gives None;
* results: ``format_results`` / ``bbox2result_kitti`` / ``bbox2result_kitti2d`` / ``convert_valid_bboxes`` / ``evaluate``;
  ground truth comes from ``anno_infos`` (the info pickle), AP from ``gga_amd.kitti_eval.kitti_eval``.
  ``bbox2result_kitti(device=...)`` formats all frames in one launch (``kitti_format.format_kitti_dets_cam``) unless
  ``GGA_KITTI_FORMAT=0``.

Pinned by tests/test_kitti_mono.py against vectors of the reference's own method bodies (tests/golden/kitti_mono.npz)."""
import copy
import json
import os
import pickle
import tempfile

import numpy as np
import torch

from .box3d import CameraInstance3DBoxes, points_cam2img
from .datasets import KittiDataset_GGA_train, camera_boxes_to_lidar
from .pipelines import Compose
from .registry import DATASETS


def _empty_anno():
    return dict(name=np.array([]), truncated=np.array([]), occluded=np.array([]), alpha=np.array([]), bbox=np.zeros([0, 4]),
                dimensions=np.zeros([0, 3]), location=np.zeros([0, 3]), rotation_y=np.array([]), score=np.array([]))


@DATASETS.register_module()
class KittiMonoDataset:
    CLASSES = ('Pedestrian', 'Cyclist', 'Car')

    def __init__(self, data_root, info_file, ann_file, pipeline, load_interval=1, with_velocity=False, eval_version=None,
                 version=None, modality=None, box_type_3d='Camera', use_valid_flag=False, classes=None, img_prefix='',
                 seg_prefix=None, proposal_file=None, test_mode=False, filter_empty_gt=True, **kwargs):
        if box_type_3d.lower() != 'camera':
            raise NotImplementedError('KittiMonoDataset uses box_type_3d="Camera"')
        if proposal_file is not None or eval_version is not None:
            raise NotImplementedError('KittiMonoDataset: proposals / a nuScenes eval_version are not part of the KITTI path')
        self.data_root, self.ann_file, self.img_prefix, self.seg_prefix = data_root, ann_file, img_prefix, seg_prefix
        self.proposal_file, self.test_mode, self.filter_empty_gt = proposal_file, test_mode, filter_empty_gt
        self.CLASSES = tuple(classes) if classes is not None else self.CLASSES
        self.data_infos = self.load_annotations(ann_file)
        if not test_mode:
            valid_inds = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid_inds]
            self._set_group_flag()
        self.pipeline = Compose(pipeline) if pipeline is not None else None
        self.load_interval, self.with_velocity, self.use_valid_flag, self.version = load_interval, with_velocity, use_valid_flag, version
        self.modality = modality if modality is not None else dict(use_camera=True, use_lidar=False, use_radar=False, use_map=False,
                                                                   use_external=False)
        self.box_type_3d, self.box_mode_3d = CameraInstance3DBoxes, 1           # Box3DMode.CAM
        self.eval_version = eval_version
        if isinstance(info_file, (list, tuple)):          # already loaded infos
            self.anno_infos = list(info_file)
        else:
            with open(info_file, 'rb') as f:
                self.anno_infos = pickle.load(f)
        self.bbox_code_size = 7

    # ---- the coco file (CocoDataset.load_annotations / get_ann_info / _filter_imgs, CustomDataset._set_group_flag)
    def load_annotations(self, ann_file):
        if isinstance(ann_file, dict):
            coco = ann_file
        else:
            with open(ann_file) as f:
                coco = json.load(f)
        by_name = {c['name']: c['id'] for c in coco['categories']}
        self.cat_ids = [by_name[name] for name in self.CLASSES if name in by_name]
        self.cat2label = {cat_id: i for i, cat_id in enumerate(self.cat_ids)}
        images = sorted(coco['images'], key=lambda im: im['id'])
        self.img_ids = [im['id'] for im in images]
        assert len(set(self.img_ids)) == len(self.img_ids), f"Annotation ids in '{ann_file}' are not unique!"
        self.img_to_anns = {i: [] for i in self.img_ids}
        for ann in coco.get('annotations', []):
            self.img_to_anns[ann['image_id']].append(ann)
        data_infos = []
        for im in images:
            info = dict(im)
            info['filename'] = info['file_name']
            data_infos.append(info)
        return data_infos

    def __len__(self):
        return len(self.data_infos)

    def get_ann_info(self, idx):
        return self._parse_ann_info(self.data_infos[idx], self.img_to_anns[self.data_infos[idx]['id']])

    def _filter_imgs(self, min_size=32):
        """Images with an annotation of a known category and both sides of at least ``min_size`` (without
        ``filter_empty_gt`` only the size counts)."""
        known = set(self.cat_ids)
        ids_in_cat = {i for i, anns in self.img_to_anns.items() if any(a['category_id'] in known for a in anns)}
        valid_inds, valid_img_ids = [], []
        for i, info in enumerate(self.data_infos):
            if self.filter_empty_gt and self.img_ids[i] not in ids_in_cat:
                continue
            if min(info['width'], info['height']) >= min_size:
                valid_inds.append(i)
                valid_img_ids.append(self.img_ids[i])
        self.img_ids = valid_img_ids
        return valid_inds

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)
        for i, info in enumerate(self.data_infos):
            if info['width'] / info['height'] > 1:
                self.flag[i] = 1

    def _parse_ann_info(self, img_info, ann_info):
        """kitti_mono_dataset.py:57-145: the skip rules in their order (``ignore``; no overlap with the image; area <= 0 or a
        side below 1 px; unknown category), ``iscrowd`` boxes to ``bboxes_ignore``, boxes as xyxy, camera boxes with the
        gravity centre as origin."""
        gt_bboxes, gt_labels, gt_bboxes_ignore, gt_masks_ann, gt_bboxes_cam3d, centers2d, depths = [], [], [], [], [], [], []
        for ann in ann_info:
            if ann.get('ignore', False):
                continue
            x1, y1, w, h = ann['bbox']
            inter_w = max(0, min(x1 + w, img_info['width']) - max(x1, 0))
            inter_h = max(0, min(y1 + h, img_info['height']) - max(y1, 0))
            if inter_w * inter_h == 0:
                continue
            if ann['area'] <= 0 or w < 1 or h < 1:
                continue
            if ann['category_id'] not in self.cat_ids:
                continue
            bbox = [x1, y1, x1 + w, y1 + h]
            if ann.get('iscrowd', False):
                gt_bboxes_ignore.append(bbox)
            else:
                gt_bboxes.append(bbox)
                gt_labels.append(self.cat2label[ann['category_id']])
                gt_masks_ann.append(ann.get('segmentation', None))
                gt_bboxes_cam3d.append(np.array(ann['bbox_cam3d']).reshape(-1, ))
                centers2d.append(ann['center2d'][:2])
                depths.append(ann['center2d'][2])
        if gt_bboxes:
            gt_bboxes, gt_labels = np.array(gt_bboxes, dtype=np.float32), np.array(gt_labels, dtype=np.int64)
        else:
            gt_bboxes, gt_labels = np.zeros((0, 4), dtype=np.float32), np.array([], dtype=np.int64)
        if gt_bboxes_cam3d:
            gt_bboxes_cam3d = np.array(gt_bboxes_cam3d, dtype=np.float32)
            centers2d, depths = np.array(centers2d, dtype=np.float32), np.array(depths, dtype=np.float32)
        else:
            gt_bboxes_cam3d = np.zeros((0, self.bbox_code_size), dtype=np.float32)
            centers2d, depths = np.zeros((0, 2), dtype=np.float32), np.zeros((0), dtype=np.float32)
        gt_bboxes_cam3d = CameraInstance3DBoxes(gt_bboxes_cam3d, box_dim=gt_bboxes_cam3d.shape[-1], origin=(0.5, 0.5, 0.5))
        gt_bboxes_ignore = np.array(gt_bboxes_ignore, dtype=np.float32) if gt_bboxes_ignore else np.zeros((0, 4), dtype=np.float32)
        return dict(bboxes=gt_bboxes, labels=gt_labels, gt_bboxes_3d=gt_bboxes_cam3d, gt_labels_3d=copy.deepcopy(gt_labels),
                    centers2d=centers2d, depths=depths, bboxes_ignore=gt_bboxes_ignore, masks=gt_masks_ann,
                    seg_map=img_info['filename'].replace('jpg', 'png'))

    # ---- samples (CustomDataset.__getitem__ / prepare_*_img, NuScenesMonoDataset.pre_pipeline)
    def pre_pipeline(self, results):
        results['img_prefix'], results['seg_prefix'], results['proposal_file'] = self.img_prefix, self.seg_prefix, self.proposal_file
        for registry in KittiDataset_GGA_train._FIELD_REGISTRIES:
            results[registry] = []
        results['box_type_3d'], results['box_mode_3d'] = self.box_type_3d, self.box_mode_3d

    def prepare_train_img(self, idx):
        results = dict(img_info=self.data_infos[idx], ann_info=self.get_ann_info(idx))
        self.pre_pipeline(results)
        return self.pipeline(results)

    def prepare_test_img(self, idx):
        results = dict(img_info=self.data_infos[idx])
        self.pre_pipeline(results)
        return self.pipeline(results)

    def _rand_another(self, idx):
        return np.random.choice(np.where(self.flag == self.flag[idx])[0])

    def __getitem__(self, idx):
        if self.test_mode:
            return self.prepare_test_img(idx)
        while True:
            data = self.prepare_train_img(idx)
            if data is None:
                idx = self._rand_another(idx)
                continue
            return data

    # ---- results of a test run -> KITTI annotations -> AP / submission files (kitti_mono_dataset.py:147-570)
    def format_results(self, outputs, pklfile_prefix=None, submission_prefix=None, device=None):
        """``device``: where ``bbox2result_kitti`` formats (None = the host loop)."""
        tmp_dir = None
        if pklfile_prefix is None:
            tmp_dir = tempfile.TemporaryDirectory()
            pklfile_prefix = os.path.join(tmp_dir.name, 'results')
        if not isinstance(outputs[0], dict):
            result_files = self.bbox2result_kitti2d(outputs, self.CLASSES, pklfile_prefix, submission_prefix)
        elif 'pts_bbox' in outputs[0] or 'img_bbox' in outputs[0] or 'img_bbox2d' in outputs[0]:
            result_files = dict()
            for name in outputs[0]:
                results_ = [out[name] for out in outputs]
                sub = submission_prefix + name if submission_prefix is not None else None
                if '2d' in name:
                    result_files[name] = self.bbox2result_kitti2d(results_, self.CLASSES, pklfile_prefix + name, sub)
                else:
                    result_files[name] = self.bbox2result_kitti(results_, self.CLASSES, pklfile_prefix + name, sub, device=device)
        else:
            result_files = self.bbox2result_kitti(outputs, self.CLASSES, pklfile_prefix, submission_prefix, device=device)
        return result_files, tmp_dir

    def evaluate(self, results, metric=None, logger=None, pklfile_prefix=None, submission_prefix=None, show=False, out_dir=None,
                 pipeline=None, device='cuda:0'):
        """KITTI AP against the ``annos`` of ``anno_infos``; every result name (``img_bbox``, ``img_bbox2d``) gets its own
        call of ``kitti_eval`` - names with ``2d`` only the 2D boxes - and the keys ``{name}/{ap_type}``, rounded to four
        decimals. ``show`` / ``out_dir`` (visualisation) are not part of this repository: refused."""
        if show or out_dir:
            raise NotImplementedError('evaluate(show=..., out_dir=...): visualisation of the results is out of scope')
        from .kitti_eval import kitti_eval
        result_files, tmp_dir = self.format_results(results, pklfile_prefix, device=device)
        gt_annos = [info['annos'] for info in self.anno_infos]
        if isinstance(result_files, dict):
            ap_dict = dict()
            for name, result_files_ in result_files.items():
                eval_types = ['bbox'] if '2d' in name else ['bbox', 'bev', '3d']
                ap_result_str, ap_dict_ = kitti_eval(gt_annos, result_files_, self.CLASSES, eval_types=eval_types, device=device)
                for ap_type, ap in ap_dict_.items():
                    ap_dict[f'{name}/{ap_type}'] = float('{:.4f}'.format(ap))
                KittiDataset_GGA_train._log(f'Results of {name}:\n' + ap_result_str, logger)
        else:
            eval_types = ['bbox'] if metric == 'img_bbox2d' else ['bbox', 'bev', '3d']
            ap_result_str, ap_dict = kitti_eval(gt_annos, result_files, self.CLASSES, eval_types=eval_types, device=device)
            KittiDataset_GGA_train._log('\n' + ap_result_str, logger)
        if tmp_dir is not None:
            tmp_dir.cleanup()
        return ap_dict

    @staticmethod
    def _dump(det_annos, pklfile_prefix):
        if pklfile_prefix is not None:
            out = pklfile_prefix if pklfile_prefix.endswith(('.pkl', '.pickle')) else f'{pklfile_prefix}.pkl'
            with open(out, 'wb') as f:
                pickle.dump(det_annos, f)

    def bbox2result_kitti(self, net_outputs, class_names, pklfile_prefix=None, submission_prefix=None, device=None):
        """``device=None``: the per-frame host loop (``convert_valid_bboxes`` on CPU tensors). A device: all frames in one
        launch of ``kitti_format.format_kitti_dets_cam`` - the same annos to float32 rounding; ``GGA_KITTI_FORMAT=0`` in the
        environment keeps the host loop whatever ``device`` says."""
        assert len(net_outputs) == len(self.anno_infos), 'invalid list length of network outputs'
        if submission_prefix is not None:
            os.makedirs(submission_prefix, exist_ok=True)
        on_device = None
        if device is not None:
            from . import kitti_format
            if kitti_format.enabled():
                on_device = kitti_format.format_kitti_dets_cam(net_outputs, self.anno_infos, class_names, device)
        det_annos = []
        for idx, pred_dicts in enumerate(net_outputs):
            info = self.anno_infos[idx]
            sample_idx = info['image']['image_idx']
            if on_device is not None:
                anno = on_device[idx]
                KittiDataset_GGA_train._write_submission(anno, sample_idx, submission_prefix)
                det_annos.append(anno)
                continue
            image_shape = info['image']['image_shape'][:2]
            box_dict = self.convert_valid_bboxes(pred_dicts, info)
            n = len(box_dict['bbox'])
            if n:
                cam = np.asarray(box_dict['box3d_camera'])
                bbox = np.array(box_dict['bbox']).reshape(n, 4)
                bbox[:, 2:] = np.minimum(bbox[:, 2:], image_shape[::-1])
                bbox[:, :2] = np.maximum(bbox[:, :2], [0, 0])
                anno = dict(name=np.array([class_names[int(label)] for label in box_dict['label_preds']]),
                            truncated=np.zeros(n), occluded=np.zeros(n, dtype=np.int64),
                            alpha=-np.arctan2(cam[:, 0], cam[:, 2]) + cam[:, 6], bbox=bbox, dimensions=cam[:, 3:6],
                            location=cam[:, :3], rotation_y=cam[:, 6], score=np.asarray(box_dict['scores']))
            else:
                anno = _empty_anno()
            KittiDataset_GGA_train._write_submission(anno, sample_idx, submission_prefix)
            anno['sample_idx'] = np.array([sample_idx] * len(anno['score']), dtype=np.int64)
            det_annos.append(anno)
        self._dump(det_annos, pklfile_prefix)
        return det_annos

    def bbox2result_kitti2d(self, net_outputs, class_names, pklfile_prefix=None, submission_prefix=None):
        """kitti_mono_dataset.py:386-495: per frame a list over classes of [n, 5] arrays (x1, y1, x2, y2, score)."""
        assert len(net_outputs) == len(self.anno_infos), 'invalid list length of network outputs'
        det_annos = []
        for i, bboxes_per_sample in enumerate(net_outputs):
            sample_idx = self.anno_infos[i]['image']['image_idx']
            anno = dict(name=[], truncated=[], occluded=[], alpha=[], bbox=[], dimensions=[], location=[], rotation_y=[], score=[])
            num_example = 0
            for label in range(len(bboxes_per_sample)):
                bbox = bboxes_per_sample[label]
                for k in range(bbox.shape[0]):
                    anno['name'].append(class_names[int(label)])
                    anno['truncated'].append(0.0)
                    anno['occluded'].append(0)
                    anno['alpha'].append(-10)
                    anno['bbox'].append(bbox[k, :4])
                    anno['dimensions'].append(np.zeros(shape=[3], dtype=np.float32))
                    anno['location'].append(np.ones(shape=[3], dtype=np.float32) * (-1000.0))
                    anno['rotation_y'].append(0.0)
                    anno['score'].append(bbox[k, 4])
                    num_example += 1
            anno = _empty_anno() if num_example == 0 else {k: np.stack(v) for k, v in anno.items()}
            anno['sample_idx'] = np.array([sample_idx] * num_example, dtype=np.int64)
            det_annos.append(anno)
        self._dump(det_annos, pklfile_prefix)
        if submission_prefix is not None:
            os.makedirs(submission_prefix, exist_ok=True)
            for i, anno in enumerate(det_annos):
                sample_idx = self.anno_infos[i]['image']['image_idx']
                with open(f'{submission_prefix}/{sample_idx:06d}.txt', 'w') as f:
                    bbox, loc, dims = anno['bbox'], anno['location'], anno['dimensions'][::-1]          # lhw -> hwl
                    for idx in range(len(bbox)):
                        print('{} -1 -1 {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f} {:4f}'.format(
                            anno['name'][idx], anno['alpha'][idx], *bbox[idx], *dims[idx], *loc[idx], anno['rotation_y'][idx],
                            anno['score'][idx]), file=f)
        return det_annos

    def convert_valid_bboxes(self, box_dict, info):
        """kitti_mono_dataset.py:497-569: the detections whose projected 2D box meets the image. The reference also converts
        the boxes to the LiDAR frame (``box3d_lidar``; nothing reads it) - kept here, left out on the device."""
        box_preds, scores, labels = box_dict['boxes_3d'], box_dict['scores_3d'], box_dict['labels_3d']
        sample_idx = info['image']['image_idx']
        if len(box_preds) == 0:
            return dict(bbox=np.zeros([0, 4]), box3d_camera=np.zeros([0, 7]), scores=np.zeros([0]), label_preds=np.zeros([0, 4]),
                        sample_idx=sample_idx)
        rect = info['calib']['R0_rect'].astype(np.float32)
        Trv2c = info['calib']['Tr_velo_to_cam'].astype(np.float32)
        P2 = box_preds.tensor.new_tensor(info['calib']['P2'].astype(np.float32))
        img_shape = info['image']['image_shape']
        box_preds_lidar = camera_boxes_to_lidar(box_preds.tensor.numpy(), np.linalg.inv(rect @ Trv2c))
        box_corners_in_image = points_cam2img(box_preds.corners, P2)
        minxy, maxxy = torch.min(box_corners_in_image, dim=1)[0], torch.max(box_corners_in_image, dim=1)[0]
        box_2d_preds = torch.cat([minxy, maxxy], dim=1)
        image_shape = box_preds.tensor.new_tensor(img_shape)
        valid_inds = ((box_2d_preds[:, 0] < image_shape[1]) & (box_2d_preds[:, 1] < image_shape[0]) &
                      (box_2d_preds[:, 2] > 0) & (box_2d_preds[:, 3] > 0))
        if valid_inds.sum() > 0:
            return dict(bbox=box_2d_preds[valid_inds, :].numpy(), box3d_camera=box_preds.tensor[valid_inds].numpy(),
                        box3d_lidar=box_preds_lidar[valid_inds].numpy(), scores=scores[valid_inds].numpy(),
                        label_preds=labels[valid_inds].numpy(), sample_idx=sample_idx)
        return dict(bbox=np.zeros([0, 4]), box3d_camera=np.zeros([0, 7]), box3d_lidar=np.zeros([0, 7]), scores=np.zeros([0]),
                    label_preds=np.zeros([0, 4]), sample_idx=sample_idx)
