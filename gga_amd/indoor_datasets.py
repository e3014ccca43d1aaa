"""The indoor datasets of configs/fcaf3d: ``SUNRGBDDataset`` (mmdet3d/datasets/sunrgbd_dataset.py), ``ScanNetDataset``
(scannet_dataset.py:18-255, the detection class) and ``S3DISDataset`` (s3dis_dataset.py:16-155) over one restatement of
mmdet3d/datasets/custom_3d.py (``Indoor3DDataset``): constructor keys, ``CLASSES``, the sample dictionaries and ``evaluate`` of
the reference.

The info files are the pickles tools/create_data.py of the reference writes. SUN RGB-D (``sunrgbd_infos_{train,val}.pkl``): per
frame ``point_cloud`` (``lidar_idx``), ``image`` (``image_idx``, ``image_path``), ``pts_path``, ``calib`` (``K``, ``Rt``) and
``annos`` (``gt_num``, ``name``, ``class``, ``gt_boxes_upright_depth`` [k,7] by gravity centre, ``bbox`` ...). ScanNet
(``scannet_infos_{train,val}.pkl``) and S3DIS (``s3dis_infos_Area_{n}.pkl``): ``point_cloud``, ``pts_path``,
``pts_instance_mask_path``, ``pts_semantic_mask_path`` and ``annos`` with axis-aligned ``gt_boxes_upright_depth`` [k,6]; ScanNet
adds ``axis_align_matrix`` [4,4], which takes the stored points into the frame of the boxes (the ``GlobalAlignment`` step).
``evaluate`` hands the detections of a test run to ``indoor_eval`` (mAP / mAR at the IoU thresholds, on the device when one is
given). Image loading, the 2D evaluation, the segmentation datasets and ``show`` are not part of this tree and raise."""
import os.path as osp
import pickle
import tempfile
import warnings

import numpy as np

from .fcaf3d import DepthInstance3DBoxes
from .indoor_eval import indoor_eval
from .pipelines import Compose
from .registry import DATASETS


class Indoor3DDataset:
    """What the three datasets share (custom_3d.py ``Custom3DDataset``): construction, class names, the pipeline entry points,
    result pickling, the indoor evaluation, indexing with the retry on filtered frames."""
    CLASSES = None

    def __init__(self, data_root, ann_file, pipeline=None, classes=None, modality=None, box_type_3d='Depth', filter_empty_gt=True,
                 test_mode=False, file_client_args=dict(backend='disk')):
        self.data_root, self.ann_file, self.test_mode, self.modality = data_root, ann_file, test_mode, modality
        self.filter_empty_gt = filter_empty_gt
        if str(box_type_3d).lower() != 'depth':
            raise NotImplementedError(f'{type(self).__name__}(box_type_3d={box_type_3d!r}): only Depth boxes are supported')
        self.box_type_3d, self.box_mode_3d = DepthInstance3DBoxes, 'Depth'          # get_box_type('Depth'), Box3DMode.DEPTH by name
        self.CLASSES = self.get_classes(classes)
        self.cat2id = {name: i for i, name in enumerate(self.CLASSES)}
        self.data_infos = self.load_annotations(self.ann_file)
        if pipeline is not None:
            self.pipeline = Compose(pipeline)
        if not self.test_mode:
            self._set_group_flag()

    @classmethod
    def get_classes(cls, classes=None):
        if classes is None:
            return cls.CLASSES
        if isinstance(classes, str):            # a file with one class name per line
            with open(classes) as f:
                return [line.rstrip('\n') for line in f]
        if isinstance(classes, (tuple, list)):
            return classes
        raise ValueError(f'Unsupported type {type(classes)} of classes.')

    def load_annotations(self, ann_file):
        with open(ann_file, 'rb') as f:
            return pickle.load(f)

    def _axis_aligned_ann_info(self, index):
        """``get_ann_info`` of ScanNet and S3DIS: [k,6] boxes by gravity centre -> Depth boxes without yaw, labels, mask paths."""
        info = self.data_infos[index]
        if info['annos']['gt_num'] != 0:
            gt_bboxes_3d = info['annos']['gt_boxes_upright_depth'].astype(np.float32)
            gt_labels_3d = info['annos']['class'].astype(np.int64)
        else:
            gt_bboxes_3d = np.zeros((0, 6), dtype=np.float32)
            gt_labels_3d = np.zeros((0, ), dtype=np.int64)
        gt_bboxes_3d = DepthInstance3DBoxes(gt_bboxes_3d, box_dim=gt_bboxes_3d.shape[-1], with_yaw=False,
                                            origin=(0.5, 0.5, 0.5)).convert_to(self.box_mode_3d)
        return dict(gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d,
                    pts_instance_mask_path=osp.join(self.data_root, info['pts_instance_mask_path']),
                    pts_semantic_mask_path=osp.join(self.data_root, info['pts_semantic_mask_path']))

    def pre_pipeline(self, results):
        for key in ('img_fields', 'bbox3d_fields', 'pts_mask_fields', 'pts_seg_fields', 'bbox_fields', 'mask_fields', 'seg_fields'):
            results[key] = []
        results['box_type_3d'] = self.box_type_3d
        results['box_mode_3d'] = self.box_mode_3d

    def prepare_train_data(self, index):
        input_dict = self.get_data_info(index)
        if input_dict is None:
            return None
        self.pre_pipeline(input_dict)
        example = self.pipeline(input_dict)
        if self.filter_empty_gt and (example is None or ~(example['gt_labels_3d']._data != -1).any()):
            return None
        return example

    def prepare_test_data(self, index):
        input_dict = self.get_data_info(index)
        self.pre_pipeline(input_dict)
        return self.pipeline(input_dict)

    def format_results(self, outputs, pklfile_prefix=None, submission_prefix=None):
        """custom_3d.py:277-299: the results pickled to ``{pklfile_prefix}.pkl`` (a temporary directory without a prefix).
        -> (outputs, the temporary directory or None)."""
        tmp_dir = None
        if pklfile_prefix is None:
            tmp_dir = tempfile.TemporaryDirectory()
            pklfile_prefix = osp.join(tmp_dir.name, 'results')
        with open(f'{pklfile_prefix}.pkl', 'wb') as f:
            pickle.dump(outputs, f)
        return outputs, tmp_dir

    def evaluate(self, results, metric=None, iou_thr=(0.25, 0.5), logger=None, show=False, out_dir=None, pipeline=None, device=None):
        """custom_3d.py:301-351: mAP and mAR of the 3D detections in the indoor protocol. ``device``: where the matching runs
        (None: the GPU when there is one; 'cpu': the host path). -> ``ret_dict``."""
        assert isinstance(results, list), f'Expect results to be list, got {type(results)}.'
        assert len(results) > 0, 'Expect length of results > 0.'
        assert len(results) == len(self.data_infos)
        assert isinstance(results[0], dict), f'Expect elements in results to be dict, got {type(results[0])}.'
        return self._indoor_eval(results, iou_thr, logger, show, out_dir, pipeline, device)

    def _indoor_eval(self, results, iou_thr, logger, show, out_dir, pipeline, device):
        gt_annos = [info['annos'] for info in self.data_infos]
        label2cat = {i: cat_id for i, cat_id in enumerate(self.CLASSES)}
        ret_dict = indoor_eval(gt_annos, results, iou_thr, label2cat, logger=logger, box_type_3d=self.box_type_3d,
                               box_mode_3d=self.box_mode_3d, device=device)
        if show:
            self.show(results, out_dir, pipeline=pipeline)
        return ret_dict

    def show(self, results, out_dir, show=True, pipeline=None):
        raise NotImplementedError('visualisation (open3d / image overlays) is not part of this tree')

    def __len__(self):
        return len(self.data_infos)

    def _rand_another(self, idx):
        pool = np.where(self.flag == self.flag[idx])[0]
        return np.random.choice(pool)

    def __getitem__(self, idx):
        if self.test_mode:
            return self.prepare_test_data(idx)
        while True:
            data = self.prepare_train_data(idx)
            if data is None:
                idx = self._rand_another(idx)
                continue
            return data

    def _set_group_flag(self):
        self.flag = np.zeros(len(self), dtype=np.uint8)


@DATASETS.register_module()
class SUNRGBDDataset(Indoor3DDataset):
    CLASSES = ('bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub')

    def __init__(self, data_root, ann_file, pipeline=None, classes=None, modality=dict(use_camera=True, use_lidar=True),
                 box_type_3d='Depth', filter_empty_gt=True, test_mode=False, file_client_args=dict(backend='disk')):
        super().__init__(data_root, ann_file, pipeline=pipeline, classes=classes, modality=modality, box_type_3d=box_type_3d,
                         filter_empty_gt=filter_empty_gt, test_mode=test_mode, file_client_args=file_client_args)
        assert 'use_camera' in self.modality and 'use_lidar' in self.modality
        assert self.modality['use_camera'] or self.modality['use_lidar']

    def get_data_info(self, index):
        info = self.data_infos[index]
        sample_idx = info['point_cloud']['lidar_idx']
        assert info['point_cloud']['lidar_idx'] == info['image']['image_idx']
        input_dict = dict(sample_idx=sample_idx)
        if self.modality['use_lidar']:
            pts_filename = osp.join(self.data_root, info['pts_path'])
            input_dict['pts_filename'] = pts_filename
            input_dict['file_name'] = pts_filename
        if self.modality['use_camera']:
            img_filename = osp.join(osp.join(self.data_root, 'sunrgbd_trainval'), info['image']['image_path'])
            input_dict['img_prefix'] = None
            input_dict['img_info'] = dict(filename=img_filename)
            calib = info['calib']
            # follow Coord3DMode.convert_point
            rt_mat = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]) @ calib['Rt'].transpose(1, 0)
            input_dict['depth2img'] = calib['K'] @ rt_mat
        if not self.test_mode:
            annos = self.get_ann_info(index)
            input_dict['ann_info'] = annos
            if self.filter_empty_gt and len(annos['gt_bboxes_3d']) == 0:
                return None
        return input_dict

    def get_ann_info(self, index):
        info = self.data_infos[index]
        if info['annos']['gt_num'] != 0:
            gt_bboxes_3d = info['annos']['gt_boxes_upright_depth'].astype(np.float32)
            gt_labels_3d = info['annos']['class'].astype(np.int64)
        else:
            gt_bboxes_3d = np.zeros((0, 7), dtype=np.float32)
            gt_labels_3d = np.zeros((0, ), dtype=np.int64)
        gt_bboxes_3d = DepthInstance3DBoxes(gt_bboxes_3d, origin=(0.5, 0.5, 0.5)).convert_to(self.box_mode_3d)
        anns_results = dict(gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d)
        if self.modality['use_camera']:
            if info['annos']['gt_num'] != 0:
                gt_bboxes_2d = info['annos']['bbox'].astype(np.float32)
            else:
                gt_bboxes_2d = np.zeros((0, 4), dtype=np.float32)
            anns_results['bboxes'] = gt_bboxes_2d
            anns_results['labels'] = gt_labels_3d
        return anns_results

    def evaluate(self, results, metric=None, iou_thr=(0.25, 0.5), iou_thr_2d=(0.5, ), logger=None, show=False, out_dir=None,
                 pipeline=None, device=None):
        """sunrgbd_dataset.py:226-280 / custom_3d.py:301-351: mAP and mAR of the 3D detections in the indoor protocol.
        ``device``: where the matching runs (None: the GPU when there is one; 'cpu': the host path). -> ``ret_dict``."""
        assert isinstance(results, list), f'Expect results to be list, got {type(results)}.'
        assert len(results) > 0, 'Expect length of results > 0.'
        if not isinstance(results[0], dict):
            raise NotImplementedError('the 2D evaluation (mmdet eval_map) is not part of this tree')
        assert len(results) == len(self.data_infos)
        return self._indoor_eval(results, iou_thr, logger, show, out_dir, pipeline, device)


@DATASETS.register_module()
class ScanNetDataset(Indoor3DDataset):
    """scannet_dataset.py:18-255: 18 classes, axis-aligned boxes, the axis-align matrix of every scan carried to the pipeline
    (in test mode too: the points have to be aligned before the detector sees them)."""
    CLASSES = ('cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk', 'curtain',
               'refrigerator', 'showercurtrain', 'toilet', 'sink', 'bathtub', 'garbagebin')

    def __init__(self, data_root, ann_file, pipeline=None, classes=None, modality=dict(use_camera=False, use_depth=True),
                 box_type_3d='Depth', filter_empty_gt=True, test_mode=False, **kwargs):
        super().__init__(data_root, ann_file, pipeline=pipeline, classes=classes, modality=modality, box_type_3d=box_type_3d,
                         filter_empty_gt=filter_empty_gt, test_mode=test_mode, **kwargs)
        assert 'use_camera' in self.modality and 'use_depth' in self.modality
        assert self.modality['use_camera'] or self.modality['use_depth']

    def get_data_info(self, index):
        info = self.data_infos[index]
        sample_idx = info['point_cloud']['lidar_idx']
        pts_filename = osp.join(self.data_root, info['pts_path'])
        input_dict = dict(sample_idx=sample_idx)
        if self.modality['use_depth']:
            input_dict['pts_filename'] = pts_filename
            input_dict['file_name'] = pts_filename
        if self.modality['use_camera']:
            raise NotImplementedError('ScanNetDataset(use_camera=True): image loading is not part of this tree')
        if not self.test_mode:
            annos = self.get_ann_info(index)
            input_dict['ann_info'] = annos
            if self.filter_empty_gt and ~(annos['gt_labels_3d'] != -1).any():
                return None
        return input_dict

    def get_ann_info(self, index):
        anns_results = self._axis_aligned_ann_info(index)
        anns_results['axis_align_matrix'] = self._get_axis_align_matrix(self.data_infos[index])
        return anns_results

    def prepare_test_data(self, index):
        input_dict = self.get_data_info(index)
        input_dict['ann_info'] = dict(axis_align_matrix=self._get_axis_align_matrix(self.data_infos[index]))
        self.pre_pipeline(input_dict)
        return self.pipeline(input_dict)

    @staticmethod
    def _get_axis_align_matrix(info):
        """The [4,4] float32 matrix of the scan, or the identity (with a warning) for an info file written without it."""
        if 'axis_align_matrix' in info['annos'].keys():
            return info['annos']['axis_align_matrix'].astype(np.float32)
        warnings.warn('axis_align_matrix is not found in ScanNet data info, please use new pre-process scripts to re-generate '
                      'ScanNet data')
        return np.eye(4).astype(np.float32)


@DATASETS.register_module()
class S3DISDataset(Indoor3DDataset):
    """s3dis_dataset.py:16-155: one area of S3DIS, 5 classes, axis-aligned boxes; the train areas are put together by
    ``ConcatDataset`` in the config."""
    CLASSES = ('table', 'chair', 'sofa', 'bookcase', 'board')

    def get_ann_info(self, index):
        return self._axis_aligned_ann_info(index)

    def get_data_info(self, index):
        info = self.data_infos[index]
        input_dict = dict(pts_filename=osp.join(self.data_root, info['pts_path']))
        if not self.test_mode:
            annos = self.get_ann_info(index)
            input_dict['ann_info'] = annos
            if self.filter_empty_gt and ~(annos['gt_labels_3d'] != -1).any():
                return None
        return input_dict
