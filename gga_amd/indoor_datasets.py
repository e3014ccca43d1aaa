"""``SUNRGBDDataset`` - the dataset of configs/fcaf3d/fcaf3d_8x2_sunrgbd-3d-10class.py (mmdet3d/datasets/sunrgbd_dataset.py over
mmdet3d/datasets/custom_3d.py): constructor keys, ``CLASSES``, the sample dictionaries and ``evaluate`` of the reference.

The info file is the pickle tools/create_data.py of the reference writes (``sunrgbd_infos_{train,val}.pkl``): per frame
``point_cloud`` (``lidar_idx``), ``image`` (``image_idx``, ``image_path``), ``pts_path``, ``calib`` (``K``, ``Rt``) and ``annos``
(``gt_num``, ``name``, ``class``, ``gt_boxes_upright_depth`` [k,7] by gravity centre, ``bbox`` ...). ``evaluate`` hands the
detections of a test run to ``indoor_eval`` (mAP / mAR at the IoU thresholds, on the device when one is given). Image loading,
the 2D evaluation and ``show`` are not part of this tree and raise."""
import os.path as osp
import pickle
import tempfile

import numpy as np

from .fcaf3d import DepthInstance3DBoxes
from .indoor_eval import indoor_eval
from .pipelines import Compose
from .registry import DATASETS


@DATASETS.register_module()
class SUNRGBDDataset:
    CLASSES = ('bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub')

    def __init__(self, data_root, ann_file, pipeline=None, classes=None, modality=dict(use_camera=True, use_lidar=True),
                 box_type_3d='Depth', filter_empty_gt=True, test_mode=False, file_client_args=dict(backend='disk')):
        self.data_root, self.ann_file, self.test_mode, self.modality = data_root, ann_file, test_mode, modality
        self.filter_empty_gt = filter_empty_gt
        if str(box_type_3d).lower() != 'depth':
            raise NotImplementedError(f'SUNRGBDDataset(box_type_3d={box_type_3d!r}): only Depth boxes are supported')
        self.box_type_3d, self.box_mode_3d = DepthInstance3DBoxes, 'Depth'          # get_box_type('Depth'), Box3DMode.DEPTH by name
        self.CLASSES = self.get_classes(classes)
        self.cat2id = {name: i for i, name in enumerate(self.CLASSES)}
        self.data_infos = self.load_annotations(self.ann_file)
        if pipeline is not None:
            self.pipeline = Compose(pipeline)
        if not self.test_mode:
            self._set_group_flag()
        assert 'use_camera' in self.modality and 'use_lidar' in self.modality
        assert self.modality['use_camera'] or self.modality['use_lidar']

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

    def evaluate(self, results, metric=None, iou_thr=(0.25, 0.5), iou_thr_2d=(0.5, ), logger=None, show=False, out_dir=None,
                 pipeline=None, device=None):
        """sunrgbd_dataset.py:226-280 / custom_3d.py:301-351: mAP and mAR of the 3D detections in the indoor protocol.
        ``device``: where the matching runs (None: the GPU when there is one; 'cpu': the host path). -> ``ret_dict``."""
        assert isinstance(results, list), f'Expect results to be list, got {type(results)}.'
        assert len(results) > 0, 'Expect length of results > 0.'
        if not isinstance(results[0], dict):
            raise NotImplementedError('the 2D evaluation (mmdet eval_map) is not part of this tree')
        assert len(results) == len(self.data_infos)
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
