# The pseudo-label matching run (gga_kitti_matching_config.py) with test-time augmentation: the same dataset and evaluation,
# the test pipeline's wrapper set to 3 point scales x horizontal flip = 6 views per frame (see gga_kitti_tta_config.py for
# why the vertical flip is off, why RandomFlip3D gets sync_2d=False, and what test_cfg.pts gains).
_base_ = './gga_kitti_matching_config.py'
dataset_type = 'KittiDataset_GGA_match'
data_root = 'data/kitti/'
class_names = ['Pedestrian', 'Cyclist', 'Car']
point_cloud_range = [0, -40, -3, 70.4, 40, 1]
input_modality = dict(use_lidar=True, use_camera=True)
model = dict(test_cfg=dict(pts=dict(use_rotate_nms=True, max_num=500)))
test_pipeline = [
    dict(type='LoadPointsFromFile', coord_type='LIDAR', load_dim=4, use_dim=4),
    dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=[0.95, 1.0, 1.05], flip=True,
         pcd_horizontal_flip=True, pcd_vertical_flip=False,
         transforms=[dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
                     dict(type='RandomFlip3D', sync_2d=False),
                     dict(type='PointsRangeFilter', point_cloud_range=point_cloud_range),
                     dict(type='DefaultFormatBundle3D', class_names=class_names, with_label=False),
                     dict(type='Collect3D', keys=['points'])])]
_test = dict(type=dataset_type, data_root=data_root, ann_file=data_root + 'kitti_infos_trainval_GGA.pkl', split='training',
             pts_prefix='velodyne_reduced', pipeline=test_pipeline, modality=input_modality, classes=class_names, test_mode=True,
             box_type_3d='LiDAR')
data = dict(val=_test, test=_test)
