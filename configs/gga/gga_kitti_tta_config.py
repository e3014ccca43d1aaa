# GGA on KITTI tested with test-time augmentation: gga_kitti_config.py (model, training data, schedule unchanged) plus a test
# section whose MultiScaleFlipAug3D wrapper delivers 3 point scales x horizontal flip = 6 views per frame, in the wrapper's
# loop order (scale outer, flip inner). GGA.aug_test runs the views of a batch as one batch, merges the head maps of a scale's
# views on the device and the boxes of the three scales by BEV NMS.
#   - the x range of KITTI is [0, 70.4]: a vertical flip (x -> -x) would send every point out of range, so only the
#     horizontal one (y -> -y, range [-40, 40]) is on; GGA.aug_test refuses a flip across an asymmetric range
#   - RandomFlip3D(sync_2d=False): with the default sync_2d=True the wrapper's flip=True would flip EVERY view
#   - test_cfg.pts gains what the box merge reads: use_rotate_nms and max_num (= max_per_img)
_base_ = './gga_kitti_config.py'
dataset_type = 'KittiDataset_GGA_train'
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
