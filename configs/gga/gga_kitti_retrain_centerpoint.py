# Supervised CenterPoint on KITTI, second stage of the GGA recipe on the LiDAR side: the trunk and head layout of
# gga_kitti_config.py, trained on the 3D boxes of the pseudo-label file a GGA run wrote
# (tools/generate_pseudo_labels_gga.py -> kitti_infos_trainval_GGA_pseudo.pkl), as gga_pdg.py is on the mono side.
#   - detector 'CenterPoint', head 'CenterHead' (mmdet3d/models/detectors/centerpoint.py, dense_heads/centerpoint_head.py):
#     the heat-map focal loss and a code-weighted L1 on (reg 2, height, dim 3, rot 2) - eight code weights
#   - dataset 'KittiDataset': needs name / location / dimensions / rotation_y / bbox of the annos, no GGA_* field
#   - the boxes follow the points through GlobalRotScaleTrans / RandomFlip3D. ObjectSample / DataBaseSampler (the stock
#     database sampler works on ground-truth boxes; the one in this repository on GGA fields) and ObjectNoise are left out
#   - validated on kitti_infos_val_GGA.pkl: tools/train.py --validate, tools/test.py --eval mAP
# The reference ships no KITTI config for its CenterPoint parts; the schedule is gga_kitti_config.py's.
_base_ = './gga_kitti_config.py'
point_cloud_range = [0, -40, -3, 70.4, 40, 1]
voxel_size = [0.05, 0.05, 0.1]
model = dict(
    type='CenterPoint',
    pts_bbox_head=dict(
        _delete_=True,
        type='CenterHead', in_channels=512,
        tasks=[dict(num_class=1, class_names=['Pedestrian']), dict(num_class=1, class_names=['Cyclist']),
               dict(num_class=1, class_names=['Car'])],
        common_heads=dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2)),
        share_conv_channel=64,
        bbox_coder=dict(type='CenterPointBBoxCoder', post_center_range=point_cloud_range, max_num=100,
                        score_threshold=0.1, out_size_factor=8, voxel_size=voxel_size[:2], code_size=7,
                        pc_range=point_cloud_range[:2]),
        separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3),
        loss_cls=dict(type='GaussianFocalLoss', reduction='mean', alpha=0.),
        loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=0.25),
        norm_bbox=True),
    train_cfg=dict(pts=dict(code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])))

dataset_type = 'KittiDataset'
data_root = 'data/kitti/'
class_names = ['Pedestrian', 'Cyclist', 'Car']
input_modality = dict(use_lidar=True, use_camera=False)
train_pipeline = [
    dict(type='LoadPointsFromFile', coord_type='LIDAR', load_dim=4, use_dim=4),
    dict(type='LoadAnnotations3D', with_bbox_3d=True, with_label_3d=True),
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05]),
    dict(type='PointsRangeFilter', point_cloud_range=point_cloud_range),
    dict(type='ObjectRangeFilter', point_cloud_range=point_cloud_range),
    dict(type='ObjectNameFilter', classes=class_names),
    dict(type='PointShuffle'),
    dict(type='DefaultFormatBundle3D', class_names=class_names),
    dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])]
test_pipeline = [
    dict(type='LoadPointsFromFile', coord_type='LIDAR', load_dim=4, use_dim=4),
    dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=False,
         transforms=[dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
                     dict(type='RandomFlip3D'),
                     dict(type='PointsRangeFilter', point_cloud_range=point_cloud_range),
                     dict(type='DefaultFormatBundle3D', class_names=class_names, with_label=False),
                     dict(type='Collect3D', keys=['points'])])]
_val = dict(type=dataset_type, data_root=data_root, ann_file=data_root + 'kitti_infos_val_GGA.pkl', split='training',
            pts_prefix='velodyne_reduced', pipeline=test_pipeline, modality=input_modality, classes=class_names, test_mode=True,
            box_type_3d='LiDAR')
data = dict(
    samples_per_gpu=32, workers_per_gpu=4,
    train=dict(type='RepeatDataset', times=1,
               dataset=dict(_delete_=True, type=dataset_type, data_root=data_root,
                            ann_file=data_root + 'kitti_infos_trainval_GGA_pseudo.pkl', split='training',
                            pts_prefix='velodyne_reduced', pipeline=train_pipeline, modality=input_modality,
                            classes=class_names, test_mode=False, box_type_3d='LiDAR')),
    val=_val, test=_val)
evaluation = dict(interval=2)
work_dir = './work_dirs/kitti_retrain_centerpoint'
