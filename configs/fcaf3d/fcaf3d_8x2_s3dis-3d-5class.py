# FCAF3D on S3DIS, 5 classes, axis-aligned boxes (reference: configs/fcaf3d/fcaf3d_8x2_s3dis-3d-5class.py over
# configs/fcaf3d/fcaf3d_8x2_scannet-3d-18class.py, configs/_base_/models/fcaf3d.py and configs/_base_/default_runtime.py), with
# the `_base_` chain merged into one file. Areas 1, 2, 3, 4 and 6 train (one info file each, concatenated), area 5 tests.
# tests/test_indoor_datasets.py asserts that its model / optimizer / schedule / pipeline sections equal what the reference's file
# resolves to.
n_points = 100000
class_names = ('table', 'chair', 'sofa', 'bookcase', 'board')
model = dict(
    type='MinkSingleStage3DDetector',
    voxel_size=.01,
    backbone=dict(type='MinkResNet', in_channels=3, depth=34),
    head=dict(
        type='FCAF3DHead', in_channels=(64, 128, 256, 512), out_channels=128, voxel_size=.01, pts_prune_threshold=100000,
        pts_assign_threshold=27, pts_center_threshold=18, n_classes=5, n_reg_outs=6),
    train_cfg=dict(),
    test_cfg=dict(nms_pre=1000, iou_thr=.5, score_thr=.01))

dataset_type = 'S3DISDataset'
data_root = './data/s3dis/'
train_area = [1, 2, 3, 4, 6]
test_area = 5
train_pipeline = [
    dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
    dict(type='LoadAnnotations3D'),
    dict(type='PointSample', num_points=n_points),
    dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-0.087266, 0.087266], scale_ratio_range=[.9, 1.1], translation_std=[.1, .1, .1],
         shift_height=False),
    dict(type='NormalizePointsColor', color_mean=None),
    dict(type='DefaultFormatBundle3D', class_names=class_names),
    dict(type='Collect3D', keys=['points', 'gt_bboxes_3d', 'gt_labels_3d'])]
test_pipeline = [
    dict(type='LoadPointsFromFile', coord_type='DEPTH', shift_height=False, use_color=True, load_dim=6, use_dim=[0, 1, 2, 3, 4, 5]),
    dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, flip=False,
         transforms=[
             dict(type='GlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1., 1.], translation_std=[0, 0, 0]),
             dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
             dict(type='PointSample', num_points=n_points),
             dict(type='NormalizePointsColor', color_mean=None),
             dict(type='DefaultFormatBundle3D', class_names=class_names, with_label=False),
             dict(type='Collect3D', keys=['points'])])]
data = dict(
    samples_per_gpu=8, workers_per_gpu=4,
    train=dict(type='RepeatDataset', times=13,
               dataset=dict(type='ConcatDataset',
                            datasets=[dict(type=dataset_type, data_root=data_root, ann_file=data_root + f's3dis_infos_Area_{i}.pkl',
                                           pipeline=train_pipeline, filter_empty_gt=True, classes=class_names, box_type_3d='Depth')
                                      for i in train_area],
                            separate_eval=False)),
    val=dict(type=dataset_type, data_root=data_root, ann_file=data_root + f's3dis_infos_Area_{test_area}.pkl',
             pipeline=test_pipeline, classes=class_names, test_mode=True, box_type_3d='Depth'),
    test=dict(type=dataset_type, data_root=data_root, ann_file=data_root + f's3dis_infos_Area_{test_area}.pkl',
              pipeline=test_pipeline, classes=class_names, test_mode=True, box_type_3d='Depth'))
# The reference's file and its bases set no `evaluation`: its train entry then builds the evaluation hook with its defaults -
# every epoch, S3DISDataset.evaluate at IoU 0.25 and 0.5. Spelled out here.
evaluation = dict(interval=1)

optimizer = dict(type='AdamW', lr=0.001, weight_decay=0.0001)
optimizer_config = dict(grad_clip=dict(max_norm=10, norm_type=2))
lr_config = dict(policy='step', warmup=None, step=[8, 11])
runner = dict(type='EpochBasedRunner', max_epochs=12)
custom_hooks = [dict(type='EmptyCacheHook', after_iter=True)]
checkpoint_config = dict(interval=1)
log_config = dict(interval=50, hooks=[dict(type='TextLoggerHook'), dict(type='TensorboardLoggerHook')])
dist_params = dict(backend='nccl')
log_level = 'INFO'
work_dir = None
load_from = None
resume_from = None
workflow = [('train', 1)]
