# PGD tested with flip test-time augmentation: gga_pdg.py (model, training data, schedule unchanged) plus a test pipeline whose
# MultiScaleFlipAug delivers two views per frame, the image and its horizontal mirror. FCOSMono3D.aug_test runs the views of a
# batch as one [2 B] batch, mirrors the flipped view's head maps back and averages them with the original's on the device
# (DESIGN.md §8), then decodes the merged maps like a plain test run.
#   - one scale factor: the views' maps are averaged element by element, which needs equal sizes
#   - as in the reference, test samples carry no centers2d, so the flipped view keeps its cam2img; only view 0's metas are
#     read after the merge
_base_ = './gga_pdg.py'
class_names = ['Pedestrian', 'Cyclist', 'Car']
dataset_type = 'KittiMonoDataset'
data_root = 'data/kitti/'
input_modality = dict(use_lidar=False, use_camera=True)
img_norm_cfg = dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False)
test_pipeline = [
    dict(type='LoadImageFromFileMono3D'),
    dict(type='MultiScaleFlipAug', scale_factor=1.0, flip=True, flip_direction='horizontal',
         transforms=[dict(type='RandomFlip3D'), dict(type='Normalize', **img_norm_cfg), dict(type='Pad', size_divisor=32),
                     dict(type='DefaultFormatBundle3D', class_names=class_names, with_label=False),
                     dict(type='Collect3D', keys=['img'])]),
]
data = dict(val=dict(pipeline=test_pipeline), test=dict(pipeline=test_pipeline))
