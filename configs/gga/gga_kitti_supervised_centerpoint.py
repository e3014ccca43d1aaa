# The supervised upper bound of the GGA recipe: gga_kitti_retrain_centerpoint.py (same model, pipeline, schedule and
# validation) trained on the ground-truth boxes of kitti_infos_train_GGA.pkl instead of the pseudo labels - the comparison
# partner of every weakly supervised AP.
_base_ = './gga_kitti_retrain_centerpoint.py'
data_root = 'data/kitti/'
data = dict(train=dict(dataset=dict(ann_file=data_root + 'kitti_infos_train_GGA.pkl')))
work_dir = './work_dirs/kitti_supervised_centerpoint'
