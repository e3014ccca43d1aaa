"""In-training validation on the device (``train_detector(validate=True)``, ``gga_amd.train.EvalHook``) on the three-frame tree
of tests/test_loader.py: schedule and outputs, that a validated run trains bit for bit like an unvalidated one, that the
dataset's ``evaluate`` is the direct ``kitti_eval`` of the device-formatted detections, resume, and two ranks."""
import copy
import glob
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from gga_amd import Config
from gga_amd import loader as LD
from gga_amd.train import train_detector
from test_loader import CLASSES, dataset_cfg, kitti_tree, matching_cfg

pytestmark = pytest.mark.gpu
PP_CFG = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_pointpillars_config.py')
SECOND_CFG = os.path.join(REPO, 'configs', 'gga', 'gga_kitti_config.py')
BEST_KEY = 'KITTI/Overall_3D_AP11_moderate'


def validate_cfg(root, infos, which='pp', epochs=2, evaluation=None, work='work'):
    """The PointPillars config, or the reference's sparse config on a quarter of its voxels (0.1 m instead of 0.05 m in x / y:
    grid 704 x 800 x 40, feature map 100 x 88), pointed at the tree: ``data.train`` without the database sampler, ``data.val`` =
    the train dataset class in test mode with the reference's test pipeline."""
    path = PP_CFG if which == 'pp' else SECOND_CFG
    cfg = Config.fromfile(path)
    m = cfg.model
    m.pts_middle_encoder['channels_last'] = True
    if which != 'pp':
        voxel = [0.1, 0.1, 0.1]
        m.pts_voxel_layer['voxel_size'] = voxel
        m.pts_middle_encoder['sparse_shape'] = [41, 800, 704]
        m.pts_bbox_head['bbox_coder']['voxel_size'] = voxel[:2]
        m.train_cfg['pts'].update(grid_size=[704, 800, 40], voxel_size=voxel)
        m.test_cfg['pts']['voxel_size'] = voxel[:2]
    rng = list(m.pts_voxel_layer['point_cloud_range'])
    val = dict(matching_cfg(root, infos, path).data['test'], type='KittiDataset_GGA_train', samples_per_gpu=2)
    cfg.data = dict(samples_per_gpu=3, workers_per_gpu=0, train=dataset_cfg(root, infos, times=1, point_range=rng), val=val)
    cfg.runner = dict(type='EpochBasedRunner', max_epochs=epochs)
    cfg.work_dir, cfg.seed = os.path.join(root, work), 0
    cfg.checkpoint_config = dict(interval=1)
    cfg.evaluation = dict(evaluation if evaluation is not None else dict(interval=1))
    return cfg


def fresh_model(cfg):
    from gga_amd import build_model
    from gga_amd.cnn import to_channels_last
    torch.manual_seed(0)
    model = build_model(cfg.model)
    with torch.no_grad():          # a random-init detector with finite box sizes that reports boxes (tests/test_loader.py)
        for th in model.pts_bbox_head.task_heads:
            for name in ('reg', 'height', 'dim', 'rot'):
                getattr(th, name)[-1].weight.mul_(0.05)
            th.heatmap[-1].bias.fill_(0.5)
    model.CLASSES = tuple(CLASSES)
    return to_channels_last(model.to('cuda:0')).train()


def run_training(cfg, validate, logger=None):
    import random
    from gga_amd import dense_conv
    dense_conv.FELL_BACK = False         # every run starts like a fresh process: an earlier run's range-guard verdict is not inherited
    random.seed(0), np.random.seed(0), torch.manual_seed(0), torch.cuda.manual_seed_all(0)
    model = fresh_model(cfg)
    ds = LD.build_dataset(copy.deepcopy(cfg.data['train']))
    return train_detector(model, ds, cfg, distributed=False, validate=validate, device=torch.device('cuda:0'), logger=logger)


def direct_ap(cfg_val, infos, model, planes=None):
    """``kitti_eval(gt_annos, format_kitti_dets(single_gpu_test(...)))`` with the keys ``evaluate`` gives a ``pts_bbox`` branch."""
    from gga_amd.apis import single_gpu_test
    from gga_amd.kitti_eval import kitti_eval
    from gga_amd.kitti_format import format_kitti_dets
    ds = LD.build_dataset(dict(copy.deepcopy(cfg_val), test_mode=True))
    loader = LD.build_dataloader(ds, samples_per_gpu=2, workers_per_gpu=0, dist=False, shuffle=False)
    outs = single_gpu_test(model, loader, torch.device('cuda:0'), planes=planes)
    dets = format_kitti_dets([o['pts_bbox'] for o in copy.deepcopy(outs)], ds.data_infos, ds.CLASSES, ds.pcd_limit_range, 'cuda:0')
    text, ap = kitti_eval([i['annos'] for i in ds.data_infos], dets, ds.CLASSES, device='cuda:0')
    return ds, outs, ap


def test_validation_schedule_and_outputs(tmp_path):
    infos = kitti_tree(str(tmp_path))
    lines = []
    cfg = validate_cfg(str(tmp_path), infos, epochs=3, evaluation=dict(interval=1, save_best=BEST_KEY))
    val_cfg = copy.deepcopy(cfg.data['val'])
    runner = run_training(cfg, True, logger=lines.append)
    assert [e for e, _ in runner.eval_history] == [1, 2, 3]
    model = runner.raw_model
    assert model.training
    val_cfg.pop('samples_per_gpu')
    _, _, ap = direct_ap(val_cfg, infos, model, planes=runner.planes)
    for _, values in runner.eval_history:
        assert {k[len('pts_bbox/'):] for k in values} == set(ap) and all(k.startswith('pts_bbox/KITTI/') for k in values)
    assert sum('Epoch(val)' in l for l in lines) == 3 and any('Overall' in l for l in lines)        # one line each + the AP table
    best = glob.glob(os.path.join(cfg.work_dir, 'best_*.pth'))
    assert len(best) == 1
    key = 'pts_bbox/' + BEST_KEY
    scores = [v[key] for _, v in runner.eval_history]
    best_epoch = 1 + max(range(3), key=lambda i: (scores[i], -i))           # the first epoch that reached the maximum
    assert os.path.basename(best[0]) == f'best_pts_bbox_KITTI_Overall_3D_AP11_moderate_epoch_{best_epoch}.pth'
    meta = torch.load(best[0], map_location='cpu', weights_only=False)['meta']
    assert meta['hook_msgs'] == dict(best_score=scores[best_epoch - 1], best_ckpt=best[0]) and meta['epoch'] == best_epoch
    assert runner.hook_msgs == meta['hook_msgs']
    # interval 2 from epoch 2 on
    cfg = validate_cfg(str(tmp_path), infos, epochs=4, evaluation=dict(interval=2, start=2), work='work2')
    runner = run_training(cfg, True)
    assert [e for e, _ in runner.eval_history] == [2, 4] and not glob.glob(os.path.join(cfg.work_dir, 'best_*.pth'))


@pytest.mark.parametrize('which', ['pp', 'second'])
def test_validation_leaves_training_alone(which, tmp_path):
    infos = kitti_tree(str(tmp_path))
    states = []
    for validate in (False, True):
        cfg = validate_cfg(str(tmp_path), infos, which, epochs=2, work=f'work{int(validate)}')
        runner = run_training(cfg, validate)
        assert runner.epoch == 2 and len(runner.eval_history) == (2 if validate else 0)
        torch.cuda.synchronize()
        states.append((copy.deepcopy(runner.raw_model.state_dict()), copy.deepcopy(runner.optimizer.state_dict())))
    (m0, o0), (m1, o1) = states
    assert list(m0) == list(m1)
    for k in m0:
        assert m0[k].dtype == m1[k].dtype and m0[k].cpu().numpy().tobytes() == m1[k].cpu().numpy().tobytes(), k
    assert o0['param_groups'] == o1['param_groups'] and list(o0['state']) == list(o1['state'])
    for i in o0['state']:
        for k, v in o0['state'][i].items():
            w = o1['state'][i][k]
            if torch.is_tensor(v):
                assert v.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (i, k)
            else:
                assert v == w, (i, k)


def test_evaluate_agrees_with_a_direct_call(tmp_path):
    infos = kitti_tree(str(tmp_path))
    cfg = validate_cfg(str(tmp_path), infos)
    model = fresh_model(cfg).eval()
    val_cfg = copy.deepcopy(cfg.data['val'])
    val_cfg.pop('samples_per_gpu')
    ds, outs, ap = direct_ap(val_cfg, infos, model)
    assert type(ds).__name__ == 'KittiDataset_GGA_train' and sum(len(o['pts_bbox']['scores_3d']) for o in outs) > 0
    got = ds.evaluate(copy.deepcopy(outs), device='cuda:0')
    assert got == {f'pts_bbox/{k}': float('{:.4f}'.format(v)) for k, v in ap.items()}
    flat = ds.evaluate([o['pts_bbox'] for o in copy.deepcopy(outs)], device='cuda:0')        # a flat list: the dict as it comes
    assert set(flat) == set(ap) and all(flat[k] == ap[k] for k in ap)


def test_resume_carries_the_best_score(tmp_path):
    infos = kitti_tree(str(tmp_path))
    ev = dict(interval=1, save_best=BEST_KEY)
    cfg = validate_cfg(str(tmp_path), infos, epochs=1, evaluation=ev)
    first = run_training(cfg, True)
    ck = os.path.join(cfg.work_dir, 'epoch_1.pth')
    best = glob.glob(os.path.join(cfg.work_dir, 'best_*.pth'))
    assert len(best) == 1 and best[0].endswith('_epoch_1.pth')
    saved = torch.load(ck, map_location='cpu', weights_only=False)
    assert saved['meta']['hook_msgs'] == first.hook_msgs and first.hook_msgs['best_ckpt'] == best[0]
    # no later epoch can beat a best score of 1000: the file stays, the score travels on
    saved['meta']['hook_msgs']['best_score'] = 1000.0
    torch.save(saved, ck)
    cfg = validate_cfg(str(tmp_path), infos, epochs=2, evaluation=ev)
    cfg.resume_from = ck
    second = run_training(cfg, True)
    assert second.epoch == 2 and [e for e, _ in second.eval_history] == [2]
    assert second.hook_msgs == dict(best_score=1000.0, best_ckpt=best[0])
    assert glob.glob(os.path.join(cfg.work_dir, 'best_*.pth')) == best
    meta2 = torch.load(os.path.join(cfg.work_dir, 'epoch_2.pth'), map_location='cpu', weights_only=False)['meta']
    assert meta2['hook_msgs'] == second.hook_msgs
    # a better epoch replaces the file
    saved['meta']['hook_msgs']['best_score'] = -1.0
    torch.save(saved, ck)
    cfg = validate_cfg(str(tmp_path), infos, epochs=2, evaluation=ev)
    cfg.resume_from = ck
    third = run_training(cfg, True)
    now = glob.glob(os.path.join(cfg.work_dir, 'best_*.pth'))
    assert len(now) == 1 and now[0].endswith('_epoch_2.pth') and third.hook_msgs['best_ckpt'] == now[0]


def test_validation_over_two_ranks(tmp_path):
    """Two gloo ranks on the one GPU validate the same weights (tests/_validate_dist_worker.py): rank 0's AP dict is the
    one-process dict; rank 1 gets nothing and writes nothing."""
    infos = kitti_tree(str(tmp_path))
    cfg = validate_cfg(str(tmp_path), infos)
    model = fresh_model(cfg)
    ck = str(tmp_path / 'weights.pth')
    torch.save(dict(meta=dict(epoch=0, iter=0), state_dict=model.state_dict()), ck)
    val_cfg = copy.deepcopy(cfg.data['val'])
    val_cfg.pop('samples_per_gpu')
    ds, outs, _ = direct_ap(val_cfg, infos, model.eval())
    single = ds.evaluate(copy.deepcopy(outs), device='cuda:0')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, GGA_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    out_dir = tmp_path / 'ranks'
    os.makedirs(out_dir)
    run = subprocess.run(['timeout', '-k', '10', '420', sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(REPO, 'tests', '_validate_dist_worker.py'),
                          str(tmp_path), ck, str(out_dir)], env=env, capture_output=True, text=True, timeout=480)
    assert run.returncode == 0 and 'VALIDATE rank 0 done' in run.stdout, (run.stdout[-1500:], run.stderr[-2500:])
    assert sorted(os.listdir(out_dir)) == ['rank0.pkl']
    both = pickle.load(open(out_dir / 'rank0.pkl', 'rb'))
    assert both == single
    assert 'VALIDATE rank 1 values None' in run.stdout
