"""Worker of tests/test_validate_gpu.py::test_validation_over_two_ranks: one rank of a 2-rank gloo group on ONE GPU running one
validation pass of ``train.EvalHook`` (``multi_gpu_test`` over the sharded val loader, BatchNorm statistics broadcast first) on
given weights (argv: tree root, checkpoint, output directory); rank 0 writes its AP dict to ``rank0.pkl``, rank 1 nothing."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import pickle

import torch
import torch.distributed as dist

from gga_amd.apis import load_weights
from gga_amd.train import build_eval_hook, init_dist
from test_loader import kitti_tree
from test_validate_gpu import fresh_model, validate_cfg

root, ck, out_dir = sys.argv[1:4]
rank, world, _ = init_dist()
torch.cuda.set_device(0)
infos = kitti_tree(root)
cfg = validate_cfg(root, infos)
model = fresh_model(cfg)
load_weights(model, ck, strict=True)


class _Runner:
    """What the hook reads of a ``train.Runner`` after an epoch."""
    raw_model, device, planes, epoch = model, torch.device('cuda:0'), None, 1
    hook_msgs, eval_history = {}, []


hook = build_eval_hook(cfg, distributed=True)
values = hook.after_train_epoch(_Runner)
assert (values is None) == (rank != 0) and model.training
if rank == 0:
    with open(os.path.join(out_dir, 'rank0.pkl'), 'wb') as f:
        pickle.dump(values, f)
    print('VALIDATE rank 0 done', len(values), flush=True)
else:
    print('VALIDATE rank 1 values', values, flush=True)
dist.barrier()
dist.destroy_process_group()
