#!/usr/bin/env python
"""``python tools/test.py <config> <checkpoint> [--eval mAP] [--out results.pkl] [--eval-options k=v ...]`` - the test entry of the
reference (tools/test.py): the detector with the checkpoint's weights runs over ``cfg.data.test`` in test mode
(``apis.single_gpu_test``, or ``multi_gpu_test`` with ``--launcher pytorch`` and one process per GPU), the raw results go to
``--out`` and / or to the dataset's ``evaluate`` - for ``SUNRGBDDataset`` the mAP / mAR table at IoU 0.25 and 0.5, for the KITTI
datasets what their ``evaluate`` does. ``--eval`` names are handed on as ``metric``; ``--eval-options`` are further keyword
arguments of ``evaluate`` (e.g. ``iou_thr=(0.25,0.5,0.75)``). ``--format-only`` evaluates nothing: the results go through
``dataset.format_results(outputs, **eval_options)``, e.g. ``--eval-options submission_prefix=./pgd_results`` for the KITTI
submission files of a ``KittiMonoDataset`` test split."""
import argparse
import ast
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description='Test (and evaluate) a detector')
    ap.add_argument('config')
    ap.add_argument('checkpoint')
    ap.add_argument('--out', help='pickle file for the raw results')
    ap.add_argument('--eval', nargs='+', help='evaluation metrics, e.g. mAP')
    ap.add_argument('--eval-options', nargs='+', default=[], help='key=value arguments of dataset.evaluate() / format_results()')
    ap.add_argument('--format-only', action='store_true', help='format the results (dataset.format_results) without evaluating them')
    ap.add_argument('--gpu-id', type=int, default=0)
    ap.add_argument('--launcher', choices=['none', 'pytorch'], default='none')
    ap.add_argument('--tmpdir', help='shared directory the ranks\' results are collected through (default: a temporary one)')
    ap.add_argument('--gpu-collect', action='store_true', help='collect the ranks\' results through the process group instead')
    ap.add_argument('--local_rank', '--local-rank', type=int, default=0)
    args = ap.parse_args()
    os.environ.setdefault('LOCAL_RANK', str(args.local_rank))
    if not (args.out or args.eval or args.format_only):
        ap.error('nothing to do: give --out, --eval and / or --format-only')
    if args.eval and args.format_only:
        ap.error('--eval and --format-only cannot be both specified')
    from gga_amd import Config
    from gga_amd.apis import generate_pseudo_labels
    from gga_amd.train import setup_multi_processes
    cfg = Config.fromfile(args.config)
    setup_multi_processes(cfg)
    opts = {}
    for kv in args.eval_options:
        k, v = kv.split('=', 1)
        try:
            opts[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            opts[k] = v
    distributed = args.launcher != 'none'
    rank, gpu = 0, args.gpu_id
    if distributed:
        import torch
        from gga_amd.train import init_dist
        rank, _, local_rank = init_dist()
        gpu = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(gpu)
    # the flow of apis.generate_pseudo_labels is the generic one: dataset and loader from cfg.data.test, the detector with the
    # checkpoint's weights, single_gpu_test / multi_gpu_test, --out, dataset.evaluate on rank 0
    _, result = generate_pseudo_labels(cfg, args.checkpoint, out=args.out, eval_metrics=args.eval, eval_options=opts, device=f'cuda:{gpu}',
                                       distributed=distributed, tmpdir=args.tmpdir, gpu_collect=args.gpu_collect, format_only=args.format_only)
    if rank == 0 and result is not None:
        print(result)
    if distributed:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
