#!/usr/bin/env python
"""The mono3d test run (configs/gga/gga_pdg.py and gga_pdg_tta.py: ResNet-101 PGD, random weights) on a synthetic KITTI-size
tree (375 x 1242 frames), at 12 frames and at 1 frame per batch:

* ``plain``: the test run without TTA, ``PGDHead.get_bboxes`` as the loop over images (``GGA_MONO3D_DETECT_BATCHED=0`` - the
  parent commit's ``simple_test``) against the whole-batch detect;
* ``tta``: with the flip view, the maps merged by the eager restatement of the reference (``GGA_MONO3D_TTA_MERGE=0``) against
  ``gga_mono3d_tta_merge``, both over the batched detect; and the loop + eager pair.

The batches are collated beforehand (decoding is the loader workers' work); a pass is ``to_step_inputs`` + the detector's
``forward_test`` for every batch, timed by the host clock around a pass that ends in a synchronise; frames/s is the median of
``--reps`` passes after a warm-up pass. ``detect_ms`` / ``merge_ms``: the median host-clock time of that stage alone on one
batch's head output (synchronised before and after). ``upload_bytes``: what crosses to the device per batch of images.
Prints one JSON line per case.

    python tools_dev/bench_mono3d_test.py [--frames 24] [--reps 3] [--batches 12 1]"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch
    from gga_amd import Config, build_model, synthetic
    from gga_amd import functional as F
    from gga_amd import loader as LD
    from gga_amd.kitti_converter_mono import export_2d_annotation
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[12, 1])
    ap.add_argument('--score-thr', type=float, default=None, help='test_cfg.score_thr (default: the config\'s)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    os.environ['GGA_MONO_IMAGE_DEVICE'] = '1'
    with tempfile.TemporaryDirectory() as root:
        info_path, test_path = synthetic.write_kitti_mono_tree(root, args.frames, img_hw=(375, 1242), seed=77)
        json_path = export_2d_annotation(root, info_path)
        cfgs = {}
        for name, file in (('plain', 'gga_pdg.py'), ('tta', 'gga_pdg_tta.py')):
            cfg = Config.fromfile(os.path.join(REPO, 'configs', 'gga', file))
            cfg.data['val'].update(data_root=root + '/', img_prefix=root + '/', ann_file=json_path, info_file=info_path)
            cfgs[name] = cfg
        torch.manual_seed(0)
        model = build_model(cfgs['plain'].model).to(dev)
        model.init_weights()
        synthetic.damp_random_backbone(model)
        model.eval()
        if args.score_thr is not None:
            model.bbox_head.test_cfg['score_thr'] = args.score_thr
        datasets = {name: LD.build_dataset(copy.deepcopy(cfg.data['val'])) for name, cfg in cfgs.items()}
        for per_batch in args.batches:
            for name, ds in datasets.items():
                samples = [ds[i] for i in range(args.frames)]
                batches = [LD.collate(samples[i:i + per_batch], per_batch, packed=True) for i in range(0, args.frames, per_batch)]
                img0 = batches[0]['img'][0].data[0]
                upload = int(img0.buffer.numel())
                with torch.no_grad():
                    data = LD.to_step_inputs(batches[0], dev)
                    outs = (model.tta_head_outputs(data['img'], data['img_metas']) if name == 'tta' else
                            model.bbox_head(model.extract_feat(data['img'][0])))
                metas = data['img_metas'][0]

                def stage(fn, reps=7):
                    ts = []
                    for _ in range(reps):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        out = fn()
                        torch.cuda.synchronize()
                        ts.append(1e3 * (time.perf_counter() - t))
                    return round(statistics.median(ts[2:]), 3), out

                merge_ms, merged = {}, outs
                if name == 'tta':
                    merge_ms['eager'], _ = stage(lambda: model.tta_merge_eager(outs, len(metas)))
                    merge_ms['fused'], merged = stage(lambda: F.mono3d_tta_merge(outs, len(metas)))
                detect_ms, dets = {}, None
                for key, env in (('loop', '0'), ('batched', '1')):
                    os.environ['GGA_MONO3D_DETECT_BATCHED'] = env
                    detect_ms[key], dets = stage(lambda: model.bbox_head.get_bboxes(*merged, metas, rescale=True))
                cases = [('loop', '0', '1'), ('batched', '1', '1')] if name == 'plain' else \
                        [('loop+eager', '0', '0'), ('batched+eager', '1', '0'), ('batched+fused', '1', '1')]
                for label, batched, merge in cases:
                    os.environ['GGA_MONO3D_DETECT_BATCHED'], os.environ['GGA_MONO3D_TTA_MERGE'] = batched, merge
                    passes = []
                    for rep in range(args.reps + 1):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        n = 0
                        with torch.no_grad():
                            for batch in batches:
                                n += len(model(return_loss=False, rescale=True, **LD.to_step_inputs(batch, dev)))
                        torch.cuda.synchronize()
                        passes.append(args.frames / (time.perf_counter() - t))
                        assert n == args.frames
                    print(json.dumps(dict(run=name, frames_per_batch=per_batch, path=label, frames_per_s=round(statistics.median(passes[1:]), 2),
                                          frames_per_s_passes=[round(p, 2) for p in passes[1:]], detect_ms_per_batch=detect_ms,
                                          merge_ms_per_batch=merge_ms, upload_bytes_per_batch=upload,
                                          detections_first_batch=[len(d[1]) for d in dets])), flush=True)
        os.environ.pop('GGA_MONO3D_DETECT_BATCHED', None), os.environ.pop('GGA_MONO3D_TTA_MERGE', None)


if __name__ == '__main__':
    main()
