#!/usr/bin/env python
"""``python tools/create_data_gga.py kitti --root-path ./data/kitti --out-dir ./data/kitti --extra-tag kitti`` - step 1 of the
GGA recipe (tools/create_data_gga.py of the reference): from an unpacked KITTI root (``ImageSets/``, ``training/``,
``testing/``) to ``<tag>_infos_{train,val,trainval}_GGA.pkl``, ``<tag>_infos_test.pkl``, ``{training,testing}/velodyne_reduced/``,
the four ``*_mono3d.coco.json``, ``<tag>_gt_database_GGA/`` and ``<tag>_dbinfos_train_GGA.pkl``.
``--seed`` re-seeds the RANSAC ground fit per frame (seed + frame id), so that a run can be repeated; ``--resume`` keeps the
per-frame pickles of an interrupted run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description='Data converter arg parser')
    ap.add_argument('dataset', metavar='kitti', help='name of the dataset')
    ap.add_argument('--root-path', type=str, default='./data/kitti', help='specify the root path of dataset')
    ap.add_argument('--version', type=str, default='v1.0', help='specify the dataset version, no need for kitti')
    ap.add_argument('--with-plane', action='store_true', help='Whether to use plane information for kitti.')
    ap.add_argument('--out-dir', type=str, default='./data/kitti', help='name of info pkl')
    ap.add_argument('--extra-tag', type=str, default='kitti')
    ap.add_argument('--workers', type=int, default=4, help='number of threads to be used')
    ap.add_argument('--seed', type=int, default=None, help='seed of the ground fit: frame i draws from seed + i')
    ap.add_argument('--resume', action='store_true', help='keep the per-frame label files that exist already')
    args = ap.parse_args()
    if args.dataset != 'kitti':
        ap.error('only the kitti dataset is converted here')
    from gga_amd.kitti_converter import kitti_data_prep
    kitti_data_prep(root_path=args.root_path, info_prefix=args.extra_tag, version=args.version, out_dir=args.out_dir,
                    with_plane=args.with_plane, workers=args.workers, seed=args.seed, resume=args.resume)


if __name__ == '__main__':
    main()
