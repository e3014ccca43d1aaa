#!/usr/bin/env python
"""``python tools/create_data_gga_retrain_mono.py kitti --root-path ./data/kitti --extra-tag kitti`` - step 3 of the GGA recipe
(tools/create_data_gga_retrain_mono.py of the reference): the coco files ``<tag>_infos_trainval_GGA_pseudo_mono3d.coco.json``
and ``<tag>_infos_test_mono3d.coco.json`` that ``KittiMonoDataset`` (configs/gga/gga_pdg.py) reads, from the pseudo-labelled
info file and the test info file under ``--root-path``."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description='Data converter arg parser')
    ap.add_argument('dataset', metavar='kitti', help='name of the dataset')
    ap.add_argument('--root-path', type=str, default='./data/kitti', help='specify the root path of dataset')
    ap.add_argument('--version', type=str, default='v1.0', help='specify the dataset version, no need for kitti')
    ap.add_argument('--out-dir', type=str, default='./data/kitti', help='name of info pkl')
    ap.add_argument('--extra-tag', type=str, default='kitti')
    args = ap.parse_args()
    if args.dataset != 'kitti':
        ap.error('only the kitti dataset is converted here')
    from gga_amd.kitti_converter_mono import kitti_data_prep
    for path in kitti_data_prep(root_path=args.root_path, info_prefix=args.extra_tag, version=args.version, out_dir=args.out_dir):
        print(f'wrote {path}')


if __name__ == '__main__':
    main()
