"""gga_amd — MI355X-native implementation of the GGA training hot path.

Host side mirrors the reference's mmdet3d plugin surface (registry names,
constructor arguments, forward signatures); the data-movement-bound stages
run as hand-written HIP kernels for gfx950 behind a C-ABI shared library
(include/gga_hip.h, gga_amd/csrc/). See DESIGN.md.
"""
__version__ = '0.1.0'

import os as _os

# The dense 2D convolutions of SECOND / SECONDFPN / the CenterHead branches run on MIOpen. On a
# machine without a MIOpen user database the first call of every convolution shape times all
# applicable solvers, including MIOpen's naive reference kernels (0.1-1 s per launch at KITTI
# sizes, 8 launches each): 89 s before the first train step finishes versus 9 s without them,
# with the same solvers chosen and the same step time (tools_dev/miopen_env.sh). They never win,
# so they are left out of the search unless the user has set the variables already. Must happen
# before MIOpen's first use; MIOPEN_FIND_MODE is left alone (mode 2 picks the naive kernels).
for _k in ('MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD', 'MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_BWD',
           'MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_WRW'):
    _os.environ.setdefault(_k, '0')

from . import registry  # noqa: E402,F401
from . import dcn  # noqa: E402,F401  (registers 'DCNv2')
from . import losses, bbox_coders, voxel_encoders, middle_encoders, sparse, sparse_encoder, backbones, dense_heads, anchor_head, detectors, mono3d_heads, mono3d_detectors, fcaf3d  # noqa: E402,F401
from .config import Config  # noqa: E402,F401
from .registry import build_detector, build_model  # noqa: E402,F401
from .pseudo_labels import pseudo_label_matching_kitti  # noqa: E402,F401
from . import datasets  # noqa: E402,F401  (registers KittiDataset_GGA_train / LoadAnnotations3D)
from . import image_pipelines, kitti_mono  # noqa: E402,F401  (registers KittiMonoDataset and the image transforms of configs/gga/gga_pdg.py)
from . import indoor_datasets  # noqa: E402,F401  (registers SUNRGBDDataset, ScanNetDataset, S3DISDataset)
from . import weight_bank  # noqa: E402,F401  (registers the process-wide optimizer-step hook that invalidates packed weights)
