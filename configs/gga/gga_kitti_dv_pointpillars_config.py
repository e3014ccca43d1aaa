# The PointPillars GGA config with dynamic voxelization (the reference's configs/dynamic_voxelization/
# dv_pointpillars_secfpn_6x8_160e_kitti-3d-car.py voxel layer and encoder): no cap of 32 points per pillar or
# 16 000 pillars per frame, every point in range contributes.
_base_ = ['./gga_kitti_pointpillars_config.py']
voxel_size = [0.16, 0.16, 4]
point_cloud_range = [0, -39.68, -3, 69.12, 39.68, 1]

model = dict(
    pts_voxel_layer=dict(_delete_=True, max_num_points=-1, voxel_size=voxel_size, max_voxels=(-1, -1),
                         point_cloud_range=point_cloud_range),
    pts_voxel_encoder=dict(_delete_=True, type='DynamicPillarFeatureNet', in_channels=4, feat_channels=[64],
                           with_distance=False, voxel_size=voxel_size, point_cloud_range=point_cloud_range))
