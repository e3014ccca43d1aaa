# The sparse (SECOND trunk) GGA config with dynamic voxelization (the reference's configs/dynamic_voxelization/
# dv_second_secfpn_6x8_80e_kitti-3d-car.py voxel layer and encoder): DynamicSimpleVFE averages ALL the points of a voxel.
_base_ = ['./gga_kitti_config.py']
voxel_size = [0.05, 0.05, 0.1]
point_cloud_range = [0, -40, -3, 70.4, 40, 1]

model = dict(
    pts_voxel_layer=dict(_delete_=True, max_num_points=-1, voxel_size=voxel_size, max_voxels=(-1, -1),
                         point_cloud_range=point_cloud_range),
    pts_voxel_encoder=dict(_delete_=True, type='DynamicSimpleVFE', voxel_size=voxel_size,
                           point_cloud_range=point_cloud_range))
