"""The face test of ``gga_frame_point_tests`` / ``gga_points_in_convex_polyhedra`` stated in numpy."""
import numpy as np


def face_test(points, normal, d):
    """float64, elementwise, the kernels' order. points [N, >=3] (float32 widens exactly), normal [P, S, 3], d [P, S]
    -> bool [N, P]: inside iff every face gives < 0."""
    p = np.asarray(points).astype(np.float64)
    a, b, c = (p[:, None, None, k] * normal[None, :, :, k] for k in range(3))
    s = ((a + b) + c) + d[None]
    return (s < 0).all(-1)
