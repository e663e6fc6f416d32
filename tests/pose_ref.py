"""R(q) of a camera-to-world pose (qw qx qy qz tx ty tz) as the library's float64 kernels form it (m4d_rot64 in
csrc/m4d_common.h: get_rot_mat's expressions, one IEEE rounding per operation), restated once for every numpy reference."""
import numpy as np

D = np.float64


def rot(q):
    """q [4] (or a pose [7]) -> R as a 3 x 3 nested tuple of float64 scalars."""
    w, x, y, z = (D(v) for v in q[:4])
    tx, ty, tz = D(2.0) * x, D(2.0) * y, D(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return ((D(1.0) - (tyy + tzz), txy - twz, txz + twy), (txy + twz, D(1.0) - (txx + tzz), tyz - twx),
            (txz - twy, tyz + twx, D(1.0) - (txx + tyy)))


def apply_pose(pose, x, y, z):
    """R(q) X + t in float64: each row summed left to right, then t (m4d_depth_cloud's and m4d_pose_accumulate's order)."""
    r = rot(pose)
    X, Y, Z = (np.asarray(v, D) for v in (x, y, z))
    return [((r[i][0] * X + r[i][1] * Y) + r[i][2] * Z) + D(pose[4 + i]) for i in range(3)]
