"""Poses the SfM adapter (plan.dense_inputs_from_reconstruction) hands to the dense kernels, for
tests: mirrored poses diag(1, -1, 1) [R|t] (orthogonal, determinant -1) and all-zero poses of
unregistered cameras.  A plain helper module: numpy only, no GPU, no package import; not a test,
not a conftest.

The twin identity.  Every dense kernel uses a pose only through sums of products, and fy only as
a factor or a divisor.  With F = diag(1, -1, 1), the call with (F P, K) ("twin A", the adapter's
case) and the call with (P, K with fy negated) ("twin B", a mirrored frame: scene C of
tsdf_cam_scenes.py) see the same pixel for every point, and in IEEE arithmetic with the same
operation order and round-to-nearest (which is symmetric under negation) they perform the same
products, quotients and sums with some signs flipped: every output of A has the bits of B's.
The premise is checked on the numpy restatements by test_mirrored_poses_cpu.py."""
import numpy as np

FLIP = np.array([1.0, -1.0, 1.0])


def twin_a(poses):
    """F P in the input dtype: row 1 of every (3,4) pose negated (exact)."""
    out = np.array(poses, copy=True)
    out[..., 1, :] = -out[..., 1, :]
    return out


def twin_b(K):
    """K (.., 4) [fx, fy, cx, cy] with fy negated (exact), in the input dtype."""
    out = np.array(K, copy=True)
    out[..., 1] = -out[..., 1]
    return out


def zeroed(poses, views):
    """The given views set to the all-zero pose of an unregistered camera."""
    out = np.array(poses, copy=True)
    out[list(views)] = 0
    return out


def mirrored_world(poses, X):
    """The adapter's true situation for proper cameras [R|t] (V,3,4) and points X (N,3), with
    M = F = diag(1, -1, 1): the world mirrored, X' = X M; the proper SfM-form cameras F [R M | t]
    of it (determinant +1: what incremental_sfm holds, in keypoint coordinates with y up); and
    the dense poses [R M | t] (determinant -1) the adapter must return for them.  [R M | t] maps
    X' onto the camera coordinates [R|t] gives X, every product with both signs flipped or none.
    -> X', sfm_cameras (V,3,4), dense_poses (V,3,4), each in the dtype of its input."""
    poses = np.asarray(poses)
    dense = np.array(poses, copy=True)
    dense[..., :, 1] = -dense[..., :, 1]           # R M: column 1 negated
    Xm = np.array(X, copy=True)
    Xm[..., 1] = -Xm[..., 1]
    return Xm, twin_a(dense), dense
