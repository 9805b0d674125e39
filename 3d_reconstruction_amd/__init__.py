"""sfmhip — MI355X-native (gfx950) backend for the dense-compute path of
daovietanh190499/3D_Reconstruction: BF-L2 descriptor matching + ratio test,
DLT triangulation, reprojection residual / FD Jacobian, voxel-grid work.

The directory name is not a Python identifier; import it as ``sfmhip`` (the
alias module ``sfmhip.py`` at the repository root) or with
``importlib.import_module("3d_reconstruction_amd")``.
The cv2 names sfm.py / matching.py use (RANSAC, SOLVEPNP_ITERATIVE and the
functions) are top-level, so ``import sfmhip as cv2`` binds them.
Every compute entry point runs a HIP kernel from ``libsfmhip.so``; there is no
CPU fallback.
"""
from ._abi import LIB_PATH, SfmHipError, knobs_reload, lib, require_gpu  # noqa: F401  (fails loudly if the .so is missing)
from .match import (MODE_FLOAT, MODE_SIFT, DescriptorBank, Matcher, all_pairs,  # noqa: F401
                    bf_match, vq)
from .geometry import (Rodrigues, ba_sparse, calculate_reprojection_error,  # noqa: F401
                       convertPointsFromHomogeneous, fd_jacobian, projectPoints,
                       residual_jacobian_batched, triangulatePoints, triangulate_batched, ba_solve_batched,
                       least_squares_ba, ba_global_structure, ba_global_linearize, ba_global_schur_matvec,
                       bundle_adjust, ba_loss_weight, ba_calib_linearize, ba_calib_matvec, undistort_points,
                       undistortPoints, triangulate_tracks)
from .voxel import (MASK_PLENOXEL, MASK_SDF, VoxelGrid, icp_normal_equations, icp_track, tsdf_block_table,  # noqa: F401,E501
                    tsdf_cull_stats, tsdf_integrate, tsdf_extract_surface, tsdf_integrate_colour, tsdf_layer_cost,
                    tsdf_layer_stats, tsdf_raycast, tsdf_track, voxel_traversal)
from .mvs import census_transform, depth_consistency, inverse_depth_planes, mvs_depth, plane_sweep  # noqa: F401
from .mvs import cost_volume, sgm_aggregate, volume_select  # noqa: F401
from .rectify import optimal_new_K, undistort_depth, undistort_images, undistort_map  # noqa: F401
from .plan import (DensePlan, cubic_grid, dense_inputs_from_reconstruction, obs_depth, plan_dense, plan_from_reconstruction, scene_bounds,  # noqa: F401
                   segmented_select, select_sources, view_depth_ranges, view_pair_counts)
from .features import (sift, sift_describe, sift_detect, sift_orient, sift_pyramid,  # noqa: F401
                       sift_tables)
from . import bow, features, mesh, mvs, pipeline, plan, reconstruct, rectify, tracks, twoview, verify  # noqa: F401,E402
from .mesh import write_ply  # noqa: F401
from .bow import kmeans  # noqa: F401
from .reconstruct import retriangulate, triangulate  # noqa: F401
from .tracks import MatchGraph, bfs_tracks, with_initial_pair  # noqa: F401
from .verify import RANSAC, SOLVEPNP_ITERATIVE, findEssentialMat, findHomography, recoverPose, solvePnPRansac  # noqa: F401
from .twoview import classify_pairs, select_initial_pair  # noqa: F401
from .dist import RcclComm, match_all_pairs_sharded  # noqa: F401

__version__ = "0.1.0"
