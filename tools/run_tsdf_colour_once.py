"""Run the C5 TSDF fusion and the colour fusion a few times with a shared block table
(for rocprofv3 --kernel-trace --stats: tsdf_fuse_kernel beside tsdf_colour_kernel)."""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfm = importlib.import_module("3d_reconstruction_amd")
syn = importlib.import_module("3d_reconstruction_amd.synthetic")
dev = torch.device("cuda", 0)
depth, poses, K = syn.tsdf_scene(int(os.environ.get("NF", "257")), syn.IMG_H, syn.IMG_W, device=dev)
colour = syn.tsdf_scene_colour(depth, poses, K)
table = sfm.tsdf_block_table(depth)
R = 256
T = torch.zeros((R, R, R), dtype=torch.float32, device=dev)
W = torch.zeros_like(T)
C = torch.zeros((R, R, R, 4), dtype=torch.int32, device=dev)
box = ((-1.2,) * 3, (1.2,) * 3, 3 * 2.4 / (R - 1))
for _ in range(int(os.environ.get("REPS", "4"))):
    sfm.tsdf_integrate(T, W, depth, poses, K, *box, block_table=table)
    sfm.tsdf_integrate_colour(C, depth, colour, poses, K, *box, block_table=table)
torch.cuda.synchronize()
print("updated", float((W > 0).double().mean()), "coloured", float((C[..., 3] > 0).double().mean()))
