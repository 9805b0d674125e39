"""The matching stage of the reference (matching.py) on the sfmhip path:
BoW retrieval graph (GPU vq) -> exhaustive all-pairs BF matching (GPU, mutual
+ ratio) -> BFS pair selection + track building on the match graph (host C++)
-> the img_pairs / all_matches that sfm.py reads (matching.py:188-189).
With ``verify="essential"`` (and ``all_points``) the geometric check of
matching.py:130-144 runs on the GPU for every candidate pair in one batch
(verify.EssentialVerifier)."""
from __future__ import annotations

import numpy as np
import torch

import os

from . import bow, features, tracks, verify as _verify
from .match import MODE_FLOAT, DescriptorBank, all_pairs


def feature_stage(images, max_num_keypoints: int = 2048, bgr: bool = True, **sift_args):
    """The feature stage of the reference (feature_extraction.py) with the V11 SIFT of
    :func:`~.features.sift` in the place of DISK: V images of one size, (V,H,W) u8 grey or
    (V,H,W,3) u8 (``bgr=True``: in cv2.imread's channel order), in; the inter-stage arrays of
    SURVEY.md Appendix A out, as a dict: ``all_points`` (V,) object, each (K,2) f32
    (x - W/2, -(y - H/2)); ``all_descriptors`` (V,) object, each (K,128) f32 with the integer
    values 0..255 (``matching_stage(..., mode=MODE_SIFT)`` takes them as they are);
    ``all_colors`` (V,) object, each (K,3) u8, the image at (int(y), int(x)) (a grey image
    gives three equal channels); ``img_size`` (V,) object, each (2,) f32 [W, H]."""
    imgs = np.asarray(images.cpu() if isinstance(images, torch.Tensor) else images)
    if imgs.dtype != np.uint8 or imgs.ndim not in (3, 4) or (imgs.ndim == 4 and imgs.shape[3] != 3):
        raise ValueError(f"images must be (V,H,W) or (V,H,W,3) uint8, got {imgs.dtype} {imgs.shape}")
    V, H, W = imgs.shape[:3]
    f = features.sift(imgs, max_num_keypoints=max_num_keypoints, bgr=bgr, **sift_args)
    count = f["count"].cpu().numpy()
    kp, desc = f["keypoints"].cpu().numpy(), f["descriptors"].cpu().numpy()
    out = {k: np.empty(V, dtype=object) for k in ("all_points", "all_descriptors", "all_colors", "img_size")}
    for v in range(V):
        xy = kp[v, :count[v]]
        out["all_points"][v] = np.stack([xy[:, 0] - np.float32(W / 2), -(xy[:, 1] - np.float32(H / 2))],
                                        1).astype(np.float32)
        out["all_descriptors"][v] = desc[v, :count[v]].astype(np.float32)
        px = imgs[v][xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)]
        out["all_colors"][v] = np.ascontiguousarray(px if imgs.ndim == 4 else np.repeat(px[:, None], 3, 1))
        out["img_size"][v] = np.array([W, H], np.float32)
    return out


def save_features(directory, feats: dict) -> None:
    """Write :func:`feature_stage`'s result as the four ``.npy`` files matching.py and sfm.py
    read (``np.load(..., allow_pickle=True)``)."""
    os.makedirs(directory, exist_ok=True)
    for name in ("all_points", "all_descriptors", "all_colors", "img_size"):
        np.save(os.path.join(directory, name + ".npy"), feats[name], allow_pickle=True)


def matching_stage(all_descriptors, codebook, ratio=0.75, mode: int = MODE_FLOAT, top_k: int = 10,
                   verify=None, min_matches: int = 500, all_points=None, focal: float = 2378.98305085,
                   exact: bool | None = None):
    """Returns dict(img_pairs, all_matches, connection, start, matches0, matches1).
    ``exact`` (default: True for float descriptors): the matcher's distance semantics
    (match.py module docstring); False selects the quantised int8 mode."""
    descs = [np.asarray(d, np.float32) for d in all_descriptors]
    _, conn, start = bow.retrieval_graph(descs, codebook, top_k=top_k)
    bank = DescriptorBank.from_float(descs, mode=mode, exact=exact)
    pairs = all_pairs(len(descs))
    m0, m1 = bank.match(pairs, ratio=ratio, mutual=True)
    torch.cuda.synchronize()
    n_kpts = [d.shape[0] for d in descs]
    graph = tracks.MatchGraph(pairs, m0, m1, n_kpts)
    if isinstance(verify, str):
        if verify != "essential" or all_points is None:
            raise ValueError('verify must be a callable, None, or "essential" with all_points given')
        K = np.array([[focal, 0, 0], [0, focal, 0], [0, 0, 1.0]])       # matching.py:133
        verify = _verify.EssentialVerifier(conn, graph, all_points, K)
    img_pairs, all_matches = tracks.bfs_tracks(conn, start, n_kpts, graph, verify=verify,
                                               min_matches=min_matches)
    return dict(img_pairs=img_pairs, all_matches=all_matches, connection=conn, start=start,
                matches0=m0, matches1=m1)
