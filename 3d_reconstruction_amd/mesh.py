"""Triangle-mesh output (host only): the reference's final artefact is a ``.ply``
(``sfm.py:54-77``, ``numpy2ply.py``: an ascii point cloud); this writes the mesh of
:func:`voxel.tsdf_extract_surface` as a standard binary PLY.
"""
from __future__ import annotations

import numpy as np
import torch


def _host(a, dtype) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, faces, normals=None, colours=None) -> None:
    """Write ``vertices`` (V,3) f32, ``faces`` (F,3) int32, optional per-vertex
    ``normals`` (V,3) f32 and optional per-vertex ``colours`` (V,3) or (V,4) uint8
    (tensors or arrays) as ``binary_little_endian 1.0`` PLY: ``element vertex`` with
    x y z [nx ny nz] floats then [red green blue [alpha]] uchars, ``element face`` with
    ``property list uchar int vertex_indices``."""
    v = _host(vertices, "<f4")
    f = _host(faces, "<i4")
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be (V,3), got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be (F,3), got {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("faces index outside the vertex array")
    fields = [("xyz", "<f4", (3,))]
    props = ["property float x", "property float y", "property float z"]
    if normals is not None:
        n = _host(normals, "<f4")
        if n.shape != v.shape:
            raise ValueError(f"normals must match vertices {v.shape}, got {n.shape}")
        fields.append(("n", "<f4", (3,)))
        props += ["property float nx", "property float ny", "property float nz"]
    if colours is not None:
        c = colours.detach().cpu().numpy() if isinstance(colours, torch.Tensor) else np.asarray(colours)
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4):
            raise ValueError(f"colours must be ({v.shape[0]},3) or ({v.shape[0]},4) uint8, got {c.dtype} {c.shape}")
        fields.append(("rgba", "u1", (c.shape[1],)))
        props += [f"property uchar {name}" for name in ("red", "green", "blue", "alpha")[:c.shape[1]]]
    vrec = np.empty(v.shape[0], dtype=fields)   # packed: one record per vertex
    vrec["xyz"] = v
    if normals is not None:
        vrec["n"] = n
    if colours is not None:
        vrec["rgba"] = c
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", *props,
              f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(rec.tobytes())
