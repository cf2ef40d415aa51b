"""Binary little-endian PLY writer for meshes (NeRF.extract_mesh); NumPy only.  Extension: the reference writes no meshes."""
from __future__ import annotations

import numpy as np


def _host(a, dtype, cols, name):
    if a is None:
        return None
    if hasattr(a, "detach"):                 # torch tensor, on any device
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"save_ply: {name} must be [n, {cols}], got {a.shape}")
    return a


def save_ply(path, vertices, faces, normals=None, colors=None) -> None:
    """vertices [V,3] float32, faces [F,3] int (triangles), normals [V,3] float or None, colors [V,3] rgb in [0, 1] (stored as
    uchar red / green / blue) or None."""
    v = _host(vertices, np.float32, 3, "vertices")
    f = _host(faces, np.int32, 3, "faces")
    n = _host(normals, np.float32, 3, "normals")
    c = colors
    if c is not None:
        c = _host(c, np.float32, 3, "colors")
        c = np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8)
    for name, a in (("normals", n), ("colors", c)):
        if a is not None and a.shape[0] != v.shape[0]:
            raise ValueError(f"save_ply: {a.shape[0]} {name} for {v.shape[0]} vertices")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_ply: a face index is outside the vertex array")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(v.shape[0], dtype=np.dtype(fields))
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"] = 3
    frec["i"] = f
    ptype = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property {ptype[t]} {name}" for name, t in fields]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
