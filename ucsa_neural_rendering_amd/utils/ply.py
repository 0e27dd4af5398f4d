"""Binary little-endian PLY, numpy only.

``write_ply`` writes the labelled meshes of ``extract_semantic_mesh``: vertex
``x y z`` (float), optionally ``nx ny nz`` (float), ``red green blue`` (uchar)
and ``label`` (ushort, an NYU40 id: class + 1, 0 = unknown, as in ScanNet's
``*_vh_clean_2.labels.ply``), faces as ``list uchar int vertex_indices``.
``read_ply`` reads those files back and also ScanNet's labelled meshes (vertex
``x y z red green blue alpha label``): any binary little-endian file whose
vertex element holds scalar properties and whose faces are triangles."""
from __future__ import annotations

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1",
          "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
          "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4",
          "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def write_ply(path, verts, faces=None, normals=None, rgb=None, labels=None):
    """verts [V,3]; faces [F,3] or None; normals [V,3] or None; rgb [V,3]
    uint8, or float in [0,1] (rounded to 0..255), or None; labels [V] NYU40 ids
    (written as they are, as ushort) or None."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    V = verts.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    cols = {"x": verts[:, 0], "y": verts[:, 1], "z": verts[:, 2]}
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(V, 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.update(nx=normals[:, 0], ny=normals[:, 1], nz=normals[:, 2])
    if rgb is not None:
        rgb = np.asarray(rgb).reshape(V, 3)
        if rgb.dtype != np.uint8:
            rgb = np.round(np.clip(rgb.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        cols.update(red=rgb[:, 0], green=rgb[:, 1], blue=rgb[:, 2])
    if labels is not None:
        labels = np.asarray(labels).reshape(V)
        if labels.size and (labels.min() < 0 or labels.max() > 65535):
            raise ValueError("PLY labels are ushort: 0..65535")
        fields.append(("label", "<u2"))
        cols["label"] = labels
    vert = np.empty(V, dtype=fields)
    for name, _ in fields:
        vert[name] = cols[name]
    type_name = {"<f4": "float", "u1": "uchar", "<u2": "ushort"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V}"]
    header += [f"property {type_name[t]} {n}" for n, t in fields]
    face = None
    if faces is not None:
        faces = np.asarray(faces).reshape(-1, 3)
        if faces.size and (faces.min() < 0 or faces.max() >= V):
            raise ValueError("face indices out of range")
        face = np.empty(faces.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
        face["n"] = 3
        face["i"] = faces
        header += [f"element face {faces.shape[0]}",
                   "property list uchar int vertex_indices"]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        if face is not None:
            f.write(face.tobytes())


def _parse_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    elements, fmt = [], None
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY header has no end_header")
        words = line.decode("ascii").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            elements[-1][2].append(words[1:])
        elif words[0] == "end_header":
            break
    if fmt != "binary_little_endian":
        raise ValueError(f"only binary_little_endian PLY is read, not {fmt}")
    return elements


def read_ply(path):
    """-> dict: ``verts`` [V,3] f32; ``faces`` [F,3] int32 (if the file has
    faces); ``normals`` [V,3] f32, ``rgb`` [V,3] uint8, ``alpha`` [V] uint8,
    ``labels`` [V] int64 where the file has them; ``vertex``: every vertex
    property as a numpy structured array."""
    with open(path, "rb") as f:
        elements = _parse_header(f)
        data = f.read()
    out, pos = {}, 0
    for name, count, props in elements:
        if all(p[0] != "list" for p in props):
            dt = np.dtype([(p[1], _TYPES[p[0]]) for p in props])
            arr = np.frombuffer(data, dt, count, pos)
            pos += count * dt.itemsize
        elif len(props) == 1:
            _, ct, it, pname = props[0]
            dt = np.dtype([("n", _TYPES[ct]), (pname, _TYPES[it], (3,))])
            arr = np.frombuffer(data, dt, count, pos)
            if count and (arr["n"] != 3).any():
                raise ValueError(f"{name}: only triangles are read")
            pos += count * dt.itemsize
        else:
            raise ValueError(f"element {name}: a list property among others is not read")
        out[name] = arr
    v = out["vertex"]
    names = v.dtype.names
    res = {"vertex": v,
           "verts": np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)}
    if {"nx", "ny", "nz"} <= set(names):
        res["normals"] = np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float32)
    if {"red", "green", "blue"} <= set(names):
        res["rgb"] = np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8)
    if "alpha" in names:
        res["alpha"] = v["alpha"].astype(np.uint8)
    if "label" in names:
        res["labels"] = v["label"].astype(np.int64)
    if "face" in out:
        fa = out["face"]
        res["faces"] = np.asarray(fa[fa.dtype.names[1]], np.int32).reshape(-1, 3)
    return res
