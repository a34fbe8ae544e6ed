"""PLY mesh loader with the dictionary layout of the reference's utils/ply_loader.py:11 load_ply: 'pts' [n,3], 'faces' [m,3]
(when the file has faces) and, when present, 'normals' [n,3], 'colors' [n,3] and 'texture_uv' [n,2], all float64 arrays like
there (face indices are whole numbers stored as floats).  ASCII and binary little-endian files; triangles only.
load_ply(path, texture=True) also reads the texture image the header names (comment TextureFile NAME, as BOP's UV-mapped
models carry it) from beside the PLY: 'texture_file' and 'texture' (uint8 [h,w,3], rows as in the file)."""
import os

import numpy as np

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
          "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
          "double": "f8", "float64": "f8"}


def _header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements, texture_file = None, [], None
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            if len(words) >= 3 and words[0] == "comment" and words[1] == "TextureFile":
                texture_file = line.decode("utf-8", "replace").split(None, 2)[2].strip()
            continue
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if not elements:
                raise ValueError("PLY property outside an element")
            if words[1] == "list":
                elements[-1][2].append((words[4], "list", _TYPES[words[2]], _TYPES[words[3]]))
            else:
                elements[-1][2].append((words[2], _TYPES[words[1]], None, None))
        elif words[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("PLY format %r is not supported (ascii, binary_little_endian)" % (fmt,))
    return fmt, elements, texture_file


def _load_texture(path, texture_file):
    """the image NAME of the header's comment TextureFile NAME, beside the PLY -> uint8 [h,w,3]"""
    if texture_file is None:
        raise ValueError("load_ply: texture=True, but %s has no 'comment TextureFile NAME' in its header" % path)
    image_path = os.path.join(os.path.dirname(os.path.abspath(path)), texture_file)
    if not os.path.isfile(image_path):
        raise ValueError("load_ply: the texture file %s named by %s does not exist" % (image_path, path))
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("load_ply: texture=True reads the texture image with PIL (Pillow), which is not installed")
    with Image.open(image_path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))


def _read_binary(f, count, props):
    if all(p[1] != "list" for p in props):
        dt = np.dtype([(p[0], "<" + p[1]) for p in props])
        return np.frombuffer(f.read(dt.itemsize * count), dt, count)
    rows = []
    for _ in range(count):
        row = {}
        for name, kind, cnt_t, item_t in props:
            if kind == "list":
                k = int(np.frombuffer(f.read(np.dtype(cnt_t).itemsize), "<" + cnt_t)[0])
                row[name] = np.frombuffer(f.read(np.dtype(item_t).itemsize * k), "<" + item_t, k)
            else:
                row[name] = np.frombuffer(f.read(np.dtype(kind).itemsize), "<" + kind)[0]
        rows.append(row)
    return rows


def _read_ascii(f, count, props):
    rows = []
    for _ in range(count):
        vals = f.readline().split()
        row, i = {}, 0
        for name, kind, _cnt_t, _item_t in props:
            if kind == "list":
                k = int(vals[i])
                row[name] = np.array([float(v) for v in vals[i + 1: i + 1 + k]])
                i += 1 + k
            else:
                row[name] = float(vals[i])
                i += 1
        rows.append(row)
    return rows


def _column(data, name):
    if isinstance(data, np.ndarray):
        return data[name].astype(np.float64)
    return np.array([r[name] for r in data], np.float64)


def load_ply(path, texture=False):
    """Mesh from a PLY file -> dict(pts, faces[, normals, colors, texture_uv]) of float64 arrays; with texture also
    texture_file (the NAME of the header's comment TextureFile NAME) and texture (that image, uint8 [h,w,3])."""
    with open(path, "rb") as f:
        fmt, elements, texture_file = _header(f)
        model = {}
        for name, count, props in elements:
            data = _read_binary(f, count, props) if fmt == "binary_little_endian" else _read_ascii(f, count, props)
            names = [p[0] for p in props]
            if name == "vertex":
                model["pts"] = np.stack([_column(data, k) for k in ("x", "y", "z")], 1) if count else np.zeros((0, 3))
                for key, cols in (("normals", ("nx", "ny", "nz")), ("colors", ("red", "green", "blue")),
                                  ("texture_uv", ("texture_u", "texture_v"))):
                    if set(cols) <= set(names):
                        model[key] = np.stack([_column(data, k) for k in cols], 1) if count else np.zeros((0, len(cols)))
            elif name == "face" and count > 0:
                key = "vertex_indices" if "vertex_indices" in names else "vertex_index" if "vertex_index" in names else None
                if key is None:
                    raise ValueError("PLY faces without vertex_indices")
                idx = [np.asarray(r[key]) for r in data]
                if any(len(v) != 3 for v in idx):
                    raise ValueError("only triangular faces are supported")
                model["faces"] = np.array(idx, np.float64).reshape(count, 3)
    if "pts" not in model:
        raise ValueError("PLY file without vertices")
    if texture:
        model["texture"] = _load_texture(path, texture_file)
        model["texture_file"] = texture_file
    return model
