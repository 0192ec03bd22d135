"""The reference's `.dmb` dumps (fileIoUtils.h:247-368): int32 {type=1, h, w, nb} followed by
h*w*nb float32, row-major.  `disp.dmb` holds norm4.w (depth), `normals.dmb` the world normals
(main.cpp:1001-1015); these are the "CPU-readable dumps" the depth-map fusion reads (gipuma_amd.fusion, the in-tree
consumer in place of the external fusibile tool of the reference's scripts)."""
import os

import numpy as np


def write_dmb(path, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, nb = a.shape
    with open(path, "wb") as f:
        np.array([1, h, w, nb], dtype=np.int32).tofile(f)
        a.tofile(f)


def read_dmb(path):
    with open(path, "rb") as f:
        hdr = np.fromfile(f, dtype=np.int32, count=4)
        if hdr[0] != 1:
            raise ValueError("%s: only float dmb (type 1) is defined" % path)
        h, w, nb = int(hdr[1]), int(hdr[2]), int(hdr[3])
        data = np.fromfile(f, dtype=np.float32, count=h * w * nb)
    out = data.reshape(h, w, nb)
    return out[:, :, 0] if nb == 1 else out


_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                        ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
               "property float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\n"
               "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def ply_points(depth, M_inv, P_col34):
    """get3Dpoint (cameraGeometryUtils.h:51-61) for every pixel, float32 like the reference:
    M_inv * (depth * (x, y, 1) - P.col(3)).  Returns (rows, cols, 3)."""
    rows, cols = depth.shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float32)
    d = depth.astype(np.float32)
    p4 = np.asarray(P_col34, dtype=np.float32)
    M = np.asarray(M_inv, dtype=np.float32).reshape(3, 3)
    v = np.stack([d * x - p4[0], d * y - p4[1], d - p4[2]], axis=-1)
    with np.errstate(invalid="ignore", over="ignore"):  # non-finite depths become (0, 0, 0) below
        X = (M[None, None, :, 0] * v[..., 0:1] + M[None, None, :, 1] * v[..., 1:2]) + M[None, None, :, 2] * v[..., 2:3]
    X = X.astype(np.float32)
    X[~np.isfinite(X).all(axis=-1)] = 0.0
    return X


def write_ply_binary(path, depth, normals, gray, M_inv, P_col34):
    """storePlyFileBinary (displayUtils.h:78-159): one vertex per pixel -- world point, normal and
    the gray value three times -- in the reference's loop order (x outer, y inner).  M_inv / P_col34
    belong to the NOT re-centred camera (getCameraParameters(..., false), main.cpp:1021)."""
    rows, cols = depth.shape
    v = np.zeros((cols, rows), dtype=_PLY_VERTEX)
    X = ply_points(depth, M_inv, P_col34)
    n = np.asarray(normals, dtype=np.float32)
    for k, name in enumerate(("x", "y", "z")):
        v[name] = X[:, :, k].T
    for k, name in enumerate(("nx", "ny", "nz")):
        v[name] = n[:, :, k].T
    g = np.asarray(gray, dtype=np.float32).astype(np.uint8).T
    v["red"] = v["green"] = v["blue"] = g
    with open(path, "wb") as f:
        f.write((_PLY_HEADER % (rows * cols)).encode())
        v.tofile(f)


def write_points_ply(path, points):
    """a point cloud (structured array of _PLY_VERTEX, e.g. gipuma_amd.fusion.fuse's result) as a binary PLY with the
    vertex layout of write_ply_binary"""
    v = np.ascontiguousarray(points, dtype=_PLY_VERTEX)
    with open(path, "wb") as f:
        f.write((_PLY_HEADER % len(v)).encode())
        v.tofile(f)


def read_ply_binary(path):
    """-> structured array of the vertices, in file order"""
    with open(path, "rb") as f:
        n = None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            if line.startswith(b"element vertex"):
                n = int(line.split()[2])
            if line.strip() == b"end_header":
                break
        return np.fromfile(f, dtype=_PLY_VERTEX, count=n)


_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
                "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
                "double": "f8", "float64": "f8"}


def _ply_header(f, path):
    """-> (format, [(element name, count, [(property name, scalar type or ("list", count type, item type))])])"""
    if f.readline().strip() != b"ply":
        raise ValueError("%s: not a PLY file" % path)
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("%s: no end_header" % path)
        w = line.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "end_header":
            break
        try:
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                elements.append((w[1], int(w[2]), []))
            elif w[0] == "property" and elements and w[1] == "list":
                elements[-1][2].append((w[4], ("list", _PLY_SCALARS[w[2]], _PLY_SCALARS[w[3]])))
            elif w[0] == "property" and elements:
                elements[-1][2].append((w[2], _PLY_SCALARS[w[1]]))
            else:
                raise ValueError
        except (IndexError, KeyError, ValueError):
            raise ValueError("%s: header line not understood: %r" % (path, line))
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError("%s: format %s is not read here (binary_little_endian and ascii are)" % (path, fmt))
    if any(n < 0 for _, n, _ in elements):
        raise ValueError("%s: negative element count" % path)
    return fmt, elements


def _ply_skip_binary(f, path, count, props):
    """moves past `count` binary elements, each property by its declared size"""
    if all(not isinstance(t, tuple) for _, t in props):
        f.seek(count * sum(np.dtype(t).itemsize for _, t in props), 1)
        return
    for _ in range(count):  # (lists: every element has its own size)
        for _, t in props:
            if isinstance(t, tuple):
                raw = f.read(np.dtype(t[1]).itemsize)
                if len(raw) < np.dtype(t[1]).itemsize:
                    raise ValueError("%s: file ends inside an element" % path)
                f.seek(int(np.frombuffer(raw, dtype="<" + t[1])[0]) * np.dtype(t[2]).itemsize, 1)
            else:
                f.seek(np.dtype(t).itemsize, 1)


def read_ply_xyz(path):
    """The x, y, z of a PLY file's element `vertex` as an (n, 3) float32 array, in file order.  Driven by the header:
    binary_little_endian or ascii, x / y / z declared float or double, every other property and every other element
    skipped by its declared size -- reference scans do not come in this project's own vertex layout, which is all
    read_ply_binary reads.  ValueError for a malformed or truncated file, a vertex without x, y or z, binary_big_endian
    and a vertex count the file cannot hold -- raised before anything of the claimed size is allocated."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        names = [e[0] for e in elements]
        if "vertex" not in names:
            raise ValueError("%s: no element vertex" % path)
        k = names.index("vertex")
        _, n, props = elements[k]
        pnames = [p for p, _ in props]
        for c in ("x", "y", "z"):
            if c not in pnames:
                raise ValueError("%s: element vertex has no property %s" % (path, c))
            if props[pnames.index(c)][1] not in ("f4", "f8"):
                raise ValueError("%s: property %s must be float or double" % (path, c))
        if fmt == "binary_little_endian":
            for _, cnt, pr in elements[:k]:
                _ply_skip_binary(f, path, cnt, pr)
            if any(isinstance(t, tuple) for _, t in props):
                raise ValueError("%s: a list property in element vertex is not read here" % path)
            dt = np.dtype([(("p%d" % i) if p not in ("x", "y", "z") else p, "<" + t) for i, (p, t) in enumerate(props)])
            if f.tell() > size or n * dt.itemsize > size - f.tell():
                raise ValueError("%s: the file cannot hold %d vertices of %d bytes" % (path, n, dt.itemsize))
            v = np.fromfile(f, dtype=dt, count=n)
            return np.stack([v["x"], v["y"], v["z"]], axis=-1).astype(np.float32).reshape(n, 3)
        # ascii: one element per line, a vertex of three one-digit numbers takes 6 bytes
        for _, cnt, _ in elements[:k]:
            for _ in range(cnt):
                if not f.readline():
                    raise ValueError("%s: file ends before element vertex" % path)
        if n * 6 > size - f.tell() + 1:
            raise ValueError("%s: the file cannot hold %d vertices" % (path, n))
        out = np.empty((n, 3), dtype=np.float32)
        for r in range(n):
            w = f.readline().split()
            at, col = 0, {}
            try:
                for p, t in props:
                    if isinstance(t, tuple):
                        at += 1 + int(w[at])
                    else:
                        col[p] = w[at]
                        at += 1
                if at > len(w):
                    raise IndexError
                out[r] = [float(col["x"]), float(col["y"]), float(col["z"])]
            except (IndexError, ValueError):
                raise ValueError("%s: vertex %d of %d is incomplete" % (path, r, n))
        return out


_PLY_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}


def read_ply_vertices(path):
    """A PLY file's element `vertex` as a structured array, in file order: every property under its own name and declared
    type (little-endian), so that a selection of the vertices can be written back with write_ply_vertices.  Reads what
    read_ply_xyz reads -- binary_little_endian or ascii, other elements skipped -- and refuses what it refuses, a list
    property in element vertex in either format included; also a property name that occurs twice."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        names = [e[0] for e in elements]
        if "vertex" not in names:
            raise ValueError("%s: no element vertex" % path)
        k = names.index("vertex")
        _, n, props = elements[k]
        if any(isinstance(t, tuple) for _, t in props):
            raise ValueError("%s: a list property in element vertex is not read here" % path)
        if len({p for p, _ in props}) != len(props):
            raise ValueError("%s: element vertex declares a property twice" % path)
        dt = np.dtype([(p, "<" + t) for p, t in props])
        if fmt == "binary_little_endian":
            for _, cnt, pr in elements[:k]:
                _ply_skip_binary(f, path, cnt, pr)
            if f.tell() > size or n * dt.itemsize > size - f.tell():
                raise ValueError("%s: the file cannot hold %d vertices of %d bytes" % (path, n, dt.itemsize))
            return np.fromfile(f, dtype=dt, count=n)
        for _, cnt, _ in elements[:k]:
            for _ in range(cnt):
                if not f.readline():
                    raise ValueError("%s: file ends before element vertex" % path)
        if n * 2 * len(props) > size - f.tell() + 1:  # (a one-digit number and its separator take 2 bytes)
            raise ValueError("%s: the file cannot hold %d vertices" % (path, n))
        out = np.empty(n, dtype=dt)
        for r in range(n):
            w = f.readline().split()
            try:
                if len(w) < len(props):
                    raise IndexError
                out[r] = tuple(float(v) if t[0] == "f" else int(v) for v, (_, t) in zip(w, props))
            except (IndexError, ValueError, OverflowError):
                raise ValueError("%s: vertex %d of %d is incomplete" % (path, r, n))
        return out


def write_ply_vertices(path, vertices):
    """a structured array of scalar fields (read_ply_vertices' result, or rows of it) as a binary_little_endian PLY with
    one element, `vertex`: every field a property of its name and type, in the array's order.  Written from this project's
    own vertex layout, the file is byte for byte write_points_ply's."""
    v = np.asarray(vertices)
    if v.dtype.names is None or v.ndim != 1:
        raise ValueError("write_ply_vertices takes a one-dimensional structured array")
    kinds = [v.dtype[name].newbyteorder("<").str[1:] for name in v.dtype.names]
    if any(k not in _PLY_NAMES for k in kinds):
        raise ValueError("a vertex property must be one of PLY's scalar types, got %s" % (v.dtype,))
    packed = np.empty(len(v), dtype=np.dtype([(name, "<" + k) for name, k in zip(v.dtype.names, kinds)]))
    for name in v.dtype.names:
        packed[name] = v[name]
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(packed)).encode())
        f.write("".join("property %s %s\n" % (_PLY_NAMES[k], name) for name, k in zip(v.dtype.names, kinds)).encode())
        f.write(b"end_header\n")
        packed.tofile(f)
