"""ESRI shapefiles (.shp / .shx / .dbf) written and read with numpy and `struct` alone: no GDAL, as h5store.py does without h5py.

The reference reads its superpixels from shapefiles written by external GIS software: a polygon layer with the 15 designed
attributes and a `PointID` string (MyUtils1.py:79-114, ExtractFeatures.py:175-179), a point layer with `inner` / `object`
(MyUtils1.py:64-65) and `lines.shp` with one polyline per shared boundary and `LEFT_FID` / `RIGHT_FID` (MyUtils2.py:155-193), into
which `test_for_shp` writes `simi` (ExtractFeatures.py:181-219).  The writers here produce those layers from `rag.polygons`,
`rag.boundary_arcs` and `rag.sample_points`; FID = record number - 1 = label / arc / point index.

Layout, from the ESRI Shapefile Technical Description (1998): a 100-byte header (file code 9994 and the file length in 16-bit
words big-endian; version 1000, shape type and the bounding box little-endian), then records of an 8-byte big-endian header (record
number from 1, content length in words) and little-endian content.  The .shx repeats the header and lists (offset, content length)
per record, in words.  The .dbf is dBASE III: `N` fields for integers, `F` for floats (%.15e: 16 significant digits, which
round-trips float32 exactly), `C` for strings of at most 254 characters.

`ShapeReader` reads back what the writers write (and other files of the three shape types).  It shares the writers' reading of
the description, so a round trip through it checks the writers' arithmetic and not their interpretation of the format: no reader
from GDAL or pyshp has opened these files.
"""
from __future__ import annotations

import os
import struct
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

NULL, POINT, POLYLINE, POLYGON = 0, 1, 3, 5
DEFAULT_GEOTRANSFORM = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
MAX_STRING = 254


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def corner_to_geo(gt: Optional[Sequence[float]], xy: np.ndarray) -> np.ndarray:
    """float64 [N,2]: X = gt[0] + x gt[1] + y gt[2], Y = gt[3] + x gt[4] + y gt[5] (None: X = x, Y = -y)."""
    gt = DEFAULT_GEOTRANSFORM if gt is None else tuple(float(v) for v in gt)
    if len(gt) != 6:
        raise ValueError("geotransform must have six entries")
    x, y = np.asarray(xy[:, 0], np.float64), np.asarray(xy[:, 1], np.float64)
    return np.stack((gt[0] + x * gt[1] + y * gt[2], gt[3] + x * gt[4] + y * gt[5]), 1)


def geo_to_corner(gt: Optional[Sequence[float]], XY: np.ndarray) -> np.ndarray:
    """float64 [N,2]: the inverse of `corner_to_geo`, the corner position (x, y) of every (X, Y).  Solves the general 2x2, so the
    rotation terms gt[2], gt[4] may be non-zero; a singular transform raises."""
    gt = DEFAULT_GEOTRANSFORM if gt is None else tuple(float(v) for v in gt)
    if len(gt) != 6:
        raise ValueError("geotransform must have six entries")
    det = gt[1] * gt[5] - gt[2] * gt[4]
    if det == 0.0 or not np.isfinite(det):
        raise ValueError(f"geotransform {gt} is singular: gt[1] gt[5] - gt[2] gt[4] = {det}")
    XY = np.asarray(XY, np.float64).reshape(-1, 2)
    dX, dY = XY[:, 0] - gt[0], XY[:, 1] - gt[3]
    return np.stack(((gt[5] * dX - gt[2] * dY) / det, (gt[1] * dY - gt[4] * dX) / det), 1)


def pixel_to_geo(gt: Optional[Sequence[float]], xy: np.ndarray) -> np.ndarray:
    """The position of pixel (x, y) for which `patches.geo_to_pixel` (the reference's conversion, int(|offset / size| + 1)) returns
    (x, y): half a pixel in front of corner (x, y).  That conversion never returns 0, so a pixel of column or row 0 reads back as 1."""
    return corner_to_geo(gt, np.asarray(xy, np.float64) - 0.5)


# ---- .dbf ---------------------------------------------------------------------------------------------------------------------------
def _dbf_columns(fields, n: int, what: str):
    cols = []
    for name, values in fields:
        if not 1 <= len(name) <= 10 or not name.isascii():
            raise ValueError(f"field name {name!r} must have 1..10 ASCII characters")
        if isinstance(values, (list, tuple)) and all(isinstance(v, str) for v in values):
            if len(values) != n:
                raise ValueError(f"field {name!r} has {len(values)} values for {n} {what}")
            for i, v in enumerate(values):
                if len(v) > MAX_STRING:
                    raise ValueError(f"field {name!r} of {what[:-1]} {i} has {len(v)} characters; a dBASE string holds at most {MAX_STRING}")
            width = max([1] + [len(v) for v in values])
            cols.append((name, b"C", width, 0, [v.encode("ascii").ljust(width) for v in values]))
            continue
        v = _np(values)
        if v.shape != (n,):
            raise ValueError(f"field {name!r} has shape {v.shape} for {n} {what}")
        if v.dtype.kind in "iub":
            width = 20 if v.dtype.itemsize == 8 else 11
            cols.append((name, b"N", width, 0, [b"%*d" % (width, int(x)) for x in v]))
        elif v.dtype.kind == "f":
            cols.append((name, b"F", 24, 15, [b"%24.15e" % float(x) for x in v]))
        else:
            raise ValueError(f"field {name!r}: dtype {v.dtype} is neither integer, float nor a list of strings")
    return cols


def _write_dbf(path: str, fields, n: int, what: str):
    cols = _dbf_columns(fields, n, what)
    if not cols:
        cols = [("FID", b"N", 11, 0, [b"%11d" % i for i in range(n)])]        # a table needs a field
    record = 1 + sum(c[2] for c in cols)
    t = time.localtime()
    out = [struct.pack("<BBBBIHH20x", 3, t.tm_year - 1900, t.tm_mon, t.tm_mday, n, 32 + 32 * len(cols) + 1, record)]
    for name, kind, width, dec, _ in cols:
        out.append(struct.pack("<11sc4xBB14x", name.encode("ascii"), kind, width, dec))
    out.append(b"\r")
    for i in range(n):
        out.append(b" " + b"".join(c[4][i] for c in cols))
    out.append(b"\x1a")
    with open(path, "wb") as f:
        f.write(b"".join(out))


def _read_dbf(path: str) -> Dict[str, object]:
    data = open(path, "rb").read()
    n, header, record = struct.unpack_from("<IHH", data, 4)
    cols, at = [], 32
    while data[at] != 0x0D:
        name, kind, width, dec = struct.unpack_from("<11sc4xBB", data, at)
        cols.append((name.split(b"\0")[0].decode("ascii"), kind, width))
        at += 32
    table: Dict[str, list] = {c[0]: [] for c in cols}
    for i in range(n):
        at = header + i * record + 1
        for name, kind, width in cols:
            text = data[at:at + width].decode("ascii")
            at += width
            table[name].append(text.rstrip() if kind == b"C" else int(text) if kind == b"N" and "." not in text and "e" not in text else float(text))
    return {k: (v if v and isinstance(v[0], str) else np.asarray(v)) for k, v in table.items()}


# ---- .shp / .shx --------------------------------------------------------------------------------------------------------------------
def _header(words: int, shape_type: int, box) -> bytes:
    return struct.pack(">i5ii", 9994, 0, 0, 0, 0, 0, words) + struct.pack("<ii4d4d", 1000, shape_type, *box, 0.0, 0.0, 0.0, 0.0)


def _box(points: np.ndarray):
    if points.shape[0] == 0:
        return (0.0, 0.0, 0.0, 0.0)
    return (points[:, 0].min(), points[:, 1].min(), points[:, 0].max(), points[:, 1].max())


def _write_shapes(path: str, shape_type: int, contents: List[bytes], all_points: np.ndarray):
    base = os.path.splitext(path)[0]
    records, index, offset = [], [], 50
    for i, c in enumerate(contents):
        assert len(c) % 2 == 0
        records.append(struct.pack(">ii", i + 1, len(c) // 2) + c)
        index.append(struct.pack(">ii", offset, len(c) // 2))
        offset += 4 + len(c) // 2
    box = _box(all_points)
    with open(base + ".shp", "wb") as f:
        f.write(_header(offset, shape_type, box) + b"".join(records))
    with open(base + ".shx", "wb") as f:
        f.write(_header(50 + 4 * len(contents), shape_type, box) + b"".join(index))


def _multipart(shape_type: int, parts: List[np.ndarray]) -> bytes:
    if not parts:
        return struct.pack("<i", NULL)
    pts = np.concatenate(parts)
    starts = np.cumsum([0] + [p.shape[0] for p in parts[:-1]])
    return (struct.pack("<i4dii", shape_type, *_box(pts), len(parts), pts.shape[0]) + np.asarray(starts, "<i4").tobytes() +
            np.ascontiguousarray(pts, "<f8").tobytes())


def write_polygons(path: str, polygons, fields, geotransform=None) -> str:
    """Shape type 5, one record per label with its rings as parts (each closed by repeating its first vertex, as the format asks); a
    label without a ring is a null shape.  polygons: `rag.Polygons`; fields: [(name, int / float array [n_labels] or list of str)].
    With a north-up transform outer rings come out clockwise and holes anticlockwise, the format's own rule."""
    region_ptr, ring_ptr = _np(polygons.region_ptr), _np(polygons.ring_ptr)
    geo = corner_to_geo(geotransform, _np(polygons.xy))
    contents = []
    for l in range(region_ptr.shape[0] - 1):
        rings = [geo[ring_ptr[r]:ring_ptr[r + 1]] for r in range(region_ptr[l], region_ptr[l + 1])]
        contents.append(_multipart(POLYGON, [np.concatenate((r, r[:1])) for r in rings]))
    _write_shapes(path, POLYGON, contents, geo)
    _write_dbf(os.path.splitext(path)[0] + ".dbf", fields, len(contents), "regions")
    return path


def write_lines(path: str, arcs, fields, geotransform=None) -> str:
    """Shape type 3, one single-part record per arc of `rag.Arcs`."""
    arc_ptr = _np(arcs.arc_ptr)
    geo = corner_to_geo(geotransform, _np(arcs.xy))
    contents = [_multipart(POLYLINE, [geo[arc_ptr[a]:arc_ptr[a + 1]]]) for a in range(arc_ptr.shape[0] - 1)]
    _write_shapes(path, POLYLINE, contents, geo)
    _write_dbf(os.path.splitext(path)[0] + ".dbf", fields, len(contents), "arcs")
    return path


def write_points(path: str, xy, fields, geotransform=None) -> str:
    """Shape type 1, one record per pixel position (x, y) of xy int [P,2], written where `patches.geo_to_pixel` reads it back
    (pixel_to_geo)."""
    geo = pixel_to_geo(geotransform, _np(xy).reshape(-1, 2))
    contents = [struct.pack("<i2d", POINT, p[0], p[1]) for p in geo]
    _write_shapes(path, POINT, contents, geo)
    _write_dbf(os.path.splitext(path)[0] + ".dbf", fields, len(contents), "points")
    return path


class ShapeReader:
    """A .shp with its .shx and .dbf: shape_type, box, `shapes` (per record: None for a null shape, float64 [2] for a point, else a
    list of float64 [n,2] parts), `offsets` (the .shx rows, in words) and `fields` (name -> int / float array or list of str)."""

    def __init__(self, path: str):
        base = os.path.splitext(path)[0]
        data = open(base + ".shp", "rb").read()
        code, words = struct.unpack_from(">i20xi", data, 0)
        version, self.shape_type = struct.unpack_from("<ii", data, 28)
        if code != 9994 or version != 1000 or 2 * words != len(data):
            raise ValueError(f"{path}: not a shapefile (file code {code}, version {version}, {2 * words} bytes declared, {len(data)} found)")
        if self.shape_type not in (POINT, POLYLINE, POLYGON):
            raise ValueError(f"{path}: shape type {self.shape_type} is not point, polyline or polygon")
        self.box = struct.unpack_from("<4d", data, 36)
        shx = open(base + ".shx", "rb").read()
        n = (len(shx) - 100) // 8
        self.offsets = np.frombuffer(shx, ">i4", 2 * n, 100).reshape(n, 2).astype(np.int64)
        self.shapes: List[object] = []
        for i, (off, length) in enumerate(self.offsets):
            at = 2 * int(off)
            number, words = struct.unpack_from(">ii", data, at)
            if number != i + 1 or words != length:
                raise ValueError(f"{path}: record {i + 1}: the .shx row does not point at its record header")
            at += 8
            kind = struct.unpack_from("<i", data, at)[0]
            if kind == NULL:
                self.shapes.append(None)
            elif kind == POINT:
                self.shapes.append(np.frombuffer(data, "<f8", 2, at + 4).copy())
            else:
                n_parts, n_points = struct.unpack_from("<ii", data, at + 36)
                starts = list(np.frombuffer(data, "<i4", n_parts, at + 44)) + [n_points]
                pts = np.frombuffer(data, "<f8", 2 * n_points, at + 44 + 4 * n_parts).reshape(n_points, 2)
                self.shapes.append([pts[starts[p]:starts[p + 1]].copy() for p in range(n_parts)])
        self.fields = _read_dbf(base + ".dbf")

    def __len__(self) -> int:
        return len(self.shapes)


def read_rings(path: str, geotransform=None, label_field: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ring_ptr int64 [R+1], xy float64 [V,2] in pixel-corner space, ring_label int32 [R]) of a polygon shapefile, the arrays of
    `rag.Rings`.  All parts of record i are rings of label i (the FID), or of the value of the integer field `label_field`; null
    shapes are skipped.  A ring keeps its repeated closing vertex (a zero-length edge to `rag.rasterize`).  A file that is not of
    polygon type, a field that is missing, not integer, negative or >= 2^31 - 1, and a part of fewer than 2 vertices raise
    ValueError naming the record."""
    return _read_rings(path, geotransform, label_field)[:3]


def _read_rings(path: str, geotransform, label_field: Optional[str]):
    """read_rings and n_labels: the record count when the label is the FID, the field's largest value + 1 otherwise."""
    shp = ShapeReader(path)
    if shp.shape_type != POLYGON:
        raise ValueError(f"{path}: shape type {shp.shape_type} is not polygon ({POLYGON})")
    values = None
    if label_field is not None:
        if label_field not in shp.fields:
            raise ValueError(f"{path}: no field {label_field!r} (fields: {sorted(shp.fields)})")
        values = shp.fields[label_field]
        if isinstance(values, list) or values.dtype.kind not in "iu":
            raise ValueError(f"{path}: field {label_field!r} is not an integer field")
        if len(values) != len(shp):
            raise ValueError(f"{path}: field {label_field!r} has {len(values)} values for {len(shp)} records")
    ring_ptr, parts, labels, n_labels = [0], [], [], 0
    for i, shape in enumerate(shp.shapes):
        label = i if values is None else int(values[i])
        if not 0 <= label < (1 << 31) - 1:
            raise ValueError(f"{path}: record {i + 1}: label {label} of field {label_field!r} is outside 0 .. 2^31 - 2")
        n_labels = max(n_labels, label + 1)
        if shape is None:
            continue
        for p, part in enumerate(shape):
            if part.shape[0] < 2:
                raise ValueError(f"{path}: record {i + 1}: part {p} has {part.shape[0]} vertices; a ring needs at least 2")
            parts.append(part)
            ring_ptr.append(ring_ptr[-1] + part.shape[0])
            labels.append(label)
    xy = geo_to_corner(geotransform, np.concatenate(parts)) if parts else np.zeros((0, 2), np.float64)
    return np.asarray(ring_ptr, np.int64), xy, np.asarray(labels, np.int32), n_labels
