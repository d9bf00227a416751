"""CPU: deepmerge_amd/shpstore.py -- the three writers read back through ShapeReader (geometry, parts, fields, FIDs), the header
bytes at the offsets the ESRI description fixes, the .shx rows, a null shape, the PointID limit and the geo_to_pixel inverse."""
import struct
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import vector_ref as V
from deepmerge_amd import shpstore
from deepmerge_amd.patches import geo_to_pixel

GT = (512345.5, 0.5, 0.0, 4187654.25, 0.0, -0.5)                    # north-up, half-metre pixels


def traced(name="absent_ids"):
    labels, n = V.host_cases()[name]
    t = V.trace(labels, n)
    polys = SimpleNamespace(region_ptr=t["region_ptr"], ring_ptr=t["ring_ptr"], xy=t["xy"])
    arcs = SimpleNamespace(arc_ptr=t["arc_ptr"], xy=t["arc_xy"], left=t["left"], right=t["right"])
    return t, n, polys, arcs


def signed_area2(p):
    q = np.roll(p, -1, 0)
    return float((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def test_polygons_round_trip_with_a_null_shape(tmp_path):
    t, n, polys, _ = traced()
    area = np.arange(n, dtype=np.float32) * np.float32(1.1)
    ids = [f"{i} {i + 1}" for i in range(n)]
    path = shpstore.write_polygons(str(tmp_path / "polygons.shp"), polys, [("area", area), ("count", np.arange(n, dtype=np.int32) - 2),
                                                                          ("PointID", ids)], GT)
    r = shpstore.ShapeReader(path)
    assert r.shape_type == 5 and len(r) == n
    for l in range(n):                                              # FID = record number - 1 = label
        rings = range(t["region_ptr"][l], t["region_ptr"][l + 1])
        if len(rings) == 0:
            assert r.shapes[l] is None                              # an absent id: a null shape
            continue
        assert len(r.shapes[l]) == len(rings)
        for part, ring in zip(r.shapes[l], rings):
            xy = t["xy"][t["ring_ptr"][ring]:t["ring_ptr"][ring + 1]].astype(np.float64)
            want = np.stack((GT[0] + xy[:, 0] * GT[1], GT[3] + xy[:, 1] * GT[5]), 1)
            assert np.array_equal(part[:-1], want) and np.array_equal(part[-1], part[0])      # closed, as the format asks
            # north-up: outer rings clockwise (negative signed area with Y up), holes anticlockwise
            assert np.sign(signed_area2(part[:-1])) == -np.sign(t["ring_area2"][ring])
    assert r.shapes[1] is None and r.shapes[0] is not None
    assert np.array_equal(r.fields["area"].astype(np.float32), area) and r.fields["count"].tolist() == list(range(-2, n - 2))
    assert r.fields["PointID"] == ids


def test_lines_and_points_round_trip(tmp_path):
    t, n, _, arcs = traced("hole_meets_outside")
    simi = np.linspace(0, 1, len(t["left"])).astype(np.float32)
    path = shpstore.write_lines(str(tmp_path / "lines.shp"), arcs, [("LEFT_FID", t["left"]), ("RIGHT_FID", t["right"]), ("simi", simi)])
    r = shpstore.ShapeReader(path)
    assert r.shape_type == 3 and len(r) == len(t["left"])
    for a, shape in enumerate(r.shapes):
        xy = t["arc_xy"][t["arc_ptr"][a]:t["arc_ptr"][a + 1]].astype(np.float64)
        assert len(shape) == 1 and np.array_equal(shape[0], np.stack((xy[:, 0], -xy[:, 1]), 1))      # the default transform: Y = -y
    assert r.fields["LEFT_FID"].tolist() == t["left"].tolist() and r.fields["RIGHT_FID"].tolist() == t["right"].tolist()
    assert np.array_equal(r.fields["simi"].astype(np.float32), simi)
    xy = np.array([[1, 1], [3, 2], [4095, 77], [17, 4095]], np.int32)
    path = shpstore.write_points(str(tmp_path / "PointsGCS.shp"), xy, [("inner", np.array([1, 3, 5, 7], np.int32)),
                                                                       ("object", np.array([9, 8, 7, 6], np.int32))], GT)
    r = shpstore.ShapeReader(path)
    assert r.shape_type == 1 and len(r) == 4 and r.fields["inner"].tolist() == [1, 3, 5, 7] and r.fields["object"].tolist() == [9, 8, 7, 6]
    geo = np.stack(r.shapes)
    back = geo_to_pixel(GT, torch.from_numpy(geo[:, 0]), torch.from_numpy(geo[:, 1]))             # the reference's conversion
    assert np.array_equal(back.numpy(), xy)


def test_header_bytes_and_index(tmp_path):
    t, n, polys, _ = traced()
    path = shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("v", np.arange(n, dtype=np.int32))])
    shp, shx, dbf = (open(str(tmp_path / ("p." + e)), "rb").read() for e in ("shp", "shx", "dbf"))
    for data in (shp, shx):
        assert struct.unpack_from(">i", data, 0)[0] == 9994 and data[4:24] == bytes(20)
        assert struct.unpack_from(">i", data, 24)[0] * 2 == len(data)                             # length in 16-bit words, big-endian
        assert struct.unpack_from("<ii", data, 28) == (1000, 5)                                   # version, shape type, little-endian
        assert struct.unpack_from("<4d", data, 36) == (0.0, -4.0, 5.0, 0.0) and data[68:100] == bytes(32)
    assert len(shx) == 100 + 8 * n
    for i in range(n):
        offset, words = struct.unpack_from(">ii", shx, 100 + 8 * i)
        assert struct.unpack_from(">ii", shp, 2 * offset) == (i + 1, words)                       # record numbers from 1
        kind = struct.unpack_from("<i", shp, 2 * offset + 8)[0]
        assert kind == (5 if t["region_ptr"][i + 1] > t["region_ptr"][i] else 0)
        assert (kind == 0) == (words == 2)
    offset, words = struct.unpack_from(">ii", shx, 100 + 8 * (n - 1))
    assert 2 * (offset + 4 + words) == len(shp)
    assert dbf[0] == 3 and struct.unpack_from("<IHH", dbf, 4) == (n, 32 + 32 + 1, 1 + 11) and dbf[32:34] == b"v\0" and dbf[43:44] == b"N"
    assert dbf[64] == 0x0D and dbf[-1] == 0x1A and len(dbf) == 65 + 12 * n + 1


def test_field_limits(tmp_path):
    _, n, polys, _ = traced()
    ids = ["1"] * n
    ids[3] = " ".join(["12345"] * 43)                               # 257 characters
    with pytest.raises(ValueError, match="region 3"):
        shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("PointID", ids)])
    ids[3] = "7" * 254
    shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("PointID", ids), ("shapeness", np.zeros(n, np.float32))])
    assert shpstore.ShapeReader(str(tmp_path / "p.shp")).fields["PointID"][3] == "7" * 254
    with pytest.raises(ValueError):
        shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("elevenchars", np.zeros(n))])
    with pytest.raises(ValueError):
        shpstore.write_polygons(str(tmp_path / "p.shp"), polys, [("v", np.zeros(n + 1))])
