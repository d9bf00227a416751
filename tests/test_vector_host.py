"""CPU: the spec tests/vector_ref.py by itself -- the tabulated ring counts, and for every case the properties that make the
rings and arcs a faithful account of the raster (oracle/rag.py's statistics and edges are the yardstick)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import vector_ref as V
from oracle import rag as O

CASES = V.host_cases()


def rings_of(t, label):
    return [r for r in range(len(t["ring_label"])) if t["ring_label"][r] == label]


def test_tabulated_ring_counts():
    t = V.trace(*CASES["one_pixel"])
    assert len(t["ring_label"]) == 1 and len(t["xy"]) == 4 and t["ring_area2"].tolist() == [2]
    t = V.trace(*CASES["single_label"])
    assert len(t["ring_label"]) == 1 and t["xy"].tolist() == [[0, 0], [7, 0], [7, 5], [0, 5]]
    assert len(t["left"]) == 1 and t["left"][0] == -1 and t["arc_xy"].tolist() == [[0, 0], [7, 0], [7, 5], [0, 5], [0, 0]]
    t = V.trace(*CASES["parity"])                                   # every interior corner is a saddle: no two pixels are joined
    assert len(t["ring_label"]) == 36 and (np.diff(t["ring_ptr"]) == 4).all() and (t["ring_area2"] == 2).all()
    t = V.trace(*CASES["frame_island"])
    frame, island = rings_of(t, 0), rings_of(t, 1)
    assert len(frame) == 2 and len(island) == 1
    assert sorted(np.sign(t["ring_area2"][frame]).tolist()) == [-1, 1] and t["ring_area2"][island[0]] > 0
    inner = [a for a in range(len(t["left"])) if t["left"][a] == 1]
    assert len(inner) == 1 and t["right"][inner[0]] == 0            # the frame-island boundary: one closed arc
    pts = t["arc_xy"][t["arc_ptr"][inner[0]]:t["arc_ptr"][inner[0] + 1]]
    assert (pts[0] == pts[-1]).all() and len(pts) == 6              # it starts inside a straight run: 4 corners + the start twice
    t = V.trace(*CASES["diagonal_holes"])                          # label 0 turns right at the saddle: its two holes are ONE ring,
    assert t["ring_area2"][rings_of(t, 0)].tolist() == [50, -4]     # the two pixels of label 1 stay two rings
    assert t["ring_area2"][rings_of(t, 1)].tolist() == [2, 2]
    t = V.trace(*CASES["hole_meets_outside"])                      # the hole joins the outer ring at the corner: one ring, 7 pixels
    assert t["ring_area2"][rings_of(t, 0)].tolist() == [14]
    t = V.trace(*CASES["absent_ids"])
    assert t["region_ptr"].tolist() == [0, 2, 2, 2, 3, 3, 3]


def test_the_head_of_a_hole_need_not_be_a_vertex_dart():
    """The smallest dart of the frame's hole is the bottom side of pixel (1, 0), in the middle of the hole's top edge."""
    labels, n = CASES["frame_island"]
    d, nxt = V.successor_map(labels)
    pred = {v: k for k, v in nxt.items()}
    assert d[6][:3] == (1, 0, 2) and d[pred[6]][2] == 2


@pytest.mark.parametrize("name", list(CASES) + ["random", "comb"])
def test_properties(name):
    if name == "random":
        labels, n = np.random.default_rng(4).integers(0, 3, (19, 23)).astype(np.int32), 3
    elif name == "comb":
        labels, n = V.comb_of_combs(34), 2
    else:
        labels, n = CASES[name]
    H, W = labels.shape
    d, nxt = V.successor_map(labels)
    assert sorted(nxt.values()) == sorted(d)                        # a permutation of the darts
    pred = {v: k for k, v in nxt.items()}
    t = V.trace(labels, n)
    for head, a2 in zip(t["ring_head"], t["ring_area2"]):
        if a2 > 0:                                                  # an outer ring starts at a corner
            assert d[int(head)][2] != d[pred[int(head)]][2]
    assert np.array_equal(V.rasterise(t, H, W), labels)
    st = O.label_stats(labels, np.zeros((1, H, W), np.uint8), n)
    ring_label = t["ring_label"].astype(np.int64)
    area2, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(area2, ring_label, t["ring_area2"])
    np.add.at(length, ring_label, V.path_length(t["xy"], t["ring_ptr"], closed=True))
    assert np.array_equal(area2, 2 * st["count"]) and np.array_equal(length, st["peri"].sum(1))
    assert np.array_equal(t["region_ptr"][1:] - t["region_ptr"][:-1], np.bincount(ring_label, minlength=n))
    edges, weights = O.rag_edges(labels, n)
    arc_len = V.path_length(t["arc_xy"], t["arc_ptr"], closed=False)
    left, right = t["left"], t["right"]
    per_edge = np.zeros(len(edges), np.int64)
    np.add.at(per_edge, V.arc_edge(left, right, edges)[left >= 0], arc_len[left >= 0])
    assert np.array_equal(per_edge, weights)
    assert arc_len[left < 0].sum() == st["peri"][:, 1].sum()
    assert not ((left >= 0) & (left <= right)).any()
    keys = list(zip(right.tolist(), left.tolist(), t["arc_first"].tolist()))
    assert keys == sorted(keys)
    rkeys = list(zip(t["ring_label"].tolist(), t["ring_head"].tolist()))
    assert rkeys == sorted(rkeys)


def test_the_spec_refuses_what_the_device_refuses():
    with pytest.raises(ValueError):
        V.trace(np.ones((2, 2), np.int32), 1)
    with pytest.raises(ValueError):
        V.trace(-np.ones((2, 2), np.int32), 1)
