"""GPU: the sweep kernels of csrc/dm_sweep.hip (segment_mean, edge_similarity) against the pinned-order oracle at every feature
width 1..128 -- the plain loop below 8, every body length next to every tail length -- on empty, single-point and long segments,
equal rows, special values and a similarity exactly at the margin.  Bit for bit, NaN positions equal."""
import numpy as np
import pytest
import torch

from oracle import sweep as OS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

COUNTS = [0, 1, 1, 2, 3, 40, 1, 1, 5, 0, 7, 9]              # points per segment
S = len(COUNTS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def segments(rng, D):
    """F [P,D], ptr, idx: segment 2 is one point and segment 3 the same point twice, so their pooled rows are equal."""
    ptr = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    P = int(ptr[-1])
    idx = rng.permutation(P).astype(np.int32)
    idx[ptr[3]:ptr[4]] = idx[ptr[2]]
    F = rng.normal(size=(P, D)).astype(np.float32)
    return F, ptr, idx


def edge_list(rng, E):
    """The first E of: the equal rows, a -1 on each side, an edge to each empty segment, then random pairs."""
    fixed = [[2, 3], [-1, 4], [5, -1], [4, 0], [9, 5], [3, 2], [0, 9]]
    e = np.concatenate((np.array(fixed, np.int32), rng.integers(0, S, size=(33, 2)).astype(np.int32)))
    return e[:E]


def assert_same_bits(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), what


def check_dim(D, F, ptr, idx, edge_lists, margin=1.0):
    """segment_mean, then edge_similarity on every edge list, against the strict oracle; returns the simi of each list."""
    from deepmerge_amd import ops
    pooled = ops.segment_mean(dev(F), dev(ptr), dev(idx))
    want_pooled = OS.strict_segment_mean(F, ptr, idx)
    assert_same_bits(pooled.cpu().numpy(), want_pooled, ("pooled", D))
    out = []
    for edges in edge_lists:
        simi, merge = ops.edge_similarity(pooled, dev(edges), margin)
        simi, merge = simi.cpu().numpy(), merge.cpu().numpy()
        want_simi, want_merge = OS.strict_edge_similarity(want_pooled, edges, margin)
        assert_same_bits(simi, want_simi, ("simi", D, len(edges)))
        assert np.array_equal(merge.astype(bool), want_merge), ("merge", D, len(edges))
        assert not merge[np.isnan(simi)].any()
        assert np.isnan(simi[(edges < 0).any(1)]).all()
        out.append(simi)
    return pooled.cpu().numpy(), out


@pytest.mark.parametrize("lo", [1, 33, 65, 97])
def test_every_feature_width(lo):
    for D in range(lo, lo + 32):
        rng = np.random.default_rng(D)
        F, ptr, idx = segments(rng, D)
        lists = [edge_list(rng, E) for E in (1, 7, 8, 9, 33)]
        _, simis = check_dim(D, F, ptr, idx, lists)
        assert len(simis) == 5
        for edges, simi in zip(lists, simis):
            equal = (edges == [2, 3]).all(1) | (edges == [3, 2]).all(1)
            assert equal.any() and (simi[equal] == 0.0).all() and not np.signbit(simi[equal]).any()      # the d < 0 clamp


@pytest.mark.parametrize("D", [129, 192, 193, 300])
def test_segment_mean_beyond_the_pinned_dims(D):
    """The lane loop of segment_mean takes three and more trips; edge_similarity refuses these widths."""
    rng = np.random.default_rng(D)
    F, ptr, idx = segments(rng, D)
    pooled, _ = check_dim(D, F, ptr, idx, [])
    assert not pooled[0].any() and not pooled[9].any()
    assert np.array_equal(pooled[1], F[idx[ptr[1]]]) and np.array_equal(pooled[2], pooled[3])


@pytest.mark.parametrize("D", [7, 8, 100])
def test_special_values(D):
    """A NaN, an Inf, 1e19 (its square, 1e38, is the largest order of magnitude float32 holds) and a pooled 2e19 (its square
    overflows), each in one pooled row, in the plain loop, the body and the tail."""
    rng = np.random.default_rng(D)
    F, ptr, idx = segments(rng, D)
    F[idx[ptr[1]], 3 % D] = np.nan
    F[idx[ptr[6]], 0] = np.inf
    F[idx[ptr[7]], D - 1] = 1e19
    F[idx[ptr[8] + 2], D // 2] = 1e20                       # in a segment of five points: the pooled value is 2e19
    a, b = np.triu_indices(S, 1)
    edges = np.concatenate((np.stack((a, b), 1), [[-1, 6], [7, -1], [6, 6], [7, 7], [8, 8], [1, 1]])).astype(np.int32)
    _, (simi,) = check_dim(D, F, ptr, idx, [edges])
    live = (edges >= 0).all(1)
    touched = np.isin(edges, [1, 6, 8]).any(1) & live
    assert not np.isfinite(simi[touched]).any() and np.isfinite(simi[~touched & live]).all()
    assert np.isnan(simi[touched]).any() and np.isinf(simi[touched]).any()
    assert (simi[(edges == 7).any(1) & ~touched & live & (edges[:, 0] != edges[:, 1])] > 9e18).all()


@pytest.mark.parametrize("D", [1, 8, 9])
def test_the_margin_is_strict(D):
    """Pooled rows e_0 and 0: simi is exactly 1.0, which is not below a margin of 1.0 and is below the next float32."""
    from deepmerge_amd.ExtractFeatures import rag_similarity_sweep
    F = np.zeros((2, D), np.float32)
    F[0, 0] = 1.0
    ptr, idx = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    edges = np.array([[0, 1], [1, 0]], np.int32)
    above = float(np.nextafter(np.float32(1), np.float32(2)))
    for margin, want in ((1.0, False), (above, True)):
        pooled, simi, merge = rag_similarity_sweep(dev(F), dev(ptr), dev(idx), dev(edges), margin)
        assert np.array_equal(pooled.cpu().numpy(), F)
        assert simi.tolist() == [1.0, 1.0] and merge.tolist() == [want, want]
        assert OS.strict_edge_similarity(F, edges, margin)[1].tolist() == [want, want]
