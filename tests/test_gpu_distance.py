"""GPU: the dense pairwise distance (dm_pairwise_distance, ops.pairwise_distance and the drop-ins
ExtractFeatures.Euclidean_distance / MC_Lyu_2020) against the reference's own outputs, a float64 truth,
and the structural contract: exact zeros for equal rows, entries that depend on their two rows only."""
import numpy as np
import pytest
import torch

from oracle import sweep as OS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
NP = {torch.float32: np.float32, torch.float64: np.float64}


def dist(X, Y):
    from deepmerge_amd import ops
    return ops.pairwise_distance(X, Y)


def truth_and_tol(X, Y, eps):
    """float64 truth (the reference formula on float64 copies) and the bound
    dd = (p+3) eps (sum x^2 + sum y^2 + 2 sum |x y|), tol = min(dd / 2D, sqrt(dd)) + 2 eps D."""
    x = np.asarray(X, np.float64); y = np.asarray(Y, np.float64)
    want = OS.euclidean_distance(x.copy(), y.copy())
    p = x.shape[1]
    dd = (p + 3) * eps * ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] + 2 * (np.abs(x) @ np.abs(y).T))
    tol = np.minimum(dd / np.maximum(2 * want, 1e-300), np.sqrt(dd)) + 2 * eps * want
    return want, tol


def assert_within(got, X, Y, eps, what=""):
    want, tol = truth_and_tol(X, Y, eps)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= tol).all(), f"{what}: max err/tol {np.max(err / tol):.3g}"


# ---- 1. the reference's fixtures (tests/golden/sweep.npz: its Euclidean_distance on float32 features) --------------------
@pytest.mark.parametrize("name", ["Euclidean_distance", "MC_Lyu_2020"])
def test_drop_in_matches_reference_fixtures(name):
    from deepmerge_amd import ExtractFeatures as EF
    from test_oracle_sweep import simi_tolerance
    from util import load_fx
    fn = getattr(EF, name)
    fx = load_fx("sweep.npz")
    tags = [str(t) for t in fx["dist/tags"]]
    assert "p3" in tags and "near_margin" in tags
    for tag in tags:
        X, Y, D = fx[f"dist/{tag}/X"], fx[f"dist/{tag}/Y"], fx[f"dist/{tag}/D"]
        got = fn(X, Y)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == D.shape, tag
        tol = simi_tolerance(X[:, None, :], Y[None, :, :], D)
        err = np.abs(got.astype(np.float64) - D.astype(np.float64))
        assert (err <= tol).all(), f"{tag}: max err/tol {np.max(err / tol):.2f}"
        equal = (X[:, None, :] == Y[None, :, :]).all(-1)
        assert (got[equal] == 0).all(), f"{tag}: equal rows must give exactly 0"
        if tag == "near_margin":
            near = np.abs(D.astype(np.float64) - 1.0) <= tol
            assert near.sum() <= 2
            assert np.array_equal((got < 1.0)[~near], (D < 1.0)[~near])


# ---- 2. random shapes against a float64 truth ---------------------------------------------------------------------------------
SIZES = (1, 15, 17, 127, 129, 300)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("p", [1, 3, 4, 5, 100, 129, 768])
def test_random_shapes_against_float64_truth(p, dtype):
    rng = np.random.default_rng(1000 * p + (dtype == torch.float64))
    for n in SIZES:
        for m in SIZES:
            X = rng.normal(size=(n, p)).astype(NP[dtype]) * 0.3
            Y = (rng.normal(size=(m, p)) * 0.3 + 0.05).astype(NP[dtype])
            got = dist(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV))
            assert got.is_cuda and got.dtype == dtype and got.shape == (n, m)
            assert_within(got.cpu().numpy(), X, Y, EPS[dtype], f"n={n} m={m} p={p}")


# ---- 3. exact zeros ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("p", [3, 100, 257])
def test_equal_rows_give_exact_zero(p, dtype):
    g = torch.Generator().manual_seed(p)
    X = (torch.randn(300, p, generator=g) * 2.5 + 1.0).to(dtype)
    Y = (torch.randn(211, p, generator=g) * 2.5 + 1.0).to(dtype)
    pairs = [(5, 3), (130, 70), (257, 129), (299, 210), (17, 200), (64, 64), (0, 131)]   # (row of X, row of Y), off tile edges
    for i, j in pairs:
        Y[j] = X[i]
    Xd, Yd = X.to(DEV), Y.to(DEV)
    D = dist(Xd, Yd).cpu()
    for i, j in pairs:
        assert D[i, j].item() == 0.0, (i, j, D[i, j].item())
    others = torch.ones_like(D, dtype=torch.bool)
    others[[i for i, _ in pairs], [j for _, j in pairs]] = False
    assert (D[others] > 0).all()
    S = dist(Xd, Xd).cpu()
    assert (torch.diagonal(S) == 0).all()
    assert torch.equal(S, S.t()), "D(X, X) must be symmetric bit for bit"


# ---- 4. bitwise structure -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("p", [5, 100, 129])
def test_entries_depend_on_their_two_rows_only(p, dtype):
    g = torch.Generator().manual_seed(7 + p)
    X = torch.randn(300, p, generator=g, dtype=dtype).to(DEV)
    Y = torch.randn(257, p, generator=g, dtype=dtype).to(DEV)
    full = dist(X, Y)
    assert torch.equal(dist(X, Y), full), "two calls must give the same bits"
    for trial in range(4):
        r = torch.randperm(300, generator=g)[: [300, 1, 131, 17][trial]].to(DEV)
        c = torch.randperm(257, generator=g)[: [257, 129, 1, 64][trial]].to(DEV)
        sub = dist(X[r], Y[c])
        assert torch.equal(sub, full[r][:, c]), f"trial {trial}"
    # a NaN in row i of X: row i all NaN, every other row unchanged bit for bit
    Xn = X.clone()
    Xn[131, p // 2] = float("nan")
    got = dist(Xn, Y)
    assert torch.isnan(got[131]).all()
    keep = torch.arange(300, device=DEV) != 131
    assert torch.equal(got[keep], full[keep])


# ---- 5. streams and a result past 2^31 entries -------------------------------------------------------------------------------
def test_side_stream():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(700, 100, generator=g).to(DEV)
    Y = torch.randn(333, 100, generator=g).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D = dist(X, Y)
    s.synchronize()
    assert_within(D.cpu().numpy(), X.cpu().numpy(), Y.cpu().numpy(), EPS[torch.float32], "side stream")


def test_result_beyond_2_to_31_entries():
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GB of free device memory, {free / 2 ** 30:.1f} GB free")
    n = m = 47000
    assert n * m > 2 ** 31
    g = torch.Generator().manual_seed(11)
    X = torch.randn(n, 4, generator=g).to(DEV)
    Y = torch.randn(m, 4, generator=g).to(DEV)
    D = dist(X, Y)
    rng = np.random.default_rng(0)
    flat = np.concatenate([[0, m - 1, (n - 1) * m, n * m - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1],
                           (n - 1) * m + rng.integers(0, m, 64), np.arange(m - 1, n * m, m)[::997],
                           rng.integers(2 ** 31, n * m, 256), rng.integers(0, n * m, 256)]).astype(np.int64)
    rows, cols = flat // m, flat % m
    got = D.view(-1)[torch.from_numpy(flat).to(DEV)].cpu().numpy()
    del D
    torch.cuda.empty_cache()
    x = X.cpu().numpy()[rows].astype(np.float64); y = Y.cpu().numpy()[cols].astype(np.float64)
    want = np.sqrt(np.maximum(0, ((x - y) ** 2).sum(1)))
    dd = 7 * EPS[torch.float32] * ((x * x).sum(1) + (y * y).sum(1) + 2 * np.abs(x * y).sum(1))
    tol = np.minimum(dd / np.maximum(2 * want, 1e-300), np.sqrt(dd)) + 2 * EPS[torch.float32] * want
    assert (np.abs(got - want) <= tol).all()


# ---- 6. argument errors and empty shapes ---------------------------------------------------------------------------------------
def test_argument_errors_and_empty_shapes():
    from deepmerge_amd import ExtractFeatures as EF
    a = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        dist(a, torch.zeros(3, 9, device=DEV))                       # unequal p
    with pytest.raises(ValueError):
        dist(torch.zeros(8, device=DEV), a)                          # 1-D
    with pytest.raises(ValueError):
        dist(a.to(torch.int32), a.to(torch.int32))
    with pytest.raises(ValueError):
        dist(a.to(torch.bfloat16), a.to(torch.bfloat16))
    with pytest.raises(ValueError):
        dist(a, a.double())                                          # mixed dtypes
    assert dist(torch.zeros(0, 8, device=DEV), a).shape == (0, 4)
    assert dist(a, torch.zeros(0, 8, device=DEV)).shape == (4, 0)
    z = dist(torch.zeros(4, 0, device=DEV), torch.zeros(6, 0, device=DEV))
    assert z.shape == (4, 6) and (z == 0).all()
    assert EF.Euclidean_distance(np.zeros((0, 3), np.float32), np.ones((2, 3), np.float32)).shape == (0, 2)


def test_drop_in_types_follow_the_input():
    from deepmerge_amd import ExtractFeatures as EF
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(9, 7)), rng.normal(size=(4, 7))            # float64, numpy's default
    got = EF.Euclidean_distance(X, Y)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert_within(got, X, Y, EPS[torch.float64], "numpy float64")
    t = EF.MC_Lyu_2020(torch.from_numpy(X).float(), torch.from_numpy(Y).float())
    assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.dtype == torch.float32
    c = EF.Euclidean_distance(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV))
    assert c.is_cuda and c.dtype == torch.float64
    assert torch.equal(c.cpu(), torch.from_numpy(got))
