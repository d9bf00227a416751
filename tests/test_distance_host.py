"""CPU: the dense distance entry point validates its arguments before any launch, and the drop-ins keep the
reference's signatures (ExtractFeatures.py:119 `Euclidean_distance(X, Y)`, :228 `MC_Lyu_2020(X, Y)`)."""
import inspect
import os

import pytest


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    from deepmerge_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib


def test_pairwise_distance_validates_without_a_gpu(built_lib):
    lib = built_lib.lib()
    assert built_lib.DM_F64 == 3
    assert lib.dm_pairwise_distance(1, 1, 1, 0, 4, 4, built_lib.DM_F32, None) == -1
    assert b"dm_pairwise_distance" in lib.dm_last_error()
    assert lib.dm_pairwise_distance(1, 1, 1, 4, 4, 0, built_lib.DM_F64, None) == -1
    assert lib.dm_pairwise_distance(None, 1, 1, 4, 4, 4, built_lib.DM_F32, None) == -1
    assert lib.dm_pairwise_distance(1, 1, 1, 4, 4, 4, built_lib.DM_BF16, None) == -2
    assert b"dm_pairwise_distance" in lib.dm_last_error()
    assert lib.dm_pairwise_distance(1, 1, 1, 4, 4, 4, 7, None) == -2


def test_drop_in_signatures_are_the_reference_ones():
    from deepmerge_amd import ExtractFeatures as EF
    for fn in (EF.Euclidean_distance, EF.MC_Lyu_2020):
        assert list(inspect.signature(fn).parameters) == ["X", "Y"]


def test_pairwise_distance_refuses_host_tensors():
    import torch
    from deepmerge_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pairwise_distance(torch.zeros(2, 3), torch.zeros(4, 3))
