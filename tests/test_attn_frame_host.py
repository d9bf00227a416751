"""CPU: the framing helper of the attention isolation tests (tests/attn_frame.py) does what tests/test_gpu_attention_edges.py relies
on -- a guard check that misses a change would let every isolation case pass."""
import numpy as np
import pytest
import torch

import attn_frame as F

DTYPES = [torch.bfloat16, torch.float32, torch.float64]


def _values(shape, dtype, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=shape).astype(np.float32)).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,guard", [((3, 37, 3, 2, 64), 64 * 3 * 2 * 64), ((4, 2, 37), 64), ((5,), 1)])
def test_round_trip(dtype, shape, guard):
    """The view holds the tensor's values in its shape, contiguous, inside one allocation whose two ends hold the NaN pattern."""
    t = _values(shape, dtype)
    view, h = F.framed(t, guard)
    assert view.shape == t.shape and view.dtype == t.dtype and view.is_contiguous()
    assert torch.equal(F.bits(view), F.bits(t))
    assert view.data_ptr() == h.flat.data_ptr() + h.start * t.element_size()
    front, back = h.guards()
    assert front.numel() >= guard and back.numel() >= guard
    assert front.numel() + back.numel() + t.numel() == h.flat.numel()
    assert h.pattern == F.NAN_BITS[dtype]
    assert torch.isnan(h.flat[:h.start]).all() and torch.isnan(h.flat[h.start + h.numel:]).all()
    assert F.guards_intact(h)
    view.mul_(2)                                                  # writing every element of the view leaves the guards alone
    assert F.guards_intact(h) and torch.equal(view, t * 2)


def test_bf16_nan_is_7fc0():
    _, h = F.framed(torch.zeros(8, dtype=torch.bfloat16), 4)
    assert h.pattern == 0x7fc0 and (h.guards()[0] == 0x7fc0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("skew", [0, 16, 48, 240])
def test_alignment(dtype, skew):
    """16-byte aligned always; the residue mod 256 is the one asked for (default 16: never what an allocator returns)."""
    for numel in (1, 7, 64, 1000):
        view, h = F.framed(_values((numel,), dtype), 3, skew_bytes=skew)
        assert view.data_ptr() % 16 == 0 and view.data_ptr() % 256 == skew and F.guards_intact(h)
    view, _ = F.framed(_values((5,), dtype), 3)
    assert view.data_ptr() % 256 == 16


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_changed_guard_element_is_detected(dtype):
    """Either side, first / last / nearest element, a finite value or a NaN of another payload."""
    t = _values((2, 5, 8), dtype)
    def places(h):            # (where the view starts moves with the allocation's address)
        n_front, n_back, back0 = h.guards()[0].numel(), h.guards()[1].numel(), h.start + h.numel
        return (0, n_front // 2, n_front - 1, back0, back0 + n_back // 2, back0 + n_back - 1)

    for k in range(6):
        view, h = F.framed(t, 16)
        pos = places(h)[k]
        h.flat[pos] = 0.0
        assert not F.guards_intact(h), pos
        assert torch.equal(F.bits(view), F.bits(t))
        view, h = F.framed(t, 16)
        pos = places(h)[k]
        F.bits(h.flat)[pos] = h.pattern | 1                       # still a NaN: only the bitwise comparison sees it
        assert torch.isnan(h.flat[pos]) and not F.guards_intact(h), pos
        view, h = F.framed(t, 16)
        pos = places(h)[k]
        F.bits(h.flat)[pos] = -1                                  # the NaN with every bit set
        assert torch.isnan(h.flat[pos]) and not F.guards_intact(h), pos


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_nan_in_a_finite_guard_is_detected(dtype):
    """A quiet NaN written over a NaN guard leaves the same bits (the isolation tests therefore give every edge sample a run in which
    it is finite); with a finite fill the same write is seen."""
    t = _values((3, 8), dtype)
    for side in (0, 1):
        view, h = F.framed(t, 16, fill=1.5)
        assert F.guards_intact(h) and not torch.isnan(h.flat).any()
        h.flat[h.start - 1 if side == 0 else h.start + h.numel] = float("nan")
        assert not F.guards_intact(h)
    view, h = F.framed(t, 16)
    view[1, 2] = float("nan")                                     # inside the view: not the guards' business
    assert F.guards_intact(h)


def test_integer_tensors_take_an_explicit_fill():
    t = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    with pytest.raises(ValueError):
        F.framed(t, 4)
    view, h = F.framed(t, 4, fill=-7)
    assert torch.equal(view, t) and F.guards_intact(h)
    h.flat[h.start - 1] = 0
    assert not F.guards_intact(h)


def test_bad_arguments_are_refused():
    t = torch.zeros(4)
    for kw in ({"skew_bytes": 8}, {"skew_bytes": 256}, {"skew_bytes": -16}):
        with pytest.raises(ValueError):
            F.framed(t, 4, **kw)
    with pytest.raises(ValueError):
        F.framed(t, 0)
    with pytest.raises(ValueError):
        F.poison_samples(t, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 2, 4, 5])
@pytest.mark.parametrize("parity", [0, 1])
def test_poison_samples_touches_only_its_samples(dtype, B, parity):
    t = _values((B, 6, 3, 2, 8), dtype, seed=B)
    view, h = F.framed(t, 32)
    assert F.poison_samples(view, parity) is view
    for b in range(B):
        if b % 2 == parity:
            assert torch.isnan(view[b]).all()
        else:
            assert torch.equal(F.bits(view[b].contiguous()), F.bits(t[b].contiguous()))
    assert F.guards_intact(h)


def test_attn_ref_is_softmax_attention():
    """The reference against torch's own scaled_dot_product_attention in float64 (bias as an additive mask)."""
    rng = np.random.default_rng(3)
    B, N, H, D = 2, 19, 3, 8
    qkv = torch.from_numpy(rng.normal(size=(B, N, 3, H, D)))
    bias = torch.from_numpy(rng.normal(size=(H, N, N)))
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    for b in (None, bias):
        o, lse = F.attn_ref(qkv, b, 0.3)
        want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=None if b is None else b[None], scale=0.3)
        assert (o - want.permute(0, 2, 1, 3).reshape(B, N, H * D)).abs().max().item() < 1e-12
        s = (q * 0.3) @ k.transpose(-1, -2) + (0 if b is None else b[None])
        assert (lse - s.exp().sum(-1).log()).abs().max().item() < 1e-12
