"""Framing for the attention kernels' isolation tests, and the float64 reference of the fused core.  Plain torch, any device:
tests/test_attn_frame_host.py checks this file on the CPU, tests/test_gpu_attention_edges.py frames the kernels' tensors with it.

The persistent attention kernels read keys >= N of a sample through a buffer descriptor that returns zero past the sample's rows, and
mask them: the masked probability is exactly 0.  A descriptor that is too long, a stale LDS tail or a missing store guard turns that
into 0 x (whatever lies behind the sample), which is 0 -- and invisible -- as long as whatever lies there is finite.  So the tests
put every tensor a call reads or writes into the middle of one flat allocation whose two ends are NaN, and make the neighbouring
SAMPLES NaN as well:

  framed(t, guard_elems)          a view shaped like t inside [guard | t | guard]; both guards hold `fill` (the quiet NaN of t's dtype);
  guards_intact(handle)           both guards still hold the fill, compared bit for bit on integer views (NaN != NaN would hide a
                                  change, and a NaN written over a NaN of another payload is a change);
  poison_samples(t, parity)       samples b % 2 == parity along dimension 0 become NaN, in place.
"""
import torch

# integer view of each floating-point type, and the bits of its quiet NaN (what torch.full(..., nan) writes; bf16: 0x7fc0)
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64,
             torch.int8: torch.int8, torch.uint8: torch.uint8, torch.int16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64}
NAN_BITS = {torch.bfloat16: 0x7fc0, torch.float16: 0x7e00, torch.float32: 0x7fc00000, torch.float64: 0x7ff8000000000000}


def attn_ref(qkv, bias, scale):
    """fp64 reference of the fused core on CPU.  qkv [B,N,3,H,D] double; bias [H,N,N] or None."""
    q, k, v = qkv[:, :, 0].permute(0, 2, 1, 3), qkv[:, :, 1].permute(0, 2, 1, 3), qkv[:, :, 2].permute(0, 2, 1, 3)
    s = (q * scale) @ k.transpose(-1, -2)
    if bias is not None:
        s = s + bias[None]
    p = torch.softmax(s, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], -1)
    return o, torch.logsumexp(s, -1)


def bits(t):
    """`t` (contiguous) as a flat tensor of same-width integers: equality on it is equality of bit patterns."""
    return t.reshape(-1).view(_INT_VIEW[t.dtype])


class Frame:
    """What guards_intact needs: the flat allocation, where the view starts and ends in it, and the guards' bit pattern."""

    def __init__(self, flat, start, numel, pattern):
        self.flat, self.start, self.numel, self.pattern = flat, start, numel, pattern

    def guards(self):
        """(front, back) as integer views of the flat allocation."""
        b = bits(self.flat)
        return b[:self.start], b[self.start + self.numel:]


def framed(t, guard_elems, fill=None, skew_bytes=16):
    """(view, handle): a copy of `t` (same shape, dtype, device, contiguous) in the middle of one flat allocation
    [guard | t | guard].  Each guard has at least `guard_elems` elements of `fill` (None: NaN for a floating-point type, 0x7fc0 in bf16).
    view.data_ptr() is 16-byte aligned and sits `skew_bytes` (a multiple of 16 below 256) past a 256-byte boundary: the default is
    the alignment the kernels must accept but an allocator never hands out, 0 gives an allocator's."""
    esz = t.element_size()
    if fill is None:
        if not t.dtype.is_floating_point:
            raise ValueError("framed: an integer tensor needs an explicit fill")
        fill = float("nan")
    if guard_elems < 1 or skew_bytes % 16 or not 0 <= skew_bytes < 256:
        raise ValueError(f"framed: guard_elems={guard_elems}, skew_bytes={skew_bytes}")
    slack = 256 // esz                                         # room to move the view to the wanted residue mod 256
    flat = torch.full((2 * guard_elems + t.numel() + 2 * slack,), fill, dtype=t.dtype, device=t.device)
    at = flat.data_ptr() + guard_elems * esz
    start = guard_elems + ((skew_bytes - at) % 256) // esz
    if (flat.data_ptr() + start * esz) % 256 != skew_bytes:
        raise ValueError("framed: the allocation is not aligned to its element size")
    view = flat[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    pattern = bits(torch.full((1,), fill, dtype=t.dtype))[0].item()
    return view, Frame(flat, start, t.numel(), pattern)


def guards_intact(handle):
    """True if every element of both guards still has the fill's bit pattern."""
    front, back = handle.guards()
    return bool((front == handle.pattern).all().item()) and bool((back == handle.pattern).all().item())


def poison_samples(t, parity):
    """Overwrite samples b % 2 == parity along dimension 0 with NaN, in place; returns t."""
    if parity not in (0, 1):
        raise ValueError(f"poison_samples: parity {parity}")
    t[parity::2] = float("nan")
    return t
