"""GPU: the four-workgroups-per-CU 128 x 128 bf16 GEMM (dm_gemm_q4.hip) through the C-ABI.

Exact small-integer products catch any lane / swizzle / DMA-address mistake as a bit mismatch (ragged M and N exercise the zero-filled
DMA and the masked stores; M is a multiple of 64, which the family requires); the fused epilogues are compared bit for bit with the
register-staged 128 x 128 kernel (dm_gemm.hip), which runs the same MFMAs in the same K order.  Every test checks, by kernel name, which
kernel actually ran.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OTHERS_OFF = {"DM_GEMM_W4": "0", "DM_GEMM_RING": "0", "DM_GEMM_256": "0"}


def _env(monkeypatch, **kv):
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _ints(rng, shape, lo=-3, hi=4):
    return torch.from_numpy(rng.integers(lo, hi, size=shape).astype(np.float32))


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type.name == "CUDA"]


def _ran_q4(names):
    return any("gemm_q4_kernel" in n for n in names)


@pytest.mark.parametrize("layout", ["NT", "NN"])
@pytest.mark.parametrize("M,N,K", [(1088, 768, 768), (320, 2304, 768), (576, 3072, 768), (192, 200, 448), (64, 136, 64),
                                   (4096, 768, 768)])
def test_gemm_q4_exact_integers(monkeypatch, layout, M, N, K):
    from deepmerge_amd import ops
    from deepmerge_amd._lib import DM_NN, DM_NT
    _env(monkeypatch, DM_GEMM_Q4="2", **OTHERS_OFF)
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    a = _ints(rng, (M, K))
    b = _ints(rng, (N, K))
    want = a.double() @ b.double().T
    A = a.to(DEV).bfloat16()
    B_ = (b if layout == "NT" else b.T.contiguous()).to(DEV).bfloat16()
    C = torch.full((M, N), float("nan"), device=DEV)
    names = _kernel_names(lambda: ops.gemm(DM_NT if layout == "NT" else DM_NN, A, B_, C, M, N, K))
    assert _ran_q4(names), names
    got = C.cpu().double()
    assert torch.equal(got, want), f"max diff {(got - want).abs().max()}"


def _epilogue_case(name, layout, M, N, K, seed):
    """Operands and keyword arguments of one fused epilogue; outputs are fresh tensors so two runs can be compared."""
    from deepmerge_amd._lib import DM_EPI_GELU_GRAD, DM_EPI_MUL
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    B = (torch.randn(N, K, device=DEV, generator=g) if layout == "NT" else torch.randn(K, N, device=DEV, generator=g)).bfloat16() * 0.05
    bias = torch.randn(N, device=DEV, generator=g)
    res = torch.randn(M, N, device=DEV, generator=g)
    saved = torch.randn(M, N, device=DEV, generator=g).bfloat16()

    def run():
        if name == "bf16":
            C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            return [C], dict()
        if name == "bias":
            C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            return [C], dict(bias=bias)
        if name == "rf":
            C = torch.empty(M, N, device=DEV)
            return [C], dict(bias=bias, residual=res)
        if name == "e3h":
            C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            aux = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            return [C, aux], dict(bias=bias, epilogue=DM_EPI_GELU_GRAD, aux=aux, ldaux=N)
        if name == "e4h":
            C = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            return [C], dict(epilogue=DM_EPI_MUL, aux=saved, ldaux=N)
        raise ValueError(name)
    return A, B, run


@pytest.mark.parametrize("name,layout,M,N", [("bf16", "NN", 2048, 768), ("bias", "NT", 2048, 2304), ("rf", "NT", 2048, 768),
                                             ("e3h", "NT", 2048, 3072), ("e4h", "NN", 2048, 3072), ("rf", "NT", 1088, 768),
                                             ("e3h", "NT", 704, 3072), ("e4h", "NN", 1088, 3072), ("bias", "NT", 4096, 3072)])
def test_gemm_q4_epilogues_match_128x128(monkeypatch, name, layout, M, N):
    """Each fused epilogue the routed products use: bit-identical to the register-staged 128 x 128 kernel on random bf16 data."""
    from deepmerge_amd import ops
    from deepmerge_amd._lib import DM_NN, DM_NT
    K = 768
    A, B, run = _epilogue_case(name, layout, M, N, K, seed=M + N)
    outs = []
    for q4, env in ((True, {"DM_GEMM_Q4": "2", **OTHERS_OFF}), (False, {"DM_GEMM_Q4": "0", "DM_GEMM_FORCE_TILE": "128", **OTHERS_OFF})):
        _env(monkeypatch, **env)
        if "DM_GEMM_FORCE_TILE" not in env:
            monkeypatch.delenv("DM_GEMM_FORCE_TILE", raising=False)
        tensors, kw = run()
        names = _kernel_names(lambda: ops.gemm(DM_NT if layout == "NT" else DM_NN, A, B, tensors[0], M, N, K, **kw))
        assert _ran_q4(names) == q4, names
        if not q4:
            assert any("gemm_kernel" in n for n in names), names
        outs.append(tensors)
    for q4, t128 in zip(*outs):
        assert torch.isfinite(q4.float()).all()
        assert torch.equal(q4, t128), f"{name}: max diff {(q4.float() - t128.float()).abs().max()}"


# (layout, M, N, K, epilogue) of the step's products that the routing rule sends to this family
# (layout, M, N, K, epilogue, routed): the step's products, and whether the routing rule sends them to this family (the proj forward,
# NT 16384 x 768 + fp32 residual, measured no faster and stays on the 128 x 128 kernel)
ROUTED = [("NT", 16384, 3072, 768, "e3h", True), ("NN", 16384, 3072, 768, "e4h", True), ("NT", 16384, 2304, 768, "bias", True),
          ("NN", 16384, 768, 768, "bf16", True), ("NT", 4096, 3072, 768, "e3h", True), ("NN", 4096, 3072, 768, "e4h", True),
          ("NT", 16384, 768, 768, "rf", False)]


@pytest.mark.parametrize("layout,M,N,K,name,routed", ROUTED)
def test_gemm_q4_routed_shapes(monkeypatch, layout, M, N, K, name, routed):
    from deepmerge_amd import ops
    from deepmerge_amd._lib import DM_NN, DM_NT
    for k in ("DM_GEMM_Q4", "DM_GEMM_ROUTE", "DM_GEMM_FORCE_TILE", *OTHERS_OFF):
        monkeypatch.delenv(k, raising=False)
    A, B, run = _epilogue_case(name, layout, M, N, K, seed=1)
    tensors, kw = run()
    names = _kernel_names(lambda: ops.gemm(DM_NT if layout == "NT" else DM_NN, A, B, tensors[0], M, N, K, **kw))
    assert _ran_q4(names) == routed, names
