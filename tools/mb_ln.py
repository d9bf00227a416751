"""LayerNorm forward / backward device time per launch at the encoder's shapes (rows x 768 for rows = 16384 / 4096 / 1024: bf16 result
forward; bf16 upstream gradient, residual-gradient add and bf16 copy of dx backward) against the bytes each must move.

Each figure is a hipGraph replay of 30 launches of the kernel alone (as tools/mb_attn.py times attention): the library entry points are
called on buffers allocated beforehand, the backward through dm_layernorm_bwd_partials, so neither the partial-row reduce launch nor an
allocation nor the host's ~15 us per call is in it.  The launches rotate over enough operand sets that no launch finds its operands in
the 256 MiB Infinity Cache.  ROWS / COLS override the shapes; DM_LN_WG sets the backward's workgroup count (= partial rows)."""
import ctypes as C
import os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from deepmerge_amd import _lib, ops
dev = "cuda:0"
N_LAUNCH = 30
cols = int(os.environ.get("COLS", 768))
row_list = [int(r) for r in os.environ["ROWS"].split(",")] if "ROWS" in os.environ else [16384, 4096, 1024]
lib = _lib.lib()


def replay_time(launch, n=N_LAUNCH, reps=5):
    """Device time per launch: launch(0..n-1) captured into one hipGraph, best of `reps` replays."""
    for i in range(3): launch(i)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch(0); torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            for i in range(n): launch(i)
    graph.replay(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter(); graph.replay(); torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t) / n)
    return best


for rows in row_list:
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    per_set = rows * cols * 22                   # x, dres, dx fp32; dy, y, dx copy bf16
    nset = min(N_LAUNCH, max(6, -(-600_000_000 // per_set)))
    f32 = lambda: torch.randn((rows, cols), device=dev, generator=gen)
    xs, drs = [f32() for _ in range(nset)], [f32() for _ in range(nset)]
    dys = [f32().to(torch.bfloat16) for _ in range(nset)]
    ys = [torch.empty((rows, cols), device=dev, dtype=torch.bfloat16) for _ in range(nset)]
    dxs = [torch.empty((rows, cols), device=dev) for _ in range(nset)]
    lps = [torch.empty((rows, cols), device=dev, dtype=torch.bfloat16) for _ in range(nset)]
    gamma, beta = torch.randn(cols, device=dev, generator=gen), torch.randn(cols, device=dev, generator=gen)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    part = torch.empty(lib.dm_layernorm_bwd_partial_floats(cols), device=dev)
    n_part = C.c_int32(0)

    def fwd(i):
        k = i % nset
        _lib.check(lib.dm_layernorm_fwd(xs[k].data_ptr(), gamma.data_ptr(), beta.data_ptr(), ys[k].data_ptr(), _lib.DM_BF16, mean.data_ptr(),
                                       rstd.data_ptr(), rows, cols, 1e-6, torch.cuda.current_stream().cuda_stream), "dm_layernorm_fwd")

    def bwd(i):
        k = i % nset
        _lib.check(lib.dm_layernorm_bwd_partials(dys[k].data_ptr(), _lib.DM_BF16, xs[k].data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), drs[k].data_ptr(), dxs[k].data_ptr(), lps[k].data_ptr(), part.data_ptr(),
                                                rows, cols, C.byref(n_part), torch.cuda.current_stream().cuda_stream),
                  "dm_layernorm_bwd_partials")

    t = replay_time(fwd)
    print(f"fwd  rows={rows:6d} cols={cols}: {t*1e6:6.1f} us  {rows*cols*6/t/1e12:5.2f} TB/s (4 B in + 2 B out per element; {nset} operand sets)")
    t = replay_time(bwd)      # mean / rstd are those of the last forward: the backward's time does not depend on the values
    print(f"bwd  rows={rows:6d} cols={cols}: {t*1e6:6.1f} us  {rows*cols*16/t/1e12:5.2f} TB/s (2 + 4 + 4 B in, 4 + 2 B out per element; "
          f"{n_part.value} partial rows, their reduce launch not included)")
    del xs, drs, dys, ys, dxs, lps
    torch.cuda.empty_cache()
