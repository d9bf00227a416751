"""No GPU: the spec, the data, the bounds and the case table of the GEMM epilogue tests (tests/gemm_ref.py) are pinned here.

  * epilogue_ref equals the same thing built from torch float64 operators (F.gelu, autograd for GELU');
  * every EXACT configuration is exact on these inputs: the float32 restatement equals the float64 spec bit for bit in both association
    orders and with or without fused multiply-add;
  * every BOUNDED configuration's float32 restatement stays at or below half its bound, and no constant is larger than that needs;
  * the case table is well formed: the extents each family needs, 16-byte aligned views, >= 256 rows and >= 8 columns of sentinel, the
    grouped cube inside its allocation, every skip documented;
  * the DM_GEMM_* switches the GPU test clears for its children are exactly the ones the library reads.
  * the weight-gradient tests (tests/test_gpu_gemm_wgrad.py): the restated split rules give the slice structure of every shape, the data
    sums exactly in float32 in adversarial orders and needs more than 8 significand bits, the frames guard every operand.
  * the main-loop tests (tests/test_gpu_gemm_mainloop.py): every prefix sum of every contraction is a float32 in natural, reversed, per-tile,
    per-segment and per-slice order; the accumulator restated under each fault of a K loop (a tile dropped or used twice, a segment read from
    the wrong plane or computed as lo lo, a seam one tile off, a K tail dropped or read from the next row) differs from the spec in every
    16 x 16 block; which family takes which K and k_fold, with the plan's line; the plane-pair frames.

Worst err / tol of the restatements is printed ("[gemm_host] ..."; run with -s); the table is at the top of tests/test_gpu_gemm_epilogues.py.
"""
import glob
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref as G

SHAPES = sorted({f["shape"] for f in G.FAMILIES.values()})
# the (shape, fast) pairs that occur: fast parts with bf16 operands, erff with fp32 operands
SHAPE_FAST = sorted({(f["shape"], f["fast"]) for f in G.FAMILIES.values()})


def _torch_ref(acc, cfg):
    """The epilogue from torch float64 operators."""
    v = torch.from_numpy(np.array(acc))
    if cfg["bias_v"] is not None:
        v = v + torch.from_numpy(np.array(cfg["bias_v"]))[None, :]
    out = {}
    gelu = torch.nn.functional.gelu

    def grad(x):
        x = x.clone().requires_grad_(True)
        gelu(x).sum().backward()
        return x.grad

    if cfg["epi"] == "gelu":
        out["aux_v"] = v
        v = gelu(v)
    elif cfg["epi"] == "gelu_grad":
        out["aux_v"] = grad(v)
        v = gelu(v)
    elif cfg["epi"] == "dgelu":
        v = v * grad(torch.from_numpy(np.array(cfg["aux_v"])))
    elif cfg["epi"] == "mul":
        v = v * torch.from_numpy(np.array(cfg["aux_v"]))
    if cfg["res_v"] is not None:
        v = v + torch.from_numpy(np.array(cfg["res_v"]))
    if cfg["old_c"] is not None:
        v = v + torch.from_numpy(np.array(cfg["old_c"]))
    out["v"] = v
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_epilogue_ref_equals_torch_float64(shape):
    M, N, K = shape
    acc = G.operands(M, N, K)["acc"]
    for cfg in G.CONFIGS:
        c = G.case(cfg, M, N, K)
        ref, want = G.epilogue_ref(acc, c), _torch_ref(acc, c)
        # float64 on both sides: the two differ by the rounding of erf / exp and of x / sqrt(2), a few 2^-53 of the magnitudes involved
        scale = 1.0 + np.abs(acc).max()
        assert np.abs(ref["v"] - want["v"].numpy()).max() <= 8 * 2.0 ** -53 * scale, cfg["name"]
        if "aux_v" in ref:
            assert np.abs(ref["aux_v"] - want["aux_v"].numpy()).max() <= 8 * 2.0 ** -53 * scale, cfg["name"]
        if cfg["epi"] in ("none", "mul"):
            assert np.array_equal(ref["v"], want["v"].numpy()), cfg["name"]
        # the rounding of c_dtype, against torch's casts
        if cfg["c"] == G.PAIR:
            hi = torch.from_numpy(ref["v"]).float().bfloat16()
            lo = (torch.from_numpy(ref["v"]) - hi.double()).float().bfloat16()      # (the spec is float64: v - hi is not rounded to fp32 first)
            assert np.array_equal(ref["c"], hi.double().numpy()) and np.array_equal(ref["c_lo"], lo.double().numpy())
        else:
            dt = torch.float32 if cfg["c"] == G.F32 else torch.bfloat16
            assert np.array_equal(ref["c"], torch.from_numpy(ref["v"]).float().to(dt).double().numpy()), cfg["name"]


def test_grouped_rows_restate_dm_gemm_row():
    """(m / rows_per_group) * group_stride + (m % rows_per_group) * ld, spelled out row by row; a group ends inside a 16-row MFMA tile and
    inside an 8-row item."""
    ld, gs = 208, 41 * 208 + 64
    ro = G.row_offsets(328, ld, 41, gs)
    assert [int(ro[m]) for m in (0, 1, 40, 41, 42, 327)] == [0, ld, 40 * ld, gs, gs + ld, 7 * gs + 40 * ld]
    assert np.array_equal(G.row_offsets(5, 7), np.arange(5) * 7)
    assert G.GROUP_ROWS % 8 != 0 and G.GROUP_ROWS % 16 != 0 and all(t % G.GROUP_ROWS for t in (64, 128, 256))


@pytest.mark.parametrize("shape", SHAPES)
def test_data_is_exact_and_spans_the_gelu_range(shape):
    M, N, K = shape
    d = G.operands(M, N, K)
    bf = lambda x: torch.from_numpy(np.array(x)).float().bfloat16().double().numpy()
    assert np.array_equal(bf(d["a"]), d["a"]) and np.array_equal(bf(d["b"]), d["b"])                 # operands exact in bf16
    assert np.array_equal(d["acc"].astype(np.float32).astype(np.float64), d["acc"])                  # the accumulator is a float32
    assert np.array_equal(bf(d["aux_mul"]), d["aux_mul"])                                             # the bf16 aux that is read
    for k in ("bias", "res", "old_c", "aux_mul", "aux_dgelu"):
        assert np.array_equal(np.round(d[k] * 64) / 64, d[k]), k                                      # the 2^-6 grid
    # every partial sum of integer products fits: |sum| <= 4 K 2^-shift needs log2(4 K) bits
    assert 4 * K < 2 ** 24
    pre = d["acc"] + d["bias"][None, :]
    for x in (pre, d["aux_dgelu"]):
        assert (x == 0).any() and (x >= 5.5).any() and (x <= -5.5).any() and ((x > 0) & (x < 0.02)).any() and ((x < 0) & (x > -0.02)).any()
    assert 1.0 <= d["acc"].std() <= 2.5 and np.abs(pre).max() < 16
    # saturated tails: erf(6 / sqrt 2) is 1 in float32, erf(5.5 / sqrt 2) its neighbour below
    sat = lambda x: np.float32(torch.special.erf(torch.tensor(x / np.sqrt(2.0), dtype=torch.float64)).item())
    assert sat(6.0) == np.float32(1.0) and sat(5.5) == np.nextafter(np.float32(1.0), np.float32(0.0))
    assert (pre == 6.0).any() and (pre == -6.0).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_configurations_are_exact_in_float32(shape):
    M, N, K = shape
    acc = G.operands(M, N, K)["acc"]
    for cfg in G.CONFIGS:
        c = G.case(cfg, M, N, K)
        c_exact, aux_exact = G.is_exact(cfg)
        ref = G.epilogue_ref(acc, c)
        for order in ("left", "right"):
            for fma in (False, True):
                for fast in (True, False):
                    r = G.restate32(acc, c, fast, order, fma)
                    if c_exact:
                        assert np.array_equal(r["v"].astype(np.float64), ref["v"]), (cfg["name"], order, fma)
                        assert np.array_equal(np.signbit(r["v"]), np.signbit(ref["v"])), cfg["name"]
                    if aux_exact and "aux_v" in ref:
                        assert np.array_equal(r["aux_v"].astype(np.float64), ref["aux_v"]), (cfg["name"], order, fma)
    # the exact class covers what the issue lists
    assert [c["name"] for c in G.CONFIGS if G.is_exact(c)[0]] == ["none_f32", "none_bf16", "bias_res_f32", "acc_f32", "bias_res_acc_f32", "mul_bf16", "grouped41"]


def _worst_ratios(consts):
    """Worst err / tol of the float32 restatement per (fast, kind) over every shape and bounded configuration; bf16 destinations included."""
    worst = {}
    for shape, fast in SHAPE_FAST:
        M, N, K = shape
        acc = G.operands(M, N, K)["acc"]
        for cfg in G.CONFIGS:
            if all(G.is_exact(cfg)) or (cfg["c"] == G.PAIR and not fast):
                continue
            c = G.case(cfg, M, N, K)
            ref = G.epilogue_ref(acc, c)
            tol = G.bounds(cfg, ref, acc, fast, consts)
            for fma in (False, True):
                r = G.restate32(acc, c, fast, "left", fma)
                if tol["c"] is not None:
                    cdt = G.BF16 if cfg["c"] == G.PAIR else cfg["c"]
                    if cfg["c"] == G.PAIR:
                        hi = G.round_bf16(r["v"].astype(np.float64))
                        got = hi + G.round_bf16(r["v"].astype(np.float64) - hi)
                    else:
                        got = G.round_to(r["v"].astype(np.float64), cdt)
                    kind = "muld" if cfg["epi"] == "dgelu" else "gelu"
                    key = (fast, kind, cdt if cfg["c"] != G.PAIR else G.PAIR)
                    worst[key] = max(worst.get(key, 0.0), G.worst(np.abs(got - ref["v"]), tol["c"]))
                if tol["aux"] is not None:
                    got = G.round_to(r["aux_v"].astype(np.float64), cfg["aux"][0])
                    key = (fast, "dgelu", cfg["aux"][0])
                    worst[key] = max(worst.get(key, 0.0), G.worst(np.abs(got - ref["aux_v"]), tol["aux"]))
    return worst


def test_bounded_restatements_stay_below_half_their_bounds_with_the_smallest_constants():
    worst = _worst_ratios(None)
    for key, r in sorted(worst.items(), key=str):
        print(f"  [gemm_host] {'fast' if key[0] else 'erff'} {key[1]:<6s} -> {key[2]:<5s} err/tol = {r:.3f}")
        assert r <= 0.5, (key, r)
    # no constant can be one smaller: some destination of its kind then exceeds half the bound
    for ck, cv in G.C.items():
        assert cv >= 1
        if cv == 1:
            continue
        less = dict(G.C)
        less[ck] = cv - 1
        w = _worst_ratios(less)
        assert max(r for key, r in w.items() if key[:2] == ck) > 0.5, (ck, cv)
    # every kind the GPU test checks has been measured here
    assert {k[:2] for k in worst} == set(G.C)


def test_case_table_is_well_formed():
    assert [c["id"] for c in G.CONFIGS] == list(range(1, 15)) and len(G.CONFIG) == 14
    # lean keys as the issue's table names them
    keys = {c["name"]: G.lean_key(c) for c in G.CONFIGS}
    assert keys["none_f32"] == 8 and keys["none_bf16"] == 0 and keys["bias_res_f32"] == 9 and keys["acc_f32"] == 10
    assert keys["gelu_save_bf16"] == 16 == keys["gelugrad_save_bf16"] and keys["mul_bf16"] == 4 and keys["gelu_bf16_nosave"] == 0
    for name in ("bias_res_acc_f32", "gelu_save_f32", "dgelu_f32_res"):                     # the run-time lean form
        assert keys[name] >= 0 and keys[name] not in G.SPECIALISED_KEYS
    assert all(f in G.FAMILIES and G.FAMILIES[f]["tile"] == (64, 64) and n == "mul_bf16" for f, n in G.STRIP_ZERO_SIGN)
    assert keys["pair_gelu"] == 1 << 8 and keys["grouped41"] == -1 == keys["grouped41_gelugrad"]
    assert set(G.FAMILIES) == {"t64", "t128", "f32_t64", "f32_t128", "ring8", "ring4", "q4", "t96", "w4", "p256", "kslices", "generic"}

    for fam, f in G.FAMILIES.items():
        M, N, K = f["shape"]
        tm, tn = f["tile"]
        wm, wn = f["wave"]
        assert (M + tm - 1) // tm >= 2 and (N + tn - 1) // tn >= 2, fam                     # two tiles each way
        assert M % tm != 0, fam                                                             # ragged M
        last = (M // tm) * tm
        blocks = range(last, last + tm, wm)
        if fam != "generic":                                                                # (16 x 16 outputs, one per thread: no wave block)
            assert any(b >= M for b in blocks), fam                                         # a wave block that starts past M
            if fam not in ("q4", "t96"):                                                    # (q4 and t96 take M % 64 == 0: their guard)
                assert any(b < M < b + wm for b in blocks), fam                             # a partially filled wave block
                assert M % 16 != 0, fam                                                     # ... that ends inside a 16-row MFMA tile
        assert N % 8 == 0
        if fam == "w4":
            assert N % 192 == 0 and K % 128 == 0                                            # dm_gemm_w4_plan
        else:
            assert N % tn != 0 and (N % wn) == 8, fam                                       # an N tail that ends inside a wave's columns
        steps = (K + f["bk"] - 1) // f["bk"]
        assert fam in ("kslices", "generic") or 2 <= steps <= (4 if fam == "w4" else 3), fam
        if f["ab"] == G.F32 and fam != "generic":
            assert ((M + 127) // 128) * ((N + 127) // 128) >= 16 and K % 4 == 0              # stays off the generic path (gemm_prepare)
        if fam == "generic":
            assert K % 4 != 0
        if fam == "q4":
            assert M % 64 == 0
            assert set(G.family_configs(fam)) == {c["name"] for c in G.CONFIGS if G.lean_key(c) in G.SPECIALISED_KEYS}
        if fam == "t96":                                                                    # dm_gemm_t96_plan: no epilogue, no accumulate, three lean keys
            assert M % 64 == 0 and f["codes"] == (12896,) and f["env"]["DM_GEMM_T96"] == "2" and f["layouts"] == ("NT", "NN")
            assert set(G.family_configs(fam)) == {c["name"] for c in G.CONFIGS if c["epi"] == "none" and not c["acc"]
                                                  and G.lean_key(c) in (0, 1 << 3, 1 | (1 << 3))} == {"none_f32", "none_bf16", "bias_res_f32"}
        assert f["env"].get("DM_GEMM_T96") == ("2" if fam == "t96" else "0"), fam           # every other family switches it off
        if fam == "kslices":
            assert G.plan_fwd_split(M, N, K) == (2, 64) and "DM_GEMM_FORCE_TILE" in f["env"] and f["env"]["DM_GEMM_FORCE_TILE"] is None
        else:
            assert G.plan_fwd_split(M, N, K) == (1, 0), fam
        if f["ab"] == G.BF16:
            assert K % 8 == 0
        # documented skips only, each with the refusing line
        assert set(f["skips"]) <= set(G.ALL) and all(".hip" in why and "`" in why for why in f["skips"].values()), fam
        assert len(G.family_cases(fam)) == len(f["layouts"]) * (14 - len(f["skips"]))
        if fam in ("t64", "t128", "ring8", "ring4", "w4", "p256", "kslices"):
            assert not f["skips"], fam

        for cfg in G.CONFIGS:
            b = G.buffers(cfg, M, N)
            lds = []
            for op in ("c", "aux", "res"):
                if op not in b:
                    continue
                o = b[op]
                size = 4 if o["dtype"] == G.F32 else 2
                idx = o["idx"]
                assert idx.shape == (M, N) and idx.min() == G.VIEW_OFFSET == 8
                assert (G.VIEW_OFFSET * size) % 16 == 0 and (o["ld"] * size) % 16 == 0      # 16-byte aligned view and rows
                assert (b["group_stride"] * size) % 16 == 0
                assert len(np.unique(idx)) == M * N                                         # no two outputs share an element
                top = int(idx.max()) + (o.get("plane", 0))
                assert o["elems"] - 1 - top >= G.PAD_ROWS * o["ld"] >= 256 * N          # >= 256 rows of sentinel below the last row
                if cfg["c"] == G.PAIR and op == "c":
                    assert o["ld"] == N and o["plane"] == M * N and o["plane"] % 8 == 0
                else:
                    assert o["ld"] - N >= 8                                                 # >= 8 columns of sentinel right of N
                    lds.append(o["ld"])
            if cfg["grouped"]:
                assert b["rows_per_group"] == 41 and b["group_stride"] == 41 * (N + 8) + 64 and set(lds) == {N + 8}
                groups = (M + 40) // 41
                assert b["c"]["elems"] >= G.VIEW_OFFSET + groups * b["group_stride"] + 256 * (N + 8)      # the cube fits
            else:
                assert len(set(lds)) == len(lds)                                            # all leading dimensions differ
                assert b["rows_per_group"] == 0


def test_switch_list_is_what_the_library_reads():
    """The DM_GEMM_* names the library hands to getenv are, as a set, ONCE_PER_PROCESS of tests/test_gpu_gemm_epilogues.py plus the names
    read_switches() reads on every call; each name is read in exactly one place, and that place is dm_gemm.hip."""
    from test_gpu_gemm_epilogues import ONCE_PER_PROCESS
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmerge_amd", "csrc")
    pattern = re.compile(r'getenv\(\s*"(DM_GEMM_\w+)"')
    read = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        if os.path.isfile(path):
            with open(path, errors="replace") as f:
                read[os.path.basename(path)] = pattern.findall(f.read())
    names = [n for found in read.values() for n in found]
    assert names and sorted(names) == sorted(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert {f for f, found in read.items() if found} == {"dm_gemm.hip"}
    with open(os.path.join(csrc, "dm_gemm.hip")) as f:
        src = f.read()
    body = src[src.index("GemmSwitches read_switches()"):]
    per_call = pattern.findall(body[:body.index("\n}\n")])
    assert "DM_GEMM_RING_WM" in per_call and "DM_GEMM_FORCE_TILE" in per_call
    assert len(set(ONCE_PER_PROCESS)) == len(ONCE_PER_PROCESS)
    assert set(names) == set(ONCE_PER_PROCESS) | set(per_call), set(names) ^ (set(ONCE_PER_PROCESS) | set(per_call))


# ---- the weight gradient (DM_TN): tests/test_gpu_gemm_wgrad.py -------------------------------------------------------------------------
def _wg_all_cases():
    """(family, case, plan) of every product the GPU module runs, the grouped products as cases of their own."""
    out = [(fam, c, G.wg_plan(fam, c)) for fam in G.WG_FAMILIES for c in G.wg_cases(fam)]
    for c in G.WG_GROUP["cases"]:
        gp = G.wg_group_plan(c)
        for M, N in G.WG_GROUP["shapes"]:
            out.append(("grouped", dict(c, name=f"{c['name']}@{M}x{N}", M=M, N=N), dict(split=gp["split"], kps=gp["kps"])))
    return out


def test_wgrad_slice_structure_of_every_shape():
    """The restated split rules give the slice structure the case table claims; printed per product (run with -s)."""
    got = {}
    for fam, c, plan in _wg_all_cases():
        sl = G.k_slices(c["K"] if fam in ("w4", "grouped") or not c["fold"] else 3 * c["K"], plan["split"], plan["kps"])
        got[(fam, c["name"])] = [b - a for a, b in sl]
        print(f"  [gemm_host] wgrad {fam:<8s} {c['name']:<24s} M={c['M']} N={c['N']} K={c['K']}{' x3' if c['fold'] else ''} slices={got[(fam, c['name'])]} "
              f"cs={plan.get('cs')} rows={plan.get('cs_rows')}")
    for fam, tile in (("t64", 64), ("t128", 128)):
        for name in ("split", "split_acc_cs", "split_csadd"):
            assert got[(fam, name)] == [576, 524] and 524 % 64 == 12                       # the last step has 12 rows
            assert got[("f32_" + fam, name)] == [288, 288, 288, 236] and 236 % 32 == 12     # bk = 32
        for name in ("short_acc", "short_acc_csadd"):
            assert got[(fam, name)] == [76] and got[("f32_" + fam, name)] == [44]
    assert got[("t64", "fold_acc_cs")] == [576, 576]                                        # K = 3 * 384: the slices straddle the segments
    # the proposal expected 4 x 576 for the pipeline; `eff > best + 0.04` takes 3 slices (gemm_ref.WG_FAMILIES["p256"])
    assert got[("p256", "split")] == got[("p256", "split_acc_cs")] == got[("p256", "split_csadd")] == [704, 704, 648] and 648 % 64 == 8
    assert got[("p256", "short_acc")] == [72] and got[("p256", "fold_acc_cs")] == [704, 704, 704]
    for tag in ("@256x192", "@512x384"):
        for name in ("split", "split_acc_cs", "split_csadd"):
            assert got[("w4", name + tag)] == [1024, 1024, 128]
        assert got[("w4", "short_acc" + tag)] == [1024]
    assert got[("w4", "fold_acc_cs")] == [512, 512, 64]                                     # positions of each piece: 34 steps of 32
    assert got[("generic", "split")] == [288] * 7 + [34]                                    # 8 z-slices; the last: 32 + 2 + 0 + 0 over the four waves
    assert got[("generic", "split_acc_cs")] == [2050] == got[("generic", "split_csadd")]    # `!a->colsum_a`: unsliced
    assert got[("generic", "short_acc")] == [19]
    for tag in ("@256x192", "@512x192"):
        assert got[("grouped", "sliced" + tag)] == got[("grouped", "sliced_acc" + tag)] == [1024, 1024, 128]
        assert got[("grouped", "one_slice" + tag)] == [1024] and got[("grouped", "fold_sliced" + tag)] == [512, 512, 64]
        assert got[("grouped", "fold_one_slice" + tag)] == [512]
    assert [G.wg_group_plan(c)["form"] for c in G.WG_GROUP["cases"]] == ["sliced", "sliced", "one_slice", "one_slice", "sliced", "one_slice"]
    # the rule itself would leave the group to the separate calls: the forms have to be forced
    assert all(G.plan_grouped(G.WG_GROUP["shapes"], c["K"], 32 if c["fold"] else 64, 1) is None for c in G.WG_GROUP["cases"])
    # column sums: fused rows per slice on t64 (1), the pipeline (4) and the 4-wave kernel (1); dm_colsum elsewhere (5 scratch rows for K = 1100,
    # none for one slice in the vector form, always some in the scalar form of the generic family)
    rows = {(fam, c["name"]): (p.get("cs"), p.get("cs_rows")) for fam, c, p in _wg_all_cases() if fam != "grouped" and c["cs"]}
    assert rows[("t64", "split_acc_cs")] == ("fused", 2) and rows[("p256", "split_acc_cs")] == ("fused", 12) and rows[("p256", "short_acc_csadd")] == ("fused", 4)
    assert rows[("w4", "split_csadd@512x384")] == ("fused", 3) and rows[("t128", "split_acc_cs")] == ("alone", 5) == rows[("f32_t64", "split_csadd")]
    assert rows[("t128", "short_acc_csadd")] == ("alone", 0) and rows[("generic", "split_acc_cs")] == ("alone", 9) and rows[("generic", "short_acc_csadd")] == ("alone", 1)
    # every family has what it can have: two tiles each way, the ragged last tile, the N tail, >= 2 slices with a shorter, partial last one
    for fam, f in G.WG_FAMILIES.items():
        for M, N, K, Ks in f["shapes"]:
            tm, tn = f["tile"] if isinstance(f["tile"], tuple) else (f["tile"], f["tile"])
            sl = got[(fam, "split" + ("" if len(f["shapes"]) == 1 else f"@{M}x{N}"))]
            assert len(sl) >= 2 and sl[-1] < sl[0] and K <= 2304, fam
            if fam == "w4":
                assert M % tm == 0 and N % tn == 0 and K % 128 == 0 and sl[-1] % 128 == 0 and (M // tm) * (N // tn) in (1, 4)
                continue
            assert (M + tm - 1) // tm >= 2 and (N + tn - 1) // tn >= 2 and M % tm != 0 and N % tn != 0, fam
            assert sl[-1] % f["bk"] != 0 and Ks % f["bk"] != 0 and Ks < 8 * f["bk"], fam          # a partial last K step; the short case cannot split
            if fam != "generic":
                wm = tm // 2 if f["kind"] == "tile" else 128
                blocks = range((M // tm) * tm, (M // tm) * tm + tm, wm)
                assert any(b >= M for b in blocks) and any(b < M < b + wm for b in blocks) and M % 16 != 0, fam
                assert M % 8 == 0 and N % 8 == 0
            else:
                assert M % 4 != 0                                                           # gemm_prepare: off the MFMA path


def test_wgrad_data_is_exact_in_any_order_and_needs_more_than_8_bits():
    bf = lambda x: torch.from_numpy(np.array(x)).float().bfloat16().double().numpy()
    seen = set()
    for fam, c, plan in _wg_all_cases():
        M, N, K, fold = c["M"], c["N"], c["K"], c["fold"]
        d = G.wg_data(M, N, K, fold)
        # the proof: products on a grid, the sum of their magnitudes below 2^24 grid steps
        if fold:
            assert 4.02 * K * 1024 < 2 ** 24
            parts = [("dy_hi", "x_hi"), ("dy_hi", "x_lo"), ("dy_lo", "x_hi")]
            for k in ("dy_hi", "dy_lo", "x_hi", "x_lo"):
                assert np.array_equal(bf(d[k]), d[k]) and np.array_equal(np.round(d[k] * 1024) / 1024, d[k])
            assert np.abs(d["dy_hi"]).max() == 2 and np.abs(d["dy_lo"]).max() == 3 / 1024
        else:
            assert K <= 2304 and 4 * K * 64 < 2 ** 24
            parts = [("dy", "x")]
            assert np.array_equal(bf(d["dy"]), d["dy"]) and np.array_equal(bf(d["x"]), d["x"])
            assert np.array_equal(np.round(d["dy"]), d["dy"]) and np.abs(d["dy"]).max() == 2
            assert np.array_equal(np.round(d["x"] * 64) / 64, d["x"]) and np.abs(d["x"]).max() == 2
        for k in ("old_c", "old_db"):
            assert np.array_equal(np.round(d[k] * 64) / 64, d[k]) and np.abs(d[k]).max() <= 2
        dw, db = G.wg_ref(d, c["acc"], c["cs"], fold)
        assert np.array_equal(dw.astype(np.float32).astype(np.float64), dw) and np.array_equal(db.astype(np.float32).astype(np.float64), db)
        # some output, and some element of every slice's partial tile, needs more than 8 significand bits: a slab kept in bf16 would be seen
        assert (bf(dw) != dw).any(), (fam, c["name"])
        for k0, k1 in G.k_slices(K, plan["split"], plan["kps"]) if not (fold and fam in ("t64", "p256")) else [(0, K)]:
            part = G.wg_ref(d, False, None, fold, k0, k1)[0]
            assert (bf(part) != part).any(), (fam, c["name"], k0, k1)
        # the demonstration, once per data set: float32 sums over a block of outputs that holds the first and the last rows and columns, in
        # adversarial orders -- k ascending, descending, all negative products first (the largest intermediate magnitude), all positive first,
        # pairwise (numpy), and slice by slice with the partials added last
        if (M, N, K, fold) in seen:
            continue
        seen.add((M, N, K, fold))
        mi = np.r_[0:8, M - 8:M]
        ni = np.r_[0:8, N - 8:N]
        prod = np.concatenate([d[a][:, mi, None] * d[b][:, None, ni] for a, b in parts]).astype(np.float32)      # [K or 3K, 16, 16]
        assert np.array_equal(prod.astype(np.float64), np.concatenate([d[a][:, mi, None] * d[b][:, None, ni] for a, b in parts]))
        want = G.wg_ref(d, False, None, fold)[0][np.ix_(mi, ni)]
        seq = lambda p: np.cumsum(p, axis=0, dtype=np.float32)[-1]
        srt = np.sort(prod, axis=0)
        orders = {"ascending k": seq(prod), "descending k": seq(prod[::-1]), "negatives first": seq(srt), "positives first": seq(srt[::-1]),
                  "pairwise": prod.sum(axis=0, dtype=np.float32)}
        step = max(1, prod.shape[0] // 7)
        orders["slices"] = seq(np.stack([seq(prod[i:i + step]) for i in range(0, prod.shape[0], step)]))
        for name, v in orders.items():
            assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), want), (fam, c["name"], name)
        assert np.abs(np.cumsum(srt, axis=0, dtype=np.float32)).max() > np.abs(want).max()      # the sorted order does reach further out than the result


def test_wgrad_frames_are_guarded():
    """16-byte but not 256-byte aligned views, padded leading dimensions, a whole k_per_split of rows below K, sentinel around C and db."""
    for fam, c, plan in _wg_all_cases():
        M, N, K, fold = c["M"], c["N"], c["K"], c["fold"]
        esz = 4 if (G.WG_GROUP if fam == "grouped" else G.WG_FAMILIES[fam])["ab"] == G.F32 else 2
        fr = G.wg_frames(M, N, K, plan["kps"], fold)
        for nm, cols in (("dy", M), ("x", N)):
            o = fr[nm]
            assert o["idx"].min() == G.VIEW_OFFSET and (G.VIEW_OFFSET * esz) % 16 == 0 and (G.VIEW_OFFSET * esz) % 256 != 0
            assert len(np.unique(o["idx"])) == o["idx"].size == (2 if fold else 1) * K * cols
            # a slice that starts anywhere below K and runs for a whole k_per_split stays inside the allocation, all its columns included
            assert o["elems"] - 1 - int(o["idx"].max()) >= plan["kps"] * o["ld"] - (o["ld"] - cols), (fam, c["name"], nm)
            if fold:
                assert o["ld"] == cols and o["plane"] == K * cols and np.array_equal(o["idx"][1] - o["idx"][0], np.full((K, cols), K * cols))
            else:
                assert o["ld"] - cols >= 8 and (fam == "generic" or ((o["ld"] * esz) % 16 == 0 and o["ld"] % 8 == 0))      # (generic: M % 4 != 0, any alignment)
                assert o["idx"].shape == (K, cols) and o["idx"][1, 0] - o["idx"][0, 0] == o["ld"]
        assert fr["dy"]["ld"] != fr["x"]["ld"] or fold
        o = fr["c"]
        assert o["ld"] == N + 8 and o["idx"].shape == (M, N) and o["idx"].min() == G.VIEW_OFFSET and len(np.unique(o["idx"])) == M * N
        assert o["elems"] - 1 - int(o["idx"].max()) >= G.PAD_ROWS * o["ld"]
        assert fr["db"]["idx"].shape == (M,) and fr["db"]["elems"] - 1 - int(fr["db"]["idx"].max()) >= 64
        # the workspace: the planned writes lie inside the declared bytes, slab and column-sum rows apart
        if fam != "grouped":
            writes = sorted(plan["writes"])
            assert all(a + n <= plan["ws_bytes"] // 4 for a, n in writes) and all(a + n <= b for (a, n), (b, _) in zip(writes, writes[1:]))
            assert plan["ws_bytes"] == G.tn_workspace_bytes(M, N, 3 * K if fold else K, int(G.WG_FAMILIES[fam]["env"].get("DM_GEMM_FORCE_TILE") or 0))
    for c in G.WG_GROUP["cases"]:
        for p in G.wg_group_plan(c)["products"]:
            writes = sorted(p["writes"])
            assert all(a + n <= p["ws_bytes"] // 4 for a, n in writes) and all(a + n <= b for (a, n), (b, _) in zip(writes, writes[1:]))


def test_wgrad_switches_are_read_by_the_library():
    """Every switch a weight-gradient family sets is a name read_switches reads on every call."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmerge_amd", "csrc", "dm_gemm.hip")) as f:
        src = f.read()
    body = src[src.index("GemmSwitches read_switches()"):]
    per_call = set(re.findall(r'getenv\(\s*"(DM_GEMM_\w+)"', body[:body.index("\n}\n")]))
    for f in list(G.WG_FAMILIES.values()) + [G.WG_GROUP]:
        assert set(f["env"]) <= per_call, set(f["env"]) - per_call
    assert "DM_GEMM_GROUPED" in per_call
    assert set(G.WG_ALL) == {"t64", "t128", "f32_t64", "f32_t128", "p256", "w4", "generic", "grouped"}


def test_framed_operand_cases_of_the_epilogue_families():
    for fam, f in G.FAMILIES.items():
        assert G.family_framed_cases(fam) == [(lay, G.FRAMED_AB) for lay in f["layouts"]] and "none_f32" in G.family_configs(fam)
    elems, ld, idx = G.framed_operand(328, 192)
    assert ld == 200 and idx.shape == (328, 192) and idx.min() == G.VIEW_OFFSET and idx[1, 0] - idx[0, 0] == ld
    assert elems - 1 - int(idx.max()) >= G.OPERAND_PAD_ROWS * ld and len(np.unique(idx)) == idx.size


# ---- the main loop (NT / NN): tests/test_gpu_gemm_mainloop.py ----------------------------------------------------------------------------
def _ml_datasets():
    """(family, M, N, K or k_fold, fold, K step) of every product's data, each (shape, fold, step) once."""
    seen, out = set(), []
    for fam, f in G.FAMILIES.items():
        M, N, _ = f["shape"]
        for c in G.ml_cases(fam):
            fold = c["kind"] == "fold"
            bk = 32 if (fold and fam == "w4") else f["bk"]          # the 4-wave kernel's FOLD instances step through 32 positions
            key = (M, N, c["K"], fold, bk)
            if key not in seen:
                seen.add(key)
                out.append((fam,) + key)
    return out


def _tiles(K, bk):
    return [(k0, min(K, k0 + bk)) for k0 in range(0, K, bk)]


def test_mainloop_case_table():
    assert set(G.ML_K) == set(G.FAMILIES) and set(G.ML_FOLD) | set(G.ML_FOLD_REFUSED) == set(G.FAMILIES) and not set(G.ML_FOLD) & set(G.ML_FOLD_REFUSED)
    assert set(G.ML_FOLD) == {"t64", "t128", "ring8", "ring4", "p256", "w4", "kslices"}
    for fam, f in G.FAMILIES.items():
        steps = [(K + f["bk"] - 1) // f["bk"] for K in G.ML_K[fam]]
        if fam in G.ML_DEPTH:                                       # one step (w4: two) up to the pipeline's depth + 2, every count between
            assert min(steps) == (2 if fam == "w4" else 1) and max(steps) >= G.ML_DEPTH[fam] + 2, fam
            assert set(range(min(steps), G.ML_DEPTH[fam] + 3, 2 if fam == "w4" else 1)) <= set(steps), fam
        names = G.ml_configs(fam, False)
        assert names == (("none_f32", "bias_res_f32") if fam == "generic" else ("none_f32", "none_bf16", "bias_res_f32")), fam
        if fam in G.ML_FOLD:
            assert G.ml_configs(fam, True) == ("none_f32", "none_bf16", "bias_res_f32", "pair_none") and f["ab"] == G.BF16
        n_plain = len(G.ML_K[fam]) * len(f["layouts"]) * len(names)
        n_fold = len(G.ML_FOLD.get(fam, ())) * len(f["layouts"]) * 4 * 2
        assert len(G.ml_cases(fam)) == n_plain + n_fold, fam
    for fam in ("t64", "t128"):                                     # touch_at = max(0, nk - 4): nk on both sides of 4; tails alone, after one and two stages
        nk = sorted({(K + 63) // 64 for K in G.ML_K[fam]})
        assert nk == [1, 2, 3, 4, 5] and {K % 64 for K in G.ML_K[fam]} == {0, 8} and {8, 72, 136} <= set(G.ML_K[fam])
        assert G.CONFIG["bias_res_f32"]["res"]                      # ... and a configuration whose residual arms the touch
    assert G.lean_key(G.PAIR_NONE) == 1 << 8 and G.PAIR_NONE["name"] not in G.CONFIG and G.is_exact(G.PAIR_NONE) == (True, False)
    assert not [p for p in G.STRIP_ZERO_SIGN if p[1] in G.ML_CONFIG]          # every comparison of the main-loop tests is strict


def test_mainloop_plans_restated():
    """Which family takes which K and k_fold, each rule restated from its plan; the K slices through plan_fwd_split and k_slices."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmerge_amd", "csrc")
    assert G.ML_K_SKIPS == {}
    for fam, f in G.FAMILIES.items():
        M, N, _ = f["shape"]
        for K in list(G.ML_K[fam]) + [3 * kf for kf in G.ML_FOLD.get(fam, ())]:
            epc = 8 if f["ab"] == G.BF16 else 4
            if fam == "generic":
                assert K % 4 != 0                                   # gemm_prepare: `(a_inner % epc == 0)` fails -> gemm_generic
                continue
            assert K % epc == 0 and (K + 8) % epc == 0, (fam, K)    # mfma_ok with the framed leading dimension K + 8
            if f["ab"] == G.F32:
                assert ((M + 127) // 128) * ((N + 127) // 128) >= 16
            if fam in ("ring8", "ring4", "q4", "t96"):              # `if (p.K % BK != 0 || p.N % 8 != 0 ...) return`
                assert K % 64 == 0 and N % 8 == 0
            if fam in ("q4", "t96"):
                assert M % 64 == 0
            if fam == "p256":                                       # `if (p.K < BK256) return false`, `if ((!am || !bm) && p.K % BK256 != 0) return false`
                assert K >= 64 and K % 64 == 0 and N % 8 == 0
            if fam == "w4":                                         # `if (k_eff < 2 * bk_eff || k_eff % (2 * bk_eff) != 0 || p.N % TN != 0) return 0`
                assert N % 192 == 0 and (K % 128 == 0 and K >= 128 if K in G.ML_K[fam] else (K // 3) % 64 == 0 and K // 3 >= 64)
            if fam == "kslices":
                assert G.plan_fwd_split(M, N, K)[1] == 64
            else:
                assert G.plan_fwd_split(M, N, K) == (1, 0), (fam, K)
    width = lambda sl: [b - a for a, b in sl]
    assert width(G.ml_slices("kslices", 1536)) == [768, 768] and width(G.ml_slices("kslices", 1600)) == [832, 768]
    assert width(G.ml_slices("kslices", 2048)) == [512] * 4 and G.ml_slices("t64", 320) == [(0, 320)]
    # plane pairs: k_fold = 512 -> the seam at 512 inside slice 0 (and the one at 1024 inside slice 1); 576 -> one seam in each slice
    assert G.ML_FOLD["kslices"] == (512, 576)
    s = G.ml_slices("kslices", 3 * 512)
    assert s == [(0, 768), (768, 1536)] and s[0][0] < 512 < s[0][1] and s[1][0] < 1024 < s[1][1]
    s = G.ml_slices("kslices", 3 * 576)
    assert s == [(0, 896), (896, 1728)] and s[0][0] < 576 < s[0][1] and s[1][0] < 1152 < s[1][1]
    M, N, _ = G.FAMILIES["kslices"]["shape"]
    assert all(4 * M * N * 4 >= len(G.ml_slices("kslices", K)) * M * N * 4 for K in (1536, 1600, 1728, 2048))      # dm_gemm_workspace_bytes: four slices of room
    for fam, kfs in G.ML_FOLD.items():                              # k_fold_fault: `a.k_fold % 64 == 0`; one, two, three K tiles per segment
        assert all(kf % 64 == 0 for kf in kfs) and (fam == "kslices" or [kf // 64 for kf in kfs] == [1, 2, 3])
    # every refusal quotes a line that stands in the named file
    quotes = [v[1] for v in G.ML_FOLD_REFUSED.values()] + [G._T96_EPI, G._T96_KEY]
    for why in quotes:
        name, line = why.split(" ", 1)[0], why[why.index("`") + 1:why.rindex("`")]
        with open(os.path.join(csrc, name)) as fh:
            assert line in fh.read(), why
    assert {v[0] for v in G.ML_FOLD_REFUSED.values()} == {"plan", "dm_gemm"} and G.ML_REFUSED_K_FOLD % 64 == 0
    # the walk: eleven row tiles, the last ragged and alone in a band of three; three column tiles, the last eight wide
    assert G.GROUP_M == 8 and set(G.ML_WALK) == set(G.FAMILIES) - {"w4"}
    for fam, (M, N, K) in G.ML_WALK.items():
        tm, tn = G.FAMILIES[fam]["tile"]
        assert (M + tm - 1) // tm == G.GROUP_M + 3 and M % tm != 0 and N % tn == 8, fam
        assert (N + tn - 1) // tn == (5 if fam == "f32_t64" else 3), fam
        assert K == {"kslices": 1536, "generic": 19}.get(fam, G.FAMILIES[fam]["bk"])
        if G.FAMILIES[fam]["ab"] == G.F32 and fam != "generic":
            assert ((M + 127) // 128) * ((N + 127) // 128) >= 16
        assert (G.plan_fwd_split(M, N, K) == (2, 64)) == (fam == "kslices")
        assert fam not in ("q4", "t96") or M % 64 == 0
    M, N = G.ml_walk_w4(256)
    assert (M, N) == (98504, 192) and (M + 255) // 256 == 385 and M % 256 == 200 and all(K % 128 == 0 for K in G.ML_WALK_W4_K)


def test_mainloop_data_is_exact_in_every_order():
    """What the bit comparison rests on: every prefix sum of the contraction in float32 is the float64 value -- in natural order, reversed, tile
    by tile and (pairs) segment by segment, slice by slice with the partial sums added last -- and so is every step of the epilogue."""
    bf = lambda x: torch.from_numpy(np.array(x)).float().bfloat16().double().numpy()
    for fam, M, N, K, fold, bk in _ml_datasets():
        d = G.ml_data(M, N, K, fold)
        terms = G.ml_terms(d, fold)
        for a, b in terms:
            assert np.array_equal(bf(a), a) and np.array_equal(bf(b), b)                    # exact in bf16 (and so in fp32)
        if fold:
            assert 4.02 * K * 1024 < 2 ** 24 and np.abs(d["a_hi"]).max() == 2 and np.abs(d["b_lo"]).max() == 3 / 1024
            assert not np.array_equal(d["a_lo"] * (d["a_hi"] != 0), d["b_lo"][:M] * (d["a_hi"] != 0)) if N >= M else True
            lolo = d["a_lo"] @ d["b_lo"].T
            assert np.array_equal(np.round(lolo * 2 ** 20), lolo * 2 ** 20) and (np.round(lolo * 1024) != lolo * 1024).mean() > 0.5      # off the 2^-10 grid
            with_lolo = (d["acc"] + lolo).astype(np.float32).astype(np.float64)
            assert (with_lolo != d["acc"]).mean() > 0.5                                     # a kernel that computes Al Bl cannot match
        mi, ni = np.r_[0:8, M - 8:M], np.r_[0:8, N - 8:N]
        prod64 = np.concatenate([(a[mi][:, None, :] * b[ni][None, :, :]).transpose(2, 0, 1) for a, b in terms])      # [K or 3 K, 16, 16]
        prod = prod64.astype(np.float32)
        assert np.array_equal(prod.astype(np.float64), prod64)
        want = d["acc"][np.ix_(mi, ni)]
        pre = lambda p: np.cumsum(p, axis=0, dtype=np.float32)
        for name, p in (("natural", prod), ("reversed", prod[::-1])):
            c32, c64 = pre(p), np.cumsum(p.astype(np.float64), axis=0)
            assert c32.dtype == np.float32 and np.array_equal(c32.astype(np.float64), c64) and np.array_equal(c64[-1], want), (fam, K, fold, name)
        # tile by tile (the K step), segment by segment, slice by slice: the partial sums, then their running sum
        k_all = prod.shape[0]
        cuts = {"tiles": _tiles(k_all, bk), "slices": G.ml_slices(fam, k_all)}
        if fold:
            cuts["segments"] = _tiles(k_all, K)
        for name, cut in cuts.items():
            parts = np.stack([pre(prod[k0:k1])[-1] for k0, k1 in cut])
            assert np.array_equal(parts.astype(np.float64), np.stack([prod64[k0:k1].sum(0) for k0, k1 in cut])), (fam, K, fold, name)
            assert np.array_equal(pre(parts)[-1].astype(np.float64), want) and np.array_equal(pre(parts[::-1])[-1].astype(np.float64), want)
        # the epilogue of every configuration: exact in float32 in both orders, with and without fma; a pair's lo plane is an exact difference
        assert np.array_equal(d["acc"].astype(np.float32).astype(np.float64), d["acc"])
        for name in G.ml_configs(fam, fold):
            cfg = G.ML_CONFIG[name]
            c = G.ml_case(cfg, d)
            ref = G.epilogue_ref(d["acc"], c)
            for order in ("left", "right"):
                for fma in (False, True):
                    assert np.array_equal(G.restate32(d["acc"], c, True, order, fma)["v"].astype(np.float64), ref["v"]), (fam, K, name)
            if cfg["c"] == G.PAIR:
                hi = G.round_bf16(ref["v"])
                assert np.array_equal((ref["v"].astype(np.float32) - hi.astype(np.float32)).astype(np.float64), ref["v"] - hi)
                assert (ref["c_lo"] != 0).mean() > 0.5                                      # the lo plane carries information
            if cfg["c"] == G.BF16 and fold:
                assert (bf(ref["v"]) != ref["v"]).mean() > 0.5                              # the rounding to bf16 is a real one


def _every_block_differs(got, want):
    """Does `got` differ from `want` somewhere in every 16 x 16 block of the window (partial blocks at the edges included)?"""
    diff = (got != want) | (np.signbit(got) != np.signbit(want))
    rows = np.add.reduceat(diff.astype(np.int64), np.arange(0, diff.shape[0], 16), axis=0)
    return bool((np.add.reduceat(rows, np.arange(0, diff.shape[1], 16), axis=1) > 0).all())


def test_mainloop_net_is_tight():
    """Without a GPU: the accumulator restated under the faults a K loop can have differs from the spec, in bits, in EVERY 16 x 16 block of
    the M x N window -- as fp32 and after the rounding to bf16 (none_bf16).  So the bit comparison of the GPU test sees each of them in
    whatever tile it happens."""
    r32 = lambda x: x.astype(np.float32).astype(np.float64)
    n_faults = 0
    for fam, M, N, K, fold, bk in _ml_datasets():
        d = G.ml_data(M, N, K, fold)
        terms = G.ml_terms(d, fold)
        acc = d["acc"]
        faults = {}
        T = lambda s, k0, k1: terms[s][0][:, k0:k1] @ terms[s][1][:, k0:k1].T
        for s in range(len(terms)):
            tl = _tiles(K, bk)
            for t, (k0, k1) in enumerate(tl):
                faults[f"segment {s} tile {t} dropped"] = acc - T(s, k0, k1)
                if t + 1 < len(tl):                                 # the stale buffer: tile t once more where tile t + 1 belongs (both operands, and A alone)
                    n0, n1 = tl[t + 1]
                    w = n1 - n0
                    faults[f"segment {s} tile {t} twice"] = acc - T(s, n0, n1) + T(s, k0, k0 + w)
                    faults[f"segment {s} tile {t} of A twice"] = acc - T(s, n0, n1) + terms[s][0][:, k0:k0 + w] @ terms[s][1][:, n0:n1].T
        if fold:
            ah, al, bh, bl = d["a_hi"], d["a_lo"], d["b_hi"], d["b_lo"]
            faults["segment 2 of A read from hi"] = acc - al @ bh.T + ah @ bh.T
            faults["segment 1 of B read from hi"] = acc - ah @ bl.T + ah @ bh.T
            faults["segment 2 computed as lo lo"] = acc - al @ bh.T + al @ bl.T
            w = min(bk, K)
            for s in range(3):                                      # a seam one tile off: the segment's first tile comes from a neighbour
                for o in (s - 1, s + 1):
                    if 0 <= o < 3:
                        faults[f"segment {s}: first tile from segment {o}"] = acc - T(s, 0, w) + T(o, 0, w)
        elif K % bk:
            w = min(8, K % bk)                                      # the K tail's last 8 columns (fp32 operands: the tail is 4 wide)
            a, b = terms[0]
            faults["K tail dropped"] = acc - a[:, K - w:] @ b[:, K - w:].T
            nxt = np.roll(a, -1, axis=0)[:, :w]                      # ... read as the next row's first columns
            faults["K tail of A from the next row"] = acc - a[:, K - w:] @ b[:, K - w:].T + nxt @ b[:, K - w:].T
            nxt = np.roll(b, -1, axis=0)[:, :w]
            faults["K tail of B from the next row"] = acc - a[:, K - w:] @ b[:, K - w:].T + a[:, K - w:] @ nxt.T
        want32, want16 = r32(acc), G.round_bf16(np.array(acc))
        for name, v in faults.items():
            n_faults += 1
            assert _every_block_differs(r32(v), want32), (fam, K, fold, name, "fp32")
            if fam != "generic":
                assert _every_block_differs(G.round_bf16(v), want16), (fam, K, fold, name, "bf16")
    assert n_faults > 500


def test_mainloop_frames():
    """No element of an allocation belongs to two windows; "far" planes do not overlap and have NaN between them; strides the kernels accept."""
    for fam, M, N, K, fold, bk in _ml_datasets():
        if not fold:
            for rows, cols in ((M, K), (N, K), (K, N)):
                elems, ld, idx = G.framed_operand(rows, cols)
                assert ld == cols + 8 and len(np.unique(idx)) == idx.size and idx.min() == G.VIEW_OFFSET
                assert elems - 1 - int(idx.max()) >= G.OPERAND_PAD_ROWS * ld
            continue
        for rows, cols in ((M, K), (N, K), (K, N)):
            dense, far = G.pair_frame(rows, cols, "dense"), G.pair_frame(rows, cols, "far")
            for fr in (dense, far):
                idx = fr["idx"]
                assert idx.shape == (2, rows, cols) and len(np.unique(idx)) == idx.size and idx.min() == G.VIEW_OFFSET       # no index in two planes
                assert np.array_equal(idx[1] - idx[0], np.full((rows, cols), fr["plane"])) and fr["ld"] == cols
                assert fr["plane"] % 8 == 0 and 0 < fr["plane"] < 1 << 30                                                      # k_fold_fault: offsets % 8, below 2^30
                assert fr["elems"] - 1 - int(idx.max()) >= G.OPERAND_PAD_ROWS * cols and (G.VIEW_OFFSET * 2) % 16 == 0
            assert dense["plane"] == rows * cols and far["plane"] == rows * cols + 8 * 37 == rows * cols + G.FAR_GAP
            assert int(far["idx"][1].min()) - int(far["idx"][0].max()) - 1 == G.FAR_GAP                                        # NaN from plane to plane
    for name, cfg in G.ML_CONFIG.items():
        b = G.buffers(cfg, 328, 200)
        assert b["c"]["elems"] - 1 - int(b["c"]["idx"].max()) - b["c"].get("plane", 0) >= G.PAD_ROWS * b["c"]["ld"]
        assert (name == "pair_none") == ("plane" in b["c"]) and ("res" in b) == cfg["res"]


def test_mainloop_switches():
    """The main-loop module clears the same once-per-process switches as the epilogue module and sets only names read on every call."""
    import test_gpu_gemm_mainloop as ML
    import test_gpu_gemm_epilogues as EP
    assert ML.ONCE_PER_PROCESS is EP.ONCE_PER_PROCESS and ML.TIMEOUT == EP.TIMEOUT == 60
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmerge_amd", "csrc", "dm_gemm.hip")) as f:
        src = f.read()
    body = src[src.index("GemmSwitches read_switches()"):]
    per_call = set(re.findall(r'getenv\(\s*"(DM_GEMM_\w+)"', body[:body.index("\n}\n")]))
    for fam, f in G.FAMILIES.items():
        assert set(f["env"]) <= per_call and "DM_GEMM_T96" in f["env"], fam
