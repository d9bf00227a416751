"""The attention routing queries of a kernel library, as a table (host logic: needs no GPU).

    python tools/attn_plan_queries.py table LIB          one row per call, under the current environment
    python tools/attn_plan_queries.py digest LIB [LIB2]  one line per environment of ENVS: rows and the SHA-256 of each library's table

A row is `B N H D dtype cube : dm_attention_relpos_inkernel dm_attention_bwd_batch_chunks dm_attention_split_ok
dm_attention_split_bwd_chunks`.  The DM_ATTN_* switches are read once per process, so `digest` runs every environment in a
child process of its own.  profiles/attn_plan_queries.txt is `digest <parent commit's library> <this tree's library>`.
"""
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys

BS, NS, HS, DS = (1, 2, 3, 8, 64, 256), (64, 128, 129, 160, 192, 193, 197, 224, 256, 257), (1, 12, 16), (64, 80)
DTYPES = (("bf16", 1), ("fp32", 0))
CUBES = (None, (3, 8, 8), (4, 8, 8), (4, 4, 16))
ENVS = [{}] + [{k: v} for k in ("DM_ATTN_PIPE", "DM_ATTN_Q32", "DM_ATTN_Q32_BWD") for v in ("0", "2")] + [
    {"DM_ATTN_Q32_BWD": "3"}, {"DM_ATTN_Q32_TABKV": "0"}, {"DM_ATTN_X3": "0"},
    {"DM_ATTN_PIPE": "2", "DM_ATTN_Q32": "2", "DM_ATTN_Q32_BWD": "2"}]


def env_name(env):
    return ",".join(f"{k}={v}" for k, v in env.items()) or "none"


def row(lib, B, N, H, D, dtype, cube):
    """The four answers for one call; cube None: the queries that take a cube get (0, 0, 0) and `no table`."""
    s, h, w = cube or (0, 0, 0)
    return (lib.dm_attention_relpos_inkernel(B, N, H, D, s, h, w, dtype), lib.dm_attention_bwd_batch_chunks(B, N, H, dtype),
            lib.dm_attention_split_ok(B, N, H, D, int(cube is not None), s, h, w), lib.dm_attention_split_bwd_chunks(B, N, H))


def table(path):
    lib = C.CDLL(os.path.abspath(path))
    out = []
    for B, N, H, D, (dn, dt), cube in itertools.product(BS, NS, HS, DS, DTYPES, CUBES):
        cn = "none" if cube is None else "x".join(map(str, cube))
        out.append(f"{B} {N} {H} {D} {dn} {cn} : " + " ".join(map(str, row(lib, B, N, H, D, dt, cube))))
    return out


def main():
    mode, libs = sys.argv[1], sys.argv[2:]
    if mode == "table":
        print("\n".join(table(libs[0])))
        return
    for env in ENVS:
        clean = {k: v for k, v in os.environ.items() if not k.startswith("DM_ATTN_")}
        cols = []
        for path in libs:
            text = subprocess.run([sys.executable, os.path.abspath(__file__), "table", path], env={**clean, **env}, capture_output=True,
                                  text=True, check=True).stdout
            cols.append(f"{text.count(chr(10))} rows sha256 {hashlib.sha256(text.encode()).hexdigest()}")
        same = "" if len(cols) < 2 else ("  equal" if len(set(cols)) == 1 else "  DIFFERENT")
        print(f"{env_name(env):58s} " + "  |  ".join(cols) + same)


if __name__ == "__main__":
    main()
