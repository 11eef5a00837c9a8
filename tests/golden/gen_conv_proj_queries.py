"""Records the five host queries of the mixer middle into conv_proj_queries.json.

    python tests/golden/gen_conv_proj_queries.py <commit> [path/to/libvideomamba_hip.so]

Run against the library built at the commit the table is to name (no device needed: the
queries are pure host arithmetic).  tests/test_api_cpu.py replays every row.  A row gives
the shape; the strides the queries take are the mixer's own: xz rows of 2 * dim, batches of
out_len rows, a conv state of (batch, dim, width), u rows of dim.
"""

import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
COLUMNS = ["batch", "out_len", "seqlen", "dim", "e", "e_pad", "r_pad", "k", "cs_dtype",
           "dt_softplus", "has_dt", "width",
           "fits", "workspace_bytes", "in_proj_fits", "in_proj_workspace_bytes",
           "cm_workspace_bytes"]

LL, I = ctypes.c_longlong, ctypes.c_int


def bind(path):
    lib = ctypes.CDLL(path)
    lib.vm_conv_proj_fits.argtypes = [I] * 7 + [LL, LL, I, I, LL, LL, I, LL]
    lib.vm_in_proj_conv_proj_fits.argtypes = [I] * 9
    for name in ("vm_conv_proj_workspace_bytes", "vm_in_proj_conv_proj_workspace_bytes",
                 "vm_conv_proj_cm_workspace_bytes"):
        getattr(lib, name).argtypes = [I] * 4
        getattr(lib, name).restype = LL
    return lib


def answers(lib, shape):
    """The five answers for one row's shape columns (cs_dtype -1: no conv state in)."""
    b, lp, l, d, e, ep, rp, k, cs, spd, has_dt, w = shape
    return [lib.vm_conv_proj_fits(b, lp, l, d, e, rp, spd, lp * 2 * d, 2 * d, int(cs >= 0),
                                  max(cs, 0), d * w, w, w, d),
            lib.vm_conv_proj_workspace_bytes(b, lp, d, e),
            lib.vm_in_proj_conv_proj_fits(k, b, lp, d, e, ep, rp, w, has_dt),
            lib.vm_in_proj_conv_proj_workspace_bytes(b, lp, d, e),
            lib.vm_conv_proj_cm_workspace_bytes(b, lp, d, e)]


AXES = [
    ("batch", [1, 8, 9, 0]),
    ("out_len", [3144, 7, 8, 23, 24, 55, 56, 300_000]),
    ("dim", [1152, 64, 192, 1280, 2048, 2112, 100]),
    ("e_epad", [(68, 80), (76, 80), (78, 80), (84, 96), (100, 128)]),  # round_up(e, 4) 76 | 80
    ("r_pad", [64, 0, 32, 96]),
    ("k", [576, 192, 1536, 1024, 200, 0]),
    ("cs_dtype", [-1, 0, 1]),
    ("dt_softplus", [0, 1]),
]


def shapes():
    """Every pair of axes in full around the first value of the others (so each limit is
    crossed with every value of every other axis), once with dt and width 4 and, for the
    in_proj query, a few rows without dt / with other widths."""
    seen, out = set(), []

    def add(vals, has_dt=1, width=4):
        b, lp, d, (e, ep), rp, k, cs, spd = vals
        row = (b, lp, lp if lp < 100_000 else lp - 7, d, e, ep, rp, k, cs, spd, has_dt, width)
        if row not in seen:
            seen.add(row)
            out.append(row)

    base = [vals[0] for _, vals in AXES]
    for i, j in itertools.combinations(range(len(AXES)), 2):
        for vi in AXES[i][1]:
            for vj in AXES[j][1]:
                v = list(base)
                v[i], v[j] = vi, vj
                add(v)
    for rp in (64, 96):
        for width in (4, 2, 5, 0):
            v = list(base)
            v[4] = rp
            add(v, has_dt=0, width=width)
    return out


def main():
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        HERE, "..", "..", "videomamba_amd", "libvideomamba_hip.so")
    lib = bind(path)
    rows = [list(s) + answers(lib, s) for s in shapes()]
    with open(os.path.join(HERE, "conv_proj_queries.json"), "w") as f:
        f.write("{\n")
        f.write(f' "commit": {json.dumps(commit)},\n')
        f.write(' "note": "vm_conv_proj_fits, vm_conv_proj_workspace_bytes, '
                'vm_in_proj_conv_proj_fits, vm_in_proj_conv_proj_workspace_bytes and '
                'vm_conv_proj_cm_workspace_bytes of the library built at `commit` '
                '(gen_conv_proj_queries.py; cs_dtype -1 = no conv state in)",\n')
        f.write(f' "columns": {json.dumps(COLUMNS)},\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]\n}\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
