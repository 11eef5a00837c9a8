"""Records how the projection GEMM's entries answer calls that cannot launch, into
gemm_refusals.json.

    python tests/golden/gen_gemm_refusals.py <commit> [path/to/libvideomamba_hip.so]

Run against the library built at the commit the table is to name.  No device is needed and
none is touched: every call has m == 0 (or m == -1, refused by the shape block), so it
returns before any launch, and the pointers are made-up addresses that are never
dereferenced.  tests/test_api_cpu.py replays every row.  A pointer column holds the offset
added to a made-up 16-byte aligned address, or -1 for NULL.
"""

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LL, I, P = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p

LINEAR_COLUMNS = ["x", "ldx", "w", "ldw", "bias", "out", "ldo", "m", "n", "k", "dtype", "form"]
ADD_NORM_COLUMNS = ["x", "ldx", "w", "ldw", "h", "ldo", "residual", "ldr", "norm_weight", "hn",
                    "ldh", "m", "n", "k", "counters", "counter_bytes"]
POINTERS = {"x", "w", "bias", "out", "h", "residual", "norm_weight", "hn", "counters"}


def bind(path):
    lib = ctypes.CDLL(path)
    lib.vm_last_error.restype = ctypes.c_char_p
    lib.vm_linear_fwd_form.argtypes = [P, LL, P, LL, P, P, LL, I, I, I, I, I, P]
    lib.vm_linear_add_norm_fwd.argtypes = [P, LL, P, LL, P, LL, P, LL, P, ctypes.c_float, P, LL,
                                           I, I, I, P, LL, P]
    lib.vm_linear_add_norm_counter_bytes.argtypes = [I]
    lib.vm_linear_add_norm_counter_bytes.restype = LL
    return lib


def pointer(slot, off):
    return None if off < 0 else ctypes.c_void_p(((slot + 1) << 20) + off)


def call_linear(lib, row):
    a = dict(zip(LINEAR_COLUMNS, row))
    assert a["m"] <= 0
    return lib.vm_linear_fwd_form(
        pointer(0, a["x"]), a["ldx"], pointer(1, a["w"]), a["ldw"], pointer(2, a["bias"]),
        pointer(3, a["out"]), a["ldo"], a["m"], a["n"], a["k"], a["dtype"], a["form"], None)


def call_add_norm(lib, row):
    a = dict(zip(ADD_NORM_COLUMNS, row))
    assert a["m"] <= 0
    return lib.vm_linear_add_norm_fwd(
        pointer(0, a["x"]), a["ldx"], pointer(1, a["w"]), a["ldw"], pointer(3, a["h"]), a["ldo"],
        pointer(4, a["residual"]), a["ldr"], pointer(5, a["norm_weight"]), 1e-5,
        pointer(6, a["hn"]), a["ldh"], a["m"], a["n"], a["k"], pointer(7, a["counters"]),
        a["counter_bytes"], None)


def answer(lib, call, row):
    rc = call(lib, row)
    return [rc, "" if rc == 0 else lib.vm_last_error().decode()]


def variants(columns, base, changes):
    """`base`, then `base` with each change (a dict of columns) applied alone."""
    rows = [[base[c] for c in columns]]
    for ch in changes:
        assert set(ch) <= set(columns), ch
        rows.append([{**base, **ch}[c] for c in columns])
    return rows


def linear_rows():
    base = dict(x=0, ldx=576, w=0, ldw=576, bias=-1, out=0, ldo=2304, m=0, n=2304, k=576,
                dtype=1, form=0)
    ch = [dict(form=f) for f in (-1, 1, 2, 3)]
    ch += [dict(form=f, k=640, ldx=640, ldw=640) for f in (-1, 0, 1, 2, 3)]  # form before K
    ch += [dict(form=3, n=7)]                                               # form before shape
    ch += [dict(k=k, ldx=max(k, 8), ldw=max(k, 8)) for k in range(0, 2048 + 64, 64)]
    ch += [dict(k=96, ldx=96, ldw=96), dict(k=200, ldx=200, ldw=200), dict(k=-64)]
    ch += [dict(dtype=0), dict(dtype=2), dict(m=-1), dict(n=0), dict(n=8, ldo=8), dict(n=-8),
           dict(n=2300, ldo=2304), dict(n=2296, ldo=2304),
           dict(ldx=575), dict(ldx=568), dict(ldx=584), dict(ldx=580),
           dict(ldw=575), dict(ldw=568), dict(ldw=584), dict(ldw=580),
           dict(ldo=2303), dict(ldo=2296), dict(ldo=2312), dict(ldo=2308),
           dict(x=8), dict(w=8), dict(out=8), dict(x=4), dict(bias=0), dict(bias=4),
           dict(x=-1), dict(w=-1), dict(out=-1),
           # n * ldw * 2 against 2^31 bytes: 2304 * 466034 * 2 is the first product past it
           dict(ldw=466032), dict(ldw=466040), dict(n=8, ldo=8, ldw=(1 << 27) - 8),
           dict(n=8, ldo=8, ldw=1 << 27),
           dict(ldx=1 << 40), dict(ldo=1 << 40),
           # the shape block comes before the K list
           dict(k=640, ldx=640, ldw=640, n=2300), dict(k=640, ldx=640, ldw=640, x=8),
           # m == -1 with a k outside the list: still the shape block
           dict(m=-1, k=640, ldx=640, ldw=640)]
    return variants(LINEAR_COLUMNS, base, ch)


def add_norm_rows():
    base = dict(x=0, ldx=1152, w=0, ldw=1152, h=0, ldo=576, residual=0, ldr=576, norm_weight=0,
                hn=0, ldh=576, m=0, n=576, k=1152, counters=0, counter_bytes=0)
    ch = [dict(k=k, ldx=max(k, 8), ldw=max(k, 8)) for k in range(0, 2048 + 64, 64)]
    ch += [dict(k=96, ldx=96, ldw=96), dict(k=-64)]
    ch += [dict(m=-1), dict(n=0), dict(n=4, ldo=8, ldr=8, ldh=8), dict(n=8, ldo=8, ldr=8, ldh=8),
           dict(n=1024, ldo=1024, ldr=1024, ldh=1024), dict(n=1032, ldo=1032, ldr=1032, ldh=1032),
           dict(n=572), dict(n=568),
           dict(ldx=1151), dict(ldx=1144), dict(ldx=1160), dict(ldx=1156),
           dict(ldw=1151), dict(ldw=1144), dict(ldw=1160), dict(ldw=1156),
           dict(ldo=575), dict(ldo=568), dict(ldo=584), dict(ldo=580),
           dict(ldr=575), dict(ldr=572), dict(ldr=580), dict(ldr=578),
           dict(ldh=575), dict(ldh=572), dict(ldh=580), dict(ldh=578),
           dict(x=8), dict(w=8), dict(h=8), dict(residual=8), dict(norm_weight=8), dict(hn=8),
           dict(counters=8), dict(counters=4),
           dict(x=-1), dict(w=-1), dict(h=-1), dict(residual=-1), dict(norm_weight=-1),
           dict(hn=-1), dict(counters=-1),
           # n * ldw * 2 against 2^31 bytes: 576 * 1864136 * 2 is the first product past it
           dict(ldw=1864128), dict(ldw=1864136),
           dict(counter_bytes=-1), dict(counter_bytes=1 << 20),
           dict(m=-1, counter_bytes=-1),
           dict(k=640, ldx=640, ldw=640, counter_bytes=-1), dict(k=640, ldx=640, ldw=640, hn=8)]
    return variants(ADD_NORM_COLUMNS, base, ch)


COUNTER_M = [-1, 0, 1, 127, 128, 129, 255, 256, 257, 3144, 12552, 40000, 1408512, 1 << 30]


def dump(f, name, rows, last=False):
    f.write(f' "{name}": [\n')
    f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
    f.write("\n ]" + ("\n" if last else ",\n"))


def main():
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        HERE, "..", "..", "videomamba_amd", "libvideomamba_hip.so")
    lib = bind(path)
    lin = [r + answer(lib, call_linear, r) for r in linear_rows()]
    fused = [r + answer(lib, call_add_norm, r) for r in add_norm_rows()]
    cnt = [[m, lib.vm_linear_add_norm_counter_bytes(m)] for m in COUNTER_M]
    with open(os.path.join(HERE, "gemm_refusals.json"), "w") as f:
        f.write("{\n")
        f.write(f' "commit": {json.dumps(commit)},\n')
        f.write(' "note": "vm_linear_fwd_form and vm_linear_add_norm_fwd on calls that cannot '
                'launch (m <= 0), and vm_linear_add_norm_counter_bytes, of the library built at '
                '`commit` (gen_gemm_refusals.py): the arguments, then the return code and the '
                'vm_last_error() text of a refusal; a pointer column is the offset from a made-up '
                'aligned address, -1 = NULL",\n')
        f.write(f' "linear_columns": {json.dumps(LINEAR_COLUMNS + ["rc", "error"])},\n')
        dump(f, "linear_rows", lin)
        f.write(f' "add_norm_columns": {json.dumps(ADD_NORM_COLUMNS + ["rc", "error"])},\n')
        dump(f, "add_norm_rows", fused)
        f.write(' "counter_bytes_columns": ["m", "bytes"],\n')
        dump(f, "counter_bytes_rows", cnt, last=True)
        f.write("}\n")
    print(len(lin), "+", len(fused), "+", len(cnt), "rows")


if __name__ == "__main__":
    main()
