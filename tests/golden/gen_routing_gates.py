"""Records what the Python routing gates answer over a grid of calls, into routing_gates.json.

    python tests/golden/gen_routing_gates.py <commit>

Run at the commit the table is to name (the last one whose gates decided from Python copies of
the kernels' limits).  The gates are ``mamba_simple._small_gemm_ok``,
``kernels._linear_fn_hip_ok``, ``kernels.scan_dtproj_segmented_pays``, ``Mamba._dtp_ok`` and
``Mamba._fused_conv_proj_ok``.  No device is needed: the operands are stand-ins that carry a
shape, strides, a made-up address, a dtype and ``is_cuda``, and the CU count is pinned
(:func:`pinned_cus`).  tests/test_routing_gates_cpu.py replays every row through the functions
below against the gates of the tree it runs in.
"""

import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
CUS = 256  # the CU count the mixer gates are recorded with


class Operand:
    """What a gate reads of a tensor, with no storage behind it.  ``off`` is the byte offset
    from a made-up 16-byte aligned address."""

    is_cuda = True
    requires_grad = False

    def __init__(self, shape, strides=None, off=0, dtype="bf16", slot=0):
        self.shape = tuple(shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(self.shape):
                strides.insert(0, acc)
                acc *= s
        self._strides = tuple(strides)
        self._ptr = ((slot + 1) << 40) + off
        self.dtype = DTYPES[dtype]
        self.device = torch.device("cuda", 0)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def data_ptr(self):
        return self._ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def element_size(self):
        return 2 if self.dtype == torch.bfloat16 else 4


@contextlib.contextmanager
def pinned_cus(cus):
    """The CU count the scan gates see: the recorded tree looked it up through
    ``kernels._cu_count``; later trees pass it to the library's query."""
    from videomamba_amd import kernels as K
    if hasattr(K, "_cu_count"):
        old, K._cu_count = K._cu_count, lambda device: cus
        try:
            yield
        finally:
            K._cu_count = old
        return
    old = K.scan_dtproj_fits
    K.scan_dtproj_fits = lambda *a, **k: old(*a, **{**k, "cus": cus})
    try:
        yield
    finally:
        K.scan_dtproj_fits = old


# ---------------------------------------------------------------- _small_gemm_ok
GEMM_COLUMNS = ["m", "n", "k", "ldx", "ldw", "ldo", "x_off", "w_off", "o_off", "bias", "dtype",
                "projection_gemm", "clips"]  # ldo -1: no out; clips -1: None
M_PAST_2GB = 5_600_000  # x (m, 192) bf16 is past 2^31 bytes from 5,592,406 rows
MS = [1, 127, 128, 129, 3144, 1 << 20, M_PAST_2GB]
MULT64 = list(range(64, 2560 + 64, 64))
PAIRS = [(2304, 576), (576, 1152), (192, 192), (200, 192), (1000, 384)]


def gemm_rows():
    def row(m, n, k, **ch):
        a = dict(m=m, n=n, k=k, ldx=k, ldw=k, ldo=-1, x_off=0, w_off=0, o_off=0, bias=0,
                 dtype="bf16", projection_gemm="hip", clips=-1)
        a.update(ch)
        return [a[c] for c in GEMM_COLUMNS]

    rows = []
    for k in MULT64 + [96, 200, 1000, 8]:
        for n in (192, 200, 256, 1152, 2304, 100):
            rows.append(row(129, n, k))
    for n in MULT64 + [8, 100, 196, 1000]:
        for k in (192, 576, 640):
            rows.append(row(3144, n, k))
    for m in MS + [0]:
        for n, k in PAIRS:
            for ldx in (k, k + 8, k + 4, k - 8):
                rows.append(row(m, n, k, ldx=ldx))
            rows.append(row(m, n, k, ldw=k + 8))
            rows.append(row(m, n, k, ldw=k + 4))
            rows.append(row(m, n, k, ldw=k - 8))
            for ldo in (n, n + 8, n + 4, n - 8):
                rows.append(row(m, n, k, ldo=ldo))
    # w past 2 GB: n * ldw * 2 >= 2^31
    rows.append(row(129, 2304, 576, ldw=466040))
    rows.append(row(129, 2304, 576, ldw=466032))
    for m in (1, 129):
        for n, k in PAIRS:
            for ch in (dict(x_off=8), dict(w_off=8), dict(ldo=n, o_off=8), dict(x_off=4),
                       dict(bias=1), dict(dtype="f32")):
                rows.append(row(m, n, k, **ch))
    for mode in ("hip", "library"):
        for clips in (-1, 1, 2, 4, 8, 9, 72):
            for m in MS:
                for n, k in PAIRS[:4]:
                    rows.append(row(m, n, k, projection_gemm=mode, clips=clips))
    return rows


def gemm_operands(r):
    a = dict(zip(GEMM_COLUMNS, r))
    x = Operand((a["m"], a["k"]), (a["ldx"], 1), a["x_off"], a["dtype"], 0)
    w = Operand((a["n"], a["k"]), (a["ldw"], 1), a["w_off"], a["dtype"], 1)
    b = Operand((a["n"],), None, 0, "f32", 2) if a["bias"] else None
    out = None if a["ldo"] < 0 else Operand((a["m"], a["n"]), (a["ldo"], 1), a["o_off"],
                                            a["dtype"], 3)
    return a, x, w, b, out


def call_gemm(r):
    from videomamba_amd import options
    from videomamba_amd.mamba_simple import _small_gemm_ok
    a, x, w, b, out = gemm_operands(r)
    with options.override(projection_gemm=a["projection_gemm"]):
        return bool(_small_gemm_ok(x, w, b, out, clips=None if a["clips"] < 0 else a["clips"]))


# ---------------------------------------------------------------- _linear_fn_hip_ok
FN_COLUMNS = ["lead", "n", "k", "bias", "x_dtype", "w_dtype"]  # x is (*lead, k)


def fn_rows():
    rows = []
    for k in MULT64 + [96, 200]:
        for n in (192, 2304, 2368, 200):
            for lead in ([1], [8, 393]):
                rows.append([lead, n, k, 0, "bf16", "bf16"])
    for n in MULT64 + [8, 100]:
        for k in (192, 576):
            rows.append([[129], n, k, 0, "bf16", "bf16"])
    for m in MS + [0, 400_000, 700_000, 932_067, 932_068]:  # m * 1152 * 2 = 2^31 at 932,067.6
        for n, k in PAIRS:
            rows.append([[m], n, k, 0, "bf16", "bf16"])
    for n, k in PAIRS:
        rows.append([[129], n, k, 1, "bf16", "bf16"])
        rows.append([[129], n, k, 0, "f32", "bf16"])
        rows.append([[129], n, k, 0, "bf16", "f32"])
        rows.append([[], n, k, 0, "bf16", "bf16"])
    return rows


def call_fn(r):
    from videomamba_amd import kernels as K
    lead, n, k, bias, xd, wd = r
    x = Operand(tuple(lead) + (k,), None, 0, xd, 0)
    w = Operand((n, k), None, 0, wd, 1)
    b = Operand((n,), None, 0, "f32", 2) if bias else None
    return bool(K._linear_fn_hip_ok(x, w, b))


# ---------------------------------------------------------------- scan_dtproj_segmented_pays
PAYS_COLUMNS = ["batch", "dim", "seqlen", "dstate", "segments", "cus"]


def pays_rows():
    table = json.load(open(os.path.join(HERE, "scan_size_queries.json")))
    rows = []
    for b, d, l, seg, n, ws, sync, steps in table["rows"]:
        wgs = (sync - 16) // (17 * 64 * 8) if steps > 0 else CUS
        rows.append([b, d, l, n, seg, wgs])
        if steps > 0 and wgs > 1:  # a CU count of 0 asks a later tree for the current device's
            rows.append([b, d, l, n, seg, wgs - 1])
    return rows


def call_pays(r):
    from videomamba_amd import kernels as K
    b, d, l, n, seg, cus = r
    if hasattr(K, "_cu_count"):
        with pinned_cus(cus):
            return bool(K.scan_dtproj_segmented_pays(b, d, l, n, "cpu", seg))
    return bool(K.scan_dtproj_segmented_pays(b, d, l, n, segments=seg, cus=cus))


# ---------------------------------------------------------------- the mixer's gates
MIXERS = [dict(d_model=576), dict(d_model=192), dict(d_model=96), dict(d_model=192, dt_rank=6),
          dict(d_model=192, d_state=8), dict(d_model=192, d_conv=5), dict(d_model=200)]
_MIXER_CACHE = {}


def mixer(i):
    from videomamba_amd.mamba_simple import Mamba
    if i not in _MIXER_CACHE:
        _MIXER_CACHE[i] = Mamba(**MIXERS[i]).to(torch.bfloat16)
    return _MIXER_CACHE[i]


def hn_of(i, clips, seqlen, dtype="bf16"):
    return Operand((clips, (max(seqlen, 1) + 7) // 8 * 8, MIXERS[i]["d_model"]), None, 0, dtype)


DTP_COLUMNS = ["mixer", "clips", "seqlen", "scan_dt_proj", "scan_segments", "fused_conv_proj"]
CLIPS = [1, 2, 4, 8, 9, 72]


def dtp_rows():
    rows = []
    for i in range(len(MIXERS)):
        for clips in CLIPS:
            for seqlen in (64, 200, 1569, 3137):
                for mode in ("auto", "on", "off"):
                    for seg in (0, 20):
                        rows.append([i, clips, seqlen, mode, seg, 1])
    for clips in CLIPS:
        rows.append([0, clips, 3137, "auto", 0, 0])
        rows.append([0, clips, 300_000, "auto", 0, 1])
        rows.append([0, clips, 300_000, "on", 0, 1])
    return rows


def call_dtp(r):
    from videomamba_amd import options
    i, clips, seqlen, mode, seg, fused = r
    with options.override(scan_dt_proj=mode, scan_segments=seg, fused_conv_proj=bool(fused)), \
            pinned_cus(CUS):
        return bool(mixer(i)._dtp_ok(hn_of(i, clips, seqlen), seqlen))


FUSED_COLUMNS = ["mixer", "clips", "seqlen", "tm", "fused_conv_proj", "dtype"]


def fused_rows():
    rows = []
    for i in range(len(MIXERS)):
        for clips in (1, 8, 9, 72):
            for seqlen in (0, 1, 3137, 300_000):
                for tm in (1, 0):
                    rows.append([i, clips, seqlen, tm, 1, "bf16"])
        rows.append([i, 2, 3137, 1, 0, "bf16"])
        rows.append([i, 2, 3137, 1, 1, "f32"])
    return rows


def call_fused(r):
    from videomamba_amd import options
    i, clips, seqlen, tm, fused, dtype = r
    with options.override(fused_conv_proj=bool(fused)):
        return bool(mixer(i)._fused_conv_proj_ok(hn_of(i, clips, seqlen, dtype), seqlen,
                                                 tm=bool(tm)))


GATES = [("small_gemm", GEMM_COLUMNS, gemm_rows, call_gemm),
         ("linear_fn", FN_COLUMNS, fn_rows, call_fn),
         ("scan_pays", PAYS_COLUMNS, pays_rows, call_pays),
         ("dtp", DTP_COLUMNS, dtp_rows, call_dtp),
         ("fused_conv_proj", FUSED_COLUMNS, fused_rows, call_fused)]


def main():
    commit = sys.argv[1]
    total = 0
    with open(os.path.join(HERE, "routing_gates.json"), "w") as f:
        f.write("{\n")
        f.write(f' "commit": {json.dumps(commit)},\n')
        f.write(' "note": "the routing gates of the tree at `commit` over stand-in operands '
                f'(gen_routing_gates.py), the mixer gates with {CUS} CUs: the arguments, then 1 '
                'where the gate sends the call to the HIP kernel, else 0",\n')
        for name, columns, rows, call in GATES:
            out = [r + [int(call(r))] for r in rows()]
            total += len(out)
            print(name, len(out), "rows,", sum(r[-1] for r in out), "accepted")
            f.write(f' "{name}_columns": {json.dumps(columns + ["answer"])},\n')
            f.write(f' "{name}_rows": [\n')
            f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in out))
            f.write("\n ],\n")
        f.write(f' "rows": {total}\n')
        f.write("}\n")
    print(total, "rows")


if __name__ == "__main__":
    main()
