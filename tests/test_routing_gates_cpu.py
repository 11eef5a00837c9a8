"""The Python routing gates against their recorded answers (tests/golden/routing_gates.json,
written by tests/golden/gen_routing_gates.py at the last commit whose gates decided from Python
copies of the kernels' limits).  The gates now keep policy and ask the library's fits queries
for everything else; every recorded answer must come back, except where the old copy said yes
and the kernel's own plan refuses (such a call used to raise).  No GPU: stand-in operands."""

import importlib.util
import json
import os

import pytest

from videomamba_amd import _lib
from videomamba_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location(
        "gen_routing_gates", os.path.join(GOLDEN, "gen_routing_gates.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(GOLDEN, "routing_gates.json")))


# ---------------------------------------------------------------- what the library says of a row
def _gemm_library(gen, r):
    a, x, w, b, out = gen.gemm_operands(r)
    ldo = a["n"] if out is None else out.stride(0)
    return K.linear_fits(a["m"], a["n"], a["k"], a["ldx"], a["ldw"], ldo, x.data_ptr(),
                         w.data_ptr(), 0 if out is None else out.data_ptr(), bool(b),
                         K.dtype_code(x.dtype))


def _fn_library(gen, r):
    lead, n, k = r[0], r[1], r[2]
    m = 1
    for s in lead:
        m *= s
    return K.linear_fn_fits(m, n, k)


def _pays_library(gen, r):
    b, d, l, n, seg, cus = r
    return K.scan_dtproj_fits(b, d, l, n, 4, seg, cus) != 0


def _conv_proj_library(gen, r):
    i, clips, seqlen = r[0], r[1], r[2]
    mx = gen.mixer(i)
    Lp, Dm = (max(seqlen, 1) + 7) // 8 * 8, mx.d_inner
    return K.conv_proj_fits(clips, Lp, seqlen, Dm, mx.dt_rank + 2 * mx.d_state,
                            32 if mx.dt_rank <= 32 else 64, (Lp * 2 * Dm, 2 * Dm), Dm, None,
                            mx.d_conv)


def _dtp_library(gen, r):
    i, clips, seqlen, seg = r[0], r[1], r[2], r[4]
    mx = gen.mixer(i)
    return _conv_proj_library(gen, r) and K.scan_dtproj_fits(
        clips, mx.d_inner, seqlen, mx.d_state, mx.dt_rank, seg, gen.CUS) != 0


def _fused_library(gen, r):
    return not r[3] or _conv_proj_library(gen, r)  # the channel-major branch has no query


LIBRARY = {"small_gemm": _gemm_library, "linear_fn": _fn_library, "scan_pays": _pays_library,
           "dtp": _dtp_library, "fused_conv_proj": _fused_library}

# ---------------------------------------------------------------- the permitted deviations
# Rows where the recorded gate said yes and the new one says no.  Each class names the limit of
# the kernel's plan that the old Python copy did not have: such a call reached the entry and
# raised, and now takes the library path.
_G = {c: i for i, c in enumerate(
    ["m", "n", "k", "ldx", "ldw", "ldo", "x_off", "w_off", "o_off", "bias", "dtype",
     "projection_gemm", "clips"])}
DEVIATIONS = {
    "small_gemm": [
        ("ldx < k: plan_linear's shape block refuses a row stride below the width",
         lambda r: r[_G["ldx"]] < r[_G["k"]]),
        ("ldw < k: the same, for w", lambda r: r[_G["ldw"]] < r[_G["k"]]),
        ("ldo < n: the same, for out", lambda r: 0 <= r[_G["ldo"]] < r[_G["n"]]),
        ("w past 2 GB: n * ldw * 2 >= 2^31 (plan_linear's shape block)",
         lambda r: r[_G["n"]] * r[_G["ldw"]] * 2 >= 1 << 31),
        ("x past 2 GB where the persistent form does not fill the chip (gemm_tile_fills: no "
         "persistent form at all on a host without a device)",
         lambda r: r[_G["m"]] * r[_G["ldx"]] * 2 >= 1 << 31),
    ],
    "scan_pays": [
        ("dstate != 16: vm_selective_scan_dtproj_fwd takes 16 states only (the mixer's own gate "
         "asked for them, so its routing is unchanged)", lambda r: r[3] != 16),
    ],
    "linear_fn": [], "dtp": [], "fused_conv_proj": [],
}


def test_routing_gates_answer_as_recorded(gen, table):
    assert table["commit"]
    assert table["rows"] == sum(len(table[name + "_rows"]) for name, *_ in gen.GATES) >= 2000
    accepted = by_policy = by_library = deviations = 0
    bad = []
    for name, columns, _rows, call in gen.GATES:
        assert table[name + "_columns"] == columns + ["answer"]
        for row in table[name + "_rows"]:
            args, old = row[:-1], bool(row[-1])
            new = call(args)
            lib = bool(LIBRARY[name](gen, args))
            if new and not lib:
                bad.append((name, row, "accepted what the library refuses"))
            if new == old:
                if new:
                    accepted += 1
                elif lib:
                    by_policy += 1
                else:
                    by_library += 1
                continue
            # a deviation: only yes -> no, only where the library itself refuses, only listed
            why = [text for text, match in DEVIATIONS[name] if match(args)]
            if not (old and not new and not lib and why):
                bad.append((name, row, new))
            deviations += 1
    assert not bad, (len(bad), bad[:8])
    assert accepted >= 100 and by_policy >= 100 and by_library >= 100, \
        (accepted, by_policy, by_library)
    print(f"{table['rows']} rows: {accepted} accepted, {by_policy} refused by policy, "
          f"{by_library} refused by the library, {deviations} deviations")


def test_conv_bwd_max_width_is_the_library_s():
    """kernels.CONV_BWD_MAX_WIDTH against vm_causal_conv1d_bwd itself.  The entry's empty
    return is ``dim == 0`` (an empty batch still launches the kernels that zero dweight), and
    it comes after the width test: with batch == 0 and dim == 0 nothing can launch, the entry
    accepts that width and refuses the next (made-up addresses, never dereferenced)."""
    lib = _lib.load()
    fake = lambda i: (i + 1) << 20  # noqa: E731

    def rc(width):
        return lib.vm_causal_conv1d_bwd(
            fake(0), 64 * 8, 1, 64, fake(1), fake(2), None, 0, 0, 0, fake(3), 64 * 8, 1, 64,
            fake(4), 64 * 8, 1, 64, None, 0, 0, fake(5), fake(6), 0, 0, 8, width, 1,
            _lib.VM_DTYPE_BF16, None, 0, None)

    assert rc(K.CONV_BWD_MAX_WIDTH) == 0, lib.vm_last_error()
    assert rc(K.CONV_BWD_MAX_WIDTH + 1) == -1
    assert b"width" in lib.vm_last_error()


def test_scan_dtproj_max_segment_is_the_library_s():
    """kernels.SCAN_DTPROJ_MAX_SEGMENT against vm_selective_scan_dtproj_fits (pure host code,
    nothing can launch): eight forced segments of exactly that many steps take the segmented
    form, one step more per segment and the entry would refuse."""
    T = K.SCAN_DTPROJ_MAX_SEGMENT
    assert K.scan_chunk_steps(1, 128, 8 * T, 16, 8) == T
    assert K.scan_dtproj_fits(1, 128, 8 * T, 16, 4, 8) >= 2
    assert K.scan_chunk_steps(1, 128, 8 * T + 8, 16, 8) == T + 1
    assert K.scan_dtproj_fits(1, 128, 8 * T + 8, 16, 4, 8) == 0
