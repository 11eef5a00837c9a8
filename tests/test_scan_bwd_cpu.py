"""CPU tests of the selective scan backward's host side: the float64 autograd reference
(tests/scan_bwd_ref.py) against the forward matrix's reference, the two ABI v15 symbols, the
workspace query's bound, the entry's refusals (no launch happens: there is no GPU here) and
the backward plan walked by a stand-alone program under ASan + UBSan."""

import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import scan_bwd_ref as sbr
import scan_matrix as sm
from videomamba_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b"vm_selective_scan_bwd"


@pytest.mark.parametrize("row", [sm.ROWS[1], sm.ROWS[4]], ids=lambda r: r.id)
def test_differentiable_reference_forward_equals_scan_ref64(row):
    """scan_fwd64 on float64 leaves computes what scan_matrix.scan_ref64 computes (the same
    operations in the same order), so its autograd gradients are the reference's."""
    inp = sm.make_inputs(row, torch.float32, 2, 136, 24, 16, seed=1)
    ref_y, ref_h = inp.ref(row.softplus)
    lv = sbr.leaves64(inp)
    y, h = sbr.scan_fwd64(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], lv["z"],
                          lv["bias"], row.softplus, lv["h0"])
    assert y.requires_grad and h.requires_grad
    torch.testing.assert_close(y.detach(), ref_y, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(h.detach(), ref_h, rtol=1e-13, atol=1e-13)


def test_reference_rows_and_gradients():
    """Eight rows, none with the in-place bf16 state, covering D / z / bias / softplus on and
    off and the four differentiable state kinds; grads64 returns one gradient per present
    operand, in the operand's shape."""
    assert len(sbr.ROWS) == 8
    assert {r.state for r in sbr.ROWS} == {"none", "hl", "h0", "h0_hl"}
    for k in ("D", "z", "bias", "softplus"):
        assert {getattr(r, k) for r in sbr.ROWS} == {False, True}
    row = sm.ROWS[1]
    shape = (2, 136, 5, 16)
    inp = sm.make_inputs(row, torch.bfloat16, *shape, seed=1)
    dout, dhl = sbr.make_dout(row, torch.bfloat16, shape)
    assert dout.dtype == torch.bfloat16 and dhl is not None and dhl.dtype == torch.float32
    g = sbr.grads64(inp, row, dout, dhl)
    assert set(g) == set(sbr.NAMES)
    for k, v in zip(sbr.NAMES, inp):
        assert g[k].shape == v.shape and g[k].dtype == torch.float64
    assert sbr.make_dout(sm.ROWS[2], torch.float32, shape)[1] is None  # state "none"


def test_comparator_has_an_rms_floor():
    ref = torch.tensor([100.0, 0.0, -100.0, 0.0])
    rms = float(ref.pow(2).mean().sqrt())
    got = ref + torch.tensor([0.0, 0.9e-4 * rms, 0.0, 1.1e-4 * rms])
    r = sbr.rms_ratio(got, ref, 1e-4)
    assert r[1] < 1.0 < r[3] and r[0] == 0.0
    with pytest.raises(AssertionError):
        sbr.assert_within_rms(got, ref, 1e-4, "x")
    assert sbr.assert_within_rms(got[:3], ref[:3], 1e-4, "x") < 1.0
    with pytest.raises(AssertionError):
        sbr.assert_within_rms(torch.tensor([float("nan")]), torch.tensor([1.0]), 1e-4, "nan")


def test_abi_v15_symbols_load():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 15 and lib.vm_abi_version() == _lib.ABI_VERSION
    for name in ("vm_selective_scan_bwd", "vm_selective_scan_bwd_workspace_bytes"):
        assert name in _lib.EXPORTED
        assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None


def test_bwd_workspace_query_is_bounded_and_grows():
    """At most 12 batch seqlen dpad + 4 batch dpad (dstate + 2) + 4096 bytes (checkpoints every
    >= 8 steps plus the dB | dC partials; a per-step state dump would be 64 bytes per
    element), more for a larger batch or a longer sequence, pure host code."""
    lib = _lib.load()
    q = lib.vm_selective_scan_bwd_workspace_bytes
    for b, d, l, n in [(2, 136, 150, 16), (32, 1152, 1569, 16), (1, 64, 1, 16)]:
        dpad = (d + 63) // 64 * 64
        got = q(b, d, l, n)
        assert 0 < got <= 12 * b * l * dpad + 4 * b * dpad * (n + 2) + 4096, (b, d, l, got)
        assert got < 64 * b * l * dpad or l < 8
        assert q(b + 1, d, l, n) > got and q(b, d, l + 8, n) > got
        assert q(b, d, l + 1, n) > got
    assert q(2, 136, 150, 8) == 0  # a state count the entry refuses


def _args(lib, ptr, *, shape=(2, 136, 24), sd=1, dstate=16, dtype=0, ws_short=0):
    """vm_selective_scan_bwd arguments of a token-major fp32 case whose every pointer is
    ``ptr`` (never dereferenced: each call here is refused before any launch)."""
    Bz, D, L = shape
    x = (ptr, L * D, sd, D)
    bc = (ptr, L * 16, 1, 16)
    st = (ptr, D * 16, 16)
    need = lib.vm_selective_scan_bwd_workspace_bytes(Bz, D, L, 16)
    return [*x, *x, ptr, *bc, *bc, ptr, *x, ptr, 1, ptr, 0, D * 16, 16,  # inputs .. h0
            *x, *st,                                                    # dout, dh_last
            *x, *x, *x, *bc, *bc, ptr, ptr, ptr, *st,                   # gradients
            Bz, D, L, dstate, dtype, ptr, need - ws_short, None]


def test_bwd_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    nargs = len(_lib._SIGNATURES["vm_selective_scan_bwd"][0])
    host = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(host)
    assert len(_args(lib, ptr)) == nargs
    null = _args(lib, None)
    null[-3:] = [None, 0, None]
    cases = {
        "all-null": null,
        "dstate 8": _args(lib, ptr, dstate=8),
        "channel stride": _args(lib, ptr, sd=2),
        "short workspace": _args(lib, ptr, ws_short=1),
        "dtype": _args(lib, ptr, dtype=7),
    }
    for what, args in cases.items():
        lib.vm_selective_scan_fwd(*([None, 0, 0, 0] * 2), None, *([None, 0, 0, 0] * 2),
                                  None, None, 0, 0, 0, None, 0, None, 0, 0, 0, None, 0, 0, 0,
                                  None, 0, 0, 0, 0, 1, 1, 1, 16, 0, 0, None, 0, None, 0, None)
        assert ENTRY not in lib.vm_last_error()  # another entry's message is in place
        assert lib.vm_selective_scan_bwd(*args) == -1, what
        assert ENTRY in lib.vm_last_error(), (what, lib.vm_last_error())
    # dz goes with z: a gradient buffer for an absent operand is refused as well
    args = _args(lib, ptr)
    args[18] = None  # z
    assert lib.vm_selective_scan_bwd(*args) == -1 and ENTRY in lib.vm_last_error()


def test_scan_bwd_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/scan_bwd_plan_check.cpp walks vm_scan_bwd_plan.h::plan_scan_bwd over batch x
    dim x seqlen and exits non-zero on overlapping or out-of-size workspace regions, a size
    past the documented bound, or an empty / overlong chunk.  A program of its own built with
    the host compiler under ASan + UBSan; nothing is loaded into Python."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "scan_bwd_plan_check")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "scan_bwd_plan_check.cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
