"""CPU tests of the conv1d and add + norm backwards' host side: the float64 autograd references
(tests/train_bwd_ref.py) against the oracle's forwards, the four ABI v16 symbols, the two
workspace queries' bounds, the entries' refusals (no launch happens: there is no GPU here) and
the two backward plans walked by stand-alone programs under ASan + UBSan."""

import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import train_bwd_ref as tbr
from oracle import videomamba_oracle as orc
from videomamba_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV, NORM = b"vm_causal_conv1d_bwd", b"vm_add_norm_bwd"


@pytest.mark.parametrize("state", [None, torch.float32], ids=["nostate", "state"])
@pytest.mark.parametrize("silu,bias", [(True, True), (False, False)], ids=["silu_bias", "plain"])
@pytest.mark.parametrize("width,L", [(4, 24), (3, 2), (2, 1)])
def test_conv_reference_forward_equals_the_oracle(width, L, silu, bias, state):
    ops, _ = tbr.conv_inputs(2, 12, L, width, torch.float32, bias, state)
    ref, _ = orc.causal_conv1d(ops["x"], ops["weight"], ops["bias"], silu=silu,
                               conv_state=ops["conv_state"])
    lv = tbr.leaves64(ops)
    out = tbr.conv_fwd64(lv["x"], lv["weight"], lv["bias"], lv["conv_state"], silu)
    assert out.requires_grad and out.dtype == torch.float64
    torch.testing.assert_close(out.detach().float(), ref, rtol=2e-6, atol=2e-6)
    g = tbr.grads64([out], [torch.ones_like(ref)], lv)
    assert set(g) == {k for k, v in ops.items() if v is not None}
    if state is not None:  # no tap reaches the oldest state entry
        assert float(g["conv_state"][..., 0].abs().max()) == 0.0
        assert width == 1 or float(g["conv_state"][..., -1].abs().max()) > 0.0


@pytest.mark.parametrize("prenorm", [False, True], ids=["y", "prenorm"])
@pytest.mark.parametrize("is_rms,bias", [(True, False), (False, True), (False, False)],
                         ids=["rms", "ln_bias", "ln"])
@pytest.mark.parametrize("res", [None, torch.float32], ids=["nores", "res"])
def test_add_norm_reference_forward_equals_the_oracle(res, is_rms, bias, prenorm):
    ops, _, _ = tbr.norm_inputs(5, 100, torch.float32, bias, res)
    ref = orc.add_norm(ops["x"], ops["residual"], ops["weight"], ops["bias"], 1e-5, prenorm,
                       True, is_rms)
    lv = tbr.leaves64(ops)
    out = tbr.add_norm_fwd64(lv["x"], lv["residual"], lv["weight"], lv["bias"], 1e-5, is_rms,
                             prenorm)
    outs, refs = (out, ref) if prenorm else ((out,), (ref,))
    assert len(outs) == len(refs)
    for o, r in zip(outs, refs):
        assert o.requires_grad
        torch.testing.assert_close(o.detach().float(), r, rtol=2e-6, atol=2e-6)


def test_abi_v16_symbols_load():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 16 and lib.vm_abi_version() == _lib.ABI_VERSION
    for name in ("vm_causal_conv1d_bwd", "vm_causal_conv1d_bwd_workspace_bytes",
                 "vm_add_norm_bwd", "vm_add_norm_bwd_workspace_bytes"):
        assert name in _lib.EXPORTED
        assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None


def test_conv_bwd_workspace_query_is_bounded_and_grows():
    """At most 20 batch dpad (seqlen / 61 + 1) bytes, dpad = round_up(dim, 64) (the header's
    bound): (width + 1) fp32 rows per (batch row, 61-step tile) — a small fraction of the
    operands — more for a larger batch, a longer sequence, more channels or a wider conv;
    pure host code."""
    q = _lib.load().vm_causal_conv1d_bwd_workspace_bytes
    for b, d, l, w in [(3, 136, 150, 4), (32, 1152, 1569, 4), (1, 64, 1, 2), (8, 1152, 1569, 3)]:
        dpad = (d + 63) // 64 * 64
        got = q(b, d, l, w)
        assert 0 < got <= 20 * b * dpad * (l // 61 + 1), (b, d, l, w, got)
        assert got % 4 == 0
        assert q(b + 1, d, l, w) > got and q(b, d, l + 61, w) > got and q(b, d + 64, l, w) > got
        assert w == 4 or q(b, d, l, w + 1) > got
        assert q(b, d, l + 1, w) >= got
    assert q(0, 64, 10, 4) == 0 and q(2, 0, 10, 4) == 0 and q(2, 64, 0, 4) == 0


def test_norm_bwd_workspace_query_is_bounded_and_grows():
    """At most 8 cpad min(2048, rows / 4 + 1) bytes, cpad = round_up(cols, 64) (the header's
    bound): two fp32 rows per workgroup, at most 2048 workgroups whatever the row count; pure
    host code."""
    q = _lib.load().vm_add_norm_bwd_workspace_bytes
    for r, c in [(1, 64), (5, 100), (257, 576), (50208, 576), (10 ** 7, 2048)]:
        cpad = (c + 63) // 64 * 64
        got = q(r, c)
        assert 0 < got <= 8 * cpad * min(2048, r // 4 + 1), (r, c, got)
        assert q(r, c + 64) > got if c + 64 <= 2048 else True
        assert q(r + 4, c) >= got
    assert q(8, 64) > q(4, 64) and q(4096, 576) > q(257, 576)
    assert q(10 ** 9, 2048) == q(10 ** 7, 2048) <= 32 << 20  # capped
    assert q(0, 64) == 0 and q(16, 2049) == 0  # a column count the entry refuses


def _conv_args(lib, ptr, *, shape=(3, 136, 24), sd=1, width=4, dtype=0, ws_short=0, bias=True,
               dbias=True):
    """vm_causal_conv1d_bwd arguments of a token-major fp32 case whose every pointer is ``ptr``
    (never dereferenced: each call here is refused before any launch)."""
    Bz, D, L = shape
    x = (ptr, L * D, sd, D)
    need = lib.vm_causal_conv1d_bwd_workspace_bytes(Bz, D, L, min(width, 4))
    return [*x, ptr, ptr if bias else None, ptr, 0, D * width, width, *x, *x,
            ptr, D * width, width, ptr, ptr if dbias else None,
            Bz, D, L, width, 1, dtype, ptr, need - ws_short, None]


def _norm_args(lib, ptr, *, rows=257, cols=576, dtype=0, ws_short=0, bias=True, dbias=True):
    need = lib.vm_add_norm_bwd_workspace_bytes(rows, min(cols, 2048))
    return [ptr, dtype, ptr, ptr if bias else None, ptr, 0, ptr, ptr, 0, ptr, 0, ptr,
            ptr if dbias else None, rows, cols, 1e-5, 1, ptr, need - ws_short, None]


def _other_entrys_message(lib):
    lib.vm_add_norm_fwd(None, 0, None, 0, None, None, None, 0, None, 0, 4, 64, 1e-5, 1, None)
    assert b"vm_add_norm_fwd" in lib.vm_last_error()


def test_conv_bwd_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    host = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(host)
    assert len(_conv_args(lib, ptr)) == len(_lib._SIGNATURES["vm_causal_conv1d_bwd"][0])
    null = _conv_args(lib, None)
    null[-3:] = [None, 0, None]
    cases = {
        "all-null": null,
        "channel stride": _conv_args(lib, ptr, sd=2),
        "width 5": _conv_args(lib, ptr, width=5),
        "dtype": _conv_args(lib, ptr, dtype=7),
        "short workspace": _conv_args(lib, ptr, ws_short=1),
        "dbias without bias": _conv_args(lib, ptr, bias=False),
        "bias without dbias": _conv_args(lib, ptr, dbias=False),
    }
    for what, args in cases.items():
        _other_entrys_message(lib)
        assert CONV not in lib.vm_last_error()
        assert lib.vm_causal_conv1d_bwd(*args) == -1, what
        assert CONV in lib.vm_last_error(), (what, lib.vm_last_error())
    args = _conv_args(lib, ptr)
    args[10] = None  # dout
    assert lib.vm_causal_conv1d_bwd(*args) == -1 and CONV in lib.vm_last_error()


def test_norm_bwd_entry_refuses_bad_arguments_without_gpu():
    lib = _lib.load()
    host = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(host)
    assert len(_norm_args(lib, ptr)) == len(_lib._SIGNATURES["vm_add_norm_bwd"][0])
    null = _norm_args(lib, None)
    null[-3:] = [None, 0, None]
    cases = {
        "all-null": null,
        "cols 2049": _norm_args(lib, ptr, cols=2049),
        "cols 0": _norm_args(lib, ptr, cols=0),
        "dtype": _norm_args(lib, ptr, dtype=7),
        "short workspace": _norm_args(lib, ptr, ws_short=1),
        "dbias without bias": _norm_args(lib, ptr, bias=False),
        "bias without dbias": _norm_args(lib, ptr, dbias=False),
    }
    for what, args in cases.items():
        _other_entrys_message(lib)
        assert NORM not in lib.vm_last_error()
        assert lib.vm_add_norm_bwd(*args) == -1, what
        assert NORM in lib.vm_last_error(), (what, lib.vm_last_error())
    args = _norm_args(lib, ptr)
    args[4] = None  # dy
    assert lib.vm_add_norm_bwd(*args) == -1 and NORM in lib.vm_last_error()


@pytest.mark.parametrize("name", ["conv_bwd_plan_check", "norm_bwd_plan_check"])
def test_bwd_plan_check_programs_pass_under_sanitizers(tmp_path, name):
    """tests/host/conv_bwd_plan_check.cpp and norm_bwd_plan_check.cpp walk plan_conv_bwd /
    plan_norm_bwd over a grid of shapes and exit non-zero on overlapping or out-of-size
    regions, an empty range, or rows / tiles / parts not covered exactly once.  Programs of
    their own built with the host compiler under ASan + UBSan; nothing is loaded into Python."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / name)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "videomamba_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe],
                   check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
