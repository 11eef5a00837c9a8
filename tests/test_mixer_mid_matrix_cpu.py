"""Keeps the mixer-middle option matrix honest without a GPU: the float64 reference against
the oracle, the state rule, each form's covering array, the inputs' sensitivity (every
operand the kernels could mishandle must move the outputs by far more than the bound the
GPU tests compare with) and the form every case names, against plan_conv_proj itself."""

import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import mixer_mid_matrix as mm
from oracle import videomamba_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _close(got, ref, tol=1e-6):
    return mm.assert_within(got, ref, (tol, tol), "reference vs oracle")


# --------------------------------------------------------------------------- reference
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("state", ["none", "bf16"])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
@pytest.mark.parametrize("L", [1, 2, 13])
def test_ref64_matches_oracle_conv_and_fp32_linear(L, width, state, with_bias):
    """mid_ref64 against oracle.causal_conv1d run in fp32 on fp32 operands (a state holding
    bf16 values: the oracle casts the state to x's dtype, fp32 here), u within 1e-6 abs+rel
    and the new state exact, for sequences shorter than the kernel too; proj_ref64 against
    fp32 F.linear of the same rows."""
    g = torch.Generator().manual_seed(100 * L + 10 * width + with_bias)
    B, D, E = 3, 24, 10
    x = torch.randn(B, L, D, generator=g).to(BF16).float()
    cw = torch.rand(D, width, generator=g) - 0.5
    cb = torch.rand(D, generator=g) - 0.5 if with_bias else None
    cs = torch.randn(B, D, width, generator=g).to(BF16).float() if state != "none" else None
    u, new = mm.mid_ref64(x, cw, cb, cs)
    ref_u, ref_new = orc.causal_conv1d(x.transpose(1, 2), cw, cb, True, cs)
    _close(u, ref_u.transpose(1, 2).double())
    assert torch.equal(new, ref_new.double())
    wx = (torch.rand(E, D, generator=g) - 0.5).to(BF16)
    ub = u.float().to(BF16)
    _close(mm.proj_ref64(ub, wx), F.linear(ub.float(), wx.float()).double())


@pytest.mark.parametrize("width", [2, 3, 4])
def test_ref64_casts_an_fp32_state_to_bf16_first(width):
    """The oracle's rule (``conv_state.to(x.dtype)`` with a bf16 x): an fp32 state and its
    bf16 rounding give the same reference, bit for bit, and the conv of the un-rounded taps
    leaves the u bound in the first width - 1 steps (where u is small: the taps move the
    pre-activation by ~2^-9 of a tap, the bound is 2^-7 |u| + 1e-5) and nowhere else.
    The oracle itself, run on the bf16 x with the fp32 state, returns the same new state
    and a u within one bf16 rounding of the reference."""
    g = torch.Generator().manual_seed(width)
    B, L, D = 2, 3, 256
    x = torch.randn(B, L, D, generator=g).to(BF16)
    cw = torch.rand(D, width, generator=g) - 0.5
    cs = torch.randn(B, D, width, generator=g)
    assert not torch.equal(cs, cs.to(BF16).float())
    u32, new32 = mm.mid_ref64(x, cw, None, cs)
    u16, new16 = mm.mid_ref64(x, cw, None, cs.to(BF16))
    assert torch.equal(u32, u16) and torch.equal(new32, new16)
    # what a kernel convolving the fp32 taps computes: the same conv on the raw state
    full = torch.cat([cs.double().transpose(1, 2), x.double()], 1)
    pre = sum(cw[:, k].double() * full[:, 1 + k: 1 + k + L] for k in range(width))
    raw = pre / (1.0 + torch.exp(-pre))
    assert mm.mismatch(raw[:, : width - 1], u32[:, : width - 1], mm.TOL_U).sum() >= 8
    assert torch.equal(raw[:, width - 1:], u32[:, width - 1:])
    ref_u, ref_new = orc.causal_conv1d(x.transpose(1, 2), cw, None, True, cs)
    assert torch.equal(ref_new.double(), new32)
    mm.assert_within(ref_u.transpose(1, 2), u32, (2.0 ** -7, 1e-5), "oracle u")


# --------------------------------------------------------------------------- tables
@pytest.mark.parametrize("form", mm.FORMS)
def test_option_table_is_a_strength_2_covering_array(form):
    rows = mm.ROWS[form]
    assert mm.covering_gaps(form, rows) == []
    assert len(rows) <= mm.MAX_ROWS and len(set(rows)) == len(rows)
    # every level of every factor is a level the form has (softplus: the wide form only)
    assert any(r.softplus for r in rows) == (form == "wide")
    assert {r.width for r in rows} == {1, 2, 3, 4}


@pytest.mark.parametrize("form", mm.FORMS)
def test_covering_gaps_rejects_a_table_with_a_row_removed(form):
    rows = mm.ROWS[form]
    for i in range(len(rows)):
        assert mm.covering_gaps(form, rows[:i] + rows[i + 1:]), i
    assert mm.covering_gaps(form, rows + rows[:1])  # too many rows
    alien = rows[0]._replace(dt="softplus" if form != "wide" else "gelu")
    assert mm.covering_gaps(form, rows[1:] + (alien,))


def test_cases_cover_every_form_and_geometry_within_the_cost_bound():
    ids = [c.id for c in mm.CASES]
    assert len(set(ids)) == len(ids)
    for form in mm.FORMS:
        for geo in mm.GEOMETRIES[form]:
            got = [c.row for c in mm.CASES if c.form == form and c.geo == geo and not c.gapped]
            assert tuple(got) == mm.ROWS[form], (form, geo)
    assert sorted(c.form for c in mm.CASES if c.gapped) == ["fused", "split_k", "wide"]
    for c in mm.CASES:
        assert c.ntok <= 1300 and 1 <= c.seqlen <= c.out_len, c.id
        assert c.e % 2 == 0 and c.e <= c.e_pad <= 80 and c.r <= c.r_pad, c.id
    # the geometries the tiling needs: a half-width last split, ten splits, nine waves
    assert any(c.dim % 128 == 64 for c in mm.CASES if c.form == "split_k")
    assert any(c.dim == 1280 and c.r == 40 and c.e == 72 for c in mm.CASES if c.form == "split_k")
    assert any(c.dim == 1152 for c in mm.CASES if c.form == "fused")
    assert {c.batch for c in mm.CASES if c.form == "wide"} == {3, 9}
    assert all((c.batch == 3) == c.row.softplus for c in mm.CASES if c.form == "wide")


# --------------------------------------------------------------------------- sensitivity
FAULTS = ("no_state", "roll_batch", "roll_cols", "no_bias", "reverse_taps")


def _applies(fault, case):
    row = case.row
    if fault in ("no_state", "roll_cols"):
        return row.state_in != "none" and row.width >= 2
    if fault == "roll_batch":
        return row.state_in != "none" and row.width >= 2 and case.batch >= 2
    if fault == "no_bias":
        return row.bias
    return row.width >= 2  # reverse_taps


def _faulted(fault, i):
    if fault == "no_state":
        return mm.mid_ref64(i.x, i.cw, i.cb, None)[0]
    if fault == "roll_batch":
        return mm.mid_ref64(i.x, i.cw, i.cb, torch.roll(i.state, 1, 0))[0]
    if fault == "roll_cols":
        return mm.mid_ref64(i.x, i.cw, i.cb, torch.roll(i.state, 1, 2))[0]
    if fault == "no_bias":
        return mm.mid_ref64(i.x, i.cw, None, i.state)[0]
    return mm.mid_ref64(i.x, torch.flip(i.cw, dims=[1]), i.cb, i.state)[0]


def _sensitivity_cases():
    """Per (form, geometry, fault) the first table row the fault can affect (a state fault
    needs a state and a width >= 2, a batch roll two sequences, ...); a geometry of batch 1
    has no batch roll."""
    out = []
    for form in mm.FORMS:
        for geo in mm.GEOMETRIES[form]:
            for fault in FAULTS:
                hit = [c for c in mm.CASES if c.form == form and c.geo == geo and not c.gapped
                       and _applies(fault, c)]
                if hit:
                    out.append(pytest.param(hit[0], fault, id=f"{hit[0].id}-{fault}"))
                else:
                    assert fault == "roll_batch" and geo.batch == 1, (form, geo, fault)
    return out


@pytest.mark.parametrize("case,fault", _sensitivity_cases())
def test_a_faulted_reference_fails_the_u_comparator(case, fault):
    """The reference recomputed without the state, with the batch's states rolled by one,
    with the state columns rolled, without the bias or with the taps reversed must fail
    the u bound on at least half of the elements the fault can affect: the first
    width - 1 steps for the state faults, every step for the others."""
    i = mm.make_inputs(case)
    L = case.seqlen
    i = i._replace(x=i.x[:, :L])
    ref, _ = mm.mid_ref64(i.x, i.cw, i.cb, i.state)
    bad = mm.mismatch(_faulted(fault, i), ref, mm.TOL_U)
    if fault in ("no_state", "roll_batch", "roll_cols"):
        n = min(L, case.width - 1)
        assert not bad[:, n:].any()
        bad = bad[:, :n]
    assert bad.numel() > 0
    assert bad.float().mean().item() >= 0.5, (case.id, fault, bad.float().mean().item())


@pytest.mark.parametrize("form", mm.FORMS)
def test_faulted_projections_fail_their_comparator(form):
    """At every geometry of the form: x_dbl with the last 64 channels dropped, and dt from
    x_dbl columns 1 .. R instead of 0 .. R - 1, each fail the projection bound on at least
    half of their elements (u and x_dbl rounded to bf16 as the kernels store them)."""
    for geo in mm.GEOMETRIES[form]:
        case = next(c for c in mm.CASES if c.form == form and c.geo == geo
                    and c.row.seqlen == "len")
        i = mm.make_inputs(case)
        u = mm.mid_ref64(i.x, i.cw, i.cb, i.state)[0].float().to(BF16).reshape(-1, case.dim)
        want = mm.proj_ref64(u, i.wx)
        cut = u.clone()
        cut[:, -64:] = 0
        frac = mm.mismatch(mm.proj_ref64(cut, i.wx), want, mm.TOL_PROJ).float().mean().item()
        assert frac >= 0.5, (case.id, "x_dbl", frac)
        xd = want.float().to(BF16)
        R = case.r
        dt = mm.proj_ref64(xd[:, :R], i.wdt)
        frac = mm.mismatch(mm.proj_ref64(xd[:, 1: R + 1], i.wdt), dt, mm.TOL_PROJ).float().mean().item()
        assert frac >= 0.5, (case.id, "dt", frac)


def test_softplus_bias_reaches_both_branches():
    """The activated-dt rows see steps small enough for the kernel's log1p correction
    (e^x below fp32's epsilon) and steps of order one."""
    case = next(c for c in mm.CASES if c.row.dt == "softplus_bias")
    b = mm.make_inputs(case).dt_bias
    assert (b < -17).any() and (b > 0).any()


# --------------------------------------------------------------------------- forms
def test_every_case_reaches_the_form_it_names(tmp_path):
    """tests/host/conv_proj_form_of.cpp feeds every case's plan input to
    vm_conv_proj_plan.h::plan_conv_proj and prints the form: it must be the one the case
    declares (and "none", with the xz-gap reason, for a gapped case of a small form).
    Built as a program of its own under ASan + UBSan, as conv_proj_plan_check.cpp is."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "conv_proj_form_of")
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-I",
                          os.path.join(ROOT, "videomamba_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", "conv_proj_form_of.cpp"),
                          "-o", exe], check=True, timeout=120)
    text = "".join(c.plan_line() + "\n" for c in mm.CASES)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    assert len(got) == len(mm.CASES)
    wrong = [(c.id, g) for c, g in zip(mm.CASES, got) if g[0] != c.planned]
    assert not wrong, wrong[:8]
    kSmallXzGap = 5  # ConvProjWhy's last member
    for c, g in zip(mm.CASES, got):
        assert int(g[1]) == (kSmallXzGap if c.planned == "none" else 0), (c.id, g)
    for form in mm.FORMS:
        assert sum(g[0] == form for g in got) >= len(mm.ROWS[form]) * len(mm.GEOMETRIES[form])
