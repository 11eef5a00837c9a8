"""Keeps the norm forward / norm + pool / one-token step matrix honest without a GPU: the
float64 references against torch and the oracle, the pooling reference against a direct
restatement of the model's pooling, the sentinel helper, the case tables' coverage — every
value of every axis, every kernel instance of the two dispatchers — and the host plan itself
(vm_norm_plan.h): walked by a stand-alone program under ASan + UBSan, and asked for the instance
of every case, which must be the one the tests' own restatement names."""

import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import norm_fwd_matrix as nm
from oracle import videomamba_oracle as orc

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- references
@pytest.mark.parametrize("cols", [1, 63, 576, 2048])
@pytest.mark.parametrize("bias", [False, True])
def test_layer_norm_refs_match_torch_float64(cols, bias):
    c = nm.NormCase(5, cols, False, bias, F32, F32, F32, "fp32")
    ops = nm.norm_inputs(c)
    s = ops["x"].double() + ops["residual"].double()
    want = F.layer_norm(s, (cols,), ops["weight"].double(),
                        ops["bias"].double() if bias else None, nm.EPS)
    torch.testing.assert_close(nm.add_norm_ref64(ops, False), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(
        nm.layer_norm_ref64(s, ops["weight"].double(), ops["bias"].double() if bias else None,
                            nm.EPS), want, rtol=1e-12, atol=1e-12)
    bare = nm.layer_norm_ref64(s, None, None, nm.EPS)
    torch.testing.assert_close(bare, F.layer_norm(s, (cols,), None, None, nm.EPS), rtol=1e-12,
                               atol=1e-12)


@pytest.mark.parametrize("rms", [True, False])
@pytest.mark.parametrize("res", [None, F32, BF16])
@pytest.mark.parametrize("xdt", [F32, BF16])
def test_add_norm_ref_matches_oracle(xdt, res, rms):
    c = nm.NormCase(5, 100, rms, not rms, xdt, xdt, res, "fp32")
    ops = nm.norm_inputs(c)
    y, s = orc.add_norm(ops["x"], ops["residual"], ops["weight"], ops["bias"], nm.EPS, True, True,
                        rms)
    tol, ref = nm.tol_and_ref(nm.add_norm_ref64(ops, rms), xdt)
    nm.assert_within_rms(y, ref, tol, "y")
    assert torch.equal(s, nm.sum_exact(ops["x"], ops["residual"], s.dtype))


def test_add_norm_ref_row_subset_is_the_rows_of_the_whole():
    c = nm.NormCase(40, 260, True, False, BF16, BF16, F32, "fp32")
    ops = nm.norm_inputs(c)
    rows = torch.tensor([0, 3, 39])
    assert torch.equal(nm.add_norm_ref64(ops, True, rows), nm.add_norm_ref64(ops, True)[rows])
    big = next(c for c in nm.NORM_CASES if c.cols == nm.BIG_COLS[0] and c.rows > 32768)
    sel = nm.norm_ref_rows(big)
    assert sel.numel() == nm.BIG_REF_ROWS and int(sel[0]) == 0 and int(sel[-1]) == big.rows - 1
    assert nm.norm_ref_rows(nm.NormCase(257, 2048, True, False, F32, F32, None, "none")) is None


def _model_pool(feats, pool, keep_temporal, frame_of_row, tt, lnw, lnb, eps):
    """The model's pooling (``_torch_pool`` of test_gpu_model.py) restated for float64 features:
    row 0 is the CLS token; the patch rows are averaged over all rows or per frame
    (``frame_of_row``: the frame index of every patch row), then the pool LayerNorm."""
    cls_tok, patch = feats[:, :1], feats[:, 1:]
    ln = lambda v: F.layer_norm(v, (v.shape[-1],), lnw, lnb, eps)  # noqa: E731
    if pool == "cls":
        return ln(cls_tok)
    if keep_temporal:
        Bz, n, C = patch.shape
        sums = torch.zeros(Bz, tt, C, dtype=F64)
        sums.scatter_add_(1, frame_of_row.unsqueeze(-1).expand(-1, -1, C), patch)
        cnt = torch.zeros(Bz, tt, 1, dtype=F64)
        cnt.scatter_add_(1, frame_of_row.unsqueeze(-1), torch.ones(Bz, n, 1, dtype=F64))
        avg = sums / cnt
    else:
        avg = patch.mean(1, keepdim=True)
    if pool == "cls+avg":
        return ln(cls_tok + avg)
    if pool == "cls_cat_avg":
        return ln(torch.cat([cls_tok, avg], 1))
    return ln(avg)


@pytest.mark.parametrize("sizes", [((17, 17, 17), (17, 17, 17)), ((5, 1, 20), (17, 8, 1))])
@pytest.mark.parametrize("keep_temporal", [False, True])
@pytest.mark.parametrize("mode", nm.POOL_MODES)
def test_pool_refs_match_the_models_pooling(mode, keep_temporal, sizes):
    """norm_pool_ref64 -> slice_sums64 -> pool_finish_ref64 on float64 inputs (no rounding
    anywhere) against the model's pooling of the same normalised features."""
    c = nm.PoolCase(64, F32, F32, F32, True, False, 1, sizes, False, 33, 0, True)
    ops = nm.pool_inputs(c)
    feats = nm.norm_pool_ref64(ops, c)
    want_feats = nm.add_norm_ref64({k: (v[:, :c.rows] if k in ("x", "residual") else v)
                                    for k, v in ops.items()}, True)
    assert torch.equal(feats, want_feats)
    bounds = c.bounds()
    ws = nm.slice_sums64(feats, bounds, c.slices)
    g = torch.Generator().manual_seed(2)
    lnw, lnb = torch.randn(64, generator=g).double(), torch.randn(64, generator=g).double()
    got = nm.pool_finish_ref64(ws, bounds[:, 1:] - bounds[:, :-1], feats[:, 0], mode,
                               keep_temporal, lnw, lnb, 1e-6, F64)
    frame = torch.stack([torch.repeat_interleave(torch.arange(3), torch.tensor(s)) for s in sizes])
    want = _model_pool(feats, mode, keep_temporal, frame, 3, lnw, lnb, 1e-6)
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-11)


def test_pool_finish_ref_rounds_the_mean_then_the_cls_sum():
    ws = torch.tensor([[[[1.0, 3.0, 5.0, 7.0]]]])            # one group, one slice, count 3
    cls = torch.tensor([[0.001, 0.002, 0.003, 0.004]])
    got = nm.pool_finish_ref64(ws, [[3]], cls, "cls+avg", False, None, None, 1e-5, BF16)
    v = ((ws[0, 0, 0] / 3).to(BF16).double() + cls[0].double()).to(BF16).double()
    torch.testing.assert_close(got[0, 0], nm.layer_norm_ref64(v, None, None, 1e-5), rtol=0, atol=0)
    cat = nm.pool_finish_ref64(ws, [[3]], cls, "cls_cat_avg", False, None, None, 1e-5, F32)
    torch.testing.assert_close(cat[0, 0], nm.layer_norm_ref64(cls[0].double(), None, None, 1e-5))


@pytest.mark.parametrize("F", [1, 3, 6])
@pytest.mark.parametrize("head", [0, 1])
def test_pool_row_map_reverses_the_frames(head, F):
    rows = head + 12
    idx = nm.pool_row_map(rows, head, F)
    body = torch.arange(head, rows).reshape(12 // F, F)
    assert torch.equal(idx[:head], torch.arange(head))
    assert torch.equal(idx[head:], torch.flip(body, dims=[0]).reshape(-1))
    assert torch.equal(nm.pool_row_map(rows, head, 0), torch.arange(rows))
    # the kernel's own formula
    for r in range(head, rows):
        x = r - head
        assert int(idx[r]) == head + x + (rows - head - F) - 2 * F * (x // F)


def test_slice_sums_are_zero_past_a_short_group():
    c = nm.PoolCase(4, F32, F32, None, True, False, 1, ((5, 1, 20), (17, 8, 1)), False, 33, 0, True)
    feats = torch.ones(2, c.rows, 4, dtype=F64)
    ws = nm.slice_sums64(feats, c.bounds(), c.slices)
    live = nm.live_slices(c.bounds(), c.slices)
    assert ws.shape == (2, 3, 3, 4)
    assert torch.equal(ws[..., 0], torch.tensor([[[5., 0, 0], [1, 0, 0], [16, 4, 0]],
                                                 [[16, 1, 0], [8, 0, 0], [1, 0, 0]]], dtype=F64))
    assert torch.equal(live, ws[..., 0] > 0)


@pytest.mark.parametrize("case", nm.STEP_CASES, ids=lambda c: c.id)
def test_ssm_step_ref_matches_oracle(case):
    """At fp32 the oracle's step is the reference's arithmetic in single precision."""
    if case.x != F32 or case.state != F32:
        case = case._replace(x=F32, state=F32)
    ops = nm.step_inputs(case)
    out64, new64 = nm.ssm_step_ref64(softplus=case.softplus, **ops)
    st = ops["state"].clone()
    out = orc.selective_state_update(st, ops["x"], ops["dt"], ops["A"], ops["B"], ops["C"],
                                     ops["D"], ops["z"], ops["dt_bias"], case.softplus)
    nm.assert_within_rms(out, out64.float(), 1e-4, "out")
    nm.assert_within_rms(st, new64.float(), 1e-4, "state")
    assert torch.isfinite(out64).all() and torch.isfinite(new64).all()


def test_ssm_step_inputs_straddle_the_softplus_branch():
    for case in nm.STEP_CASES:
        if not case.softplus:
            continue
        ops = nm.step_inputs(case)
        arg = ops["dt"].double() + (ops["dt_bias"].double()[None] if case.dt_bias else 0.0)
        assert (arg > nm.SOFTPLUS_THRESHOLD).any() and (arg < nm.SOFTPLUS_THRESHOLD).any(), case.id
        if case.dim > 1:
            assert (arg < 5).any(), case.id


@pytest.mark.parametrize("case", nm.CONV_STEP_CASES, ids=lambda c: c.id)
def test_conv_step_ref_matches_oracle(case):
    ops = nm.conv_step_inputs(case._replace(x=F32, state=F32))
    out64, new = nm.conv_step_ref64(ops["x"], ops["conv_state"], ops["weight"], ops["bias"],
                                    case.silu)
    cs = ops["conv_state"].clone()
    out = orc.causal_conv1d_update(ops["x"], cs, ops["weight"], ops["bias"], silu=case.silu)
    nm.assert_within_rms(out, out64.float(), 1e-4, "out")
    assert torch.equal(cs, new)


def test_conv_step_ref_rounds_x_into_a_bf16_state():
    x = torch.tensor([[1.00390625]])                       # 1 + 2^-8: a bf16 tie, rounds to 1
    cs = torch.tensor([[[0.5, 0.25]]]).to(BF16)
    out, new = nm.conv_step_ref64(x, cs, torch.ones(1, 2), None, False)
    assert new.dtype == BF16 and new.tolist() == [[[0.25, 1.0]]] and float(out) == 1.25


def test_guarded_notices_writes_outside_the_region_only():
    g = nm.Guarded((2, 5, 4), BF16, "cpu", region=lambda t: t[:, :3])
    assert g.t.shape == (2, 3, 4) and g.intact() and g.unchanged()
    g.t.fill_(1.0)
    assert g.intact() and not g.unchanged()
    g.full[1, 4, 0] = 2.0
    assert not g.intact()
    h = nm.Guarded((3,), F32, "cpu", fill=torch.arange(3.0))
    assert h.t.tolist() == [0.0, 1.0, 2.0] and h.intact()
    h.buf[nm.MARGIN + h.nbytes] = 0
    assert not h.intact()
    assert nm.MARGIN // 4 >= 1024 and nm.MARGIN % 16 == 0


# --------------------------------------------------------------------------- coverage
def test_add_norm_cases_reach_every_instance_and_every_axis_value():
    cases = nm.NORM_CASES
    reached = {nm.add_norm_instance(c) for c in cases}
    assert len(nm.ADD_NORM_INSTANCES) == 28 and len(set(nm.ADD_NORM_INSTANCES)) == 28
    assert reached == set(nm.ADD_NORM_INSTANCES), set(nm.ADD_NORM_INSTANCES) ^ reached
    assert {c.rows for c in cases} == set(nm.NORM_ROWS) | set(nm.WT_PAIR)
    assert {c.cols for c in cases} == set(nm.COLS_VEC) | set(nm.COLS_SCALAR) | {576}
    assert {(c.rms, c.bias) for c in cases} == set(nm.NORM_KINDS)
    assert {c.ro for c in cases} == set(nm.NORM_RO)
    for xdt in (F32, BF16):
        sub = [c for c in cases if c.x == xdt]
        assert {c.rows for c in sub} >= set(nm.NORM_ROWS)
        assert {c.cols for c in sub} >= set(nm.COLS_VEC) | set(nm.COLS_SCALAR)
        assert {c.out for c in sub} == {F32, BF16} and {c.res for c in sub} == {None, F32, BF16}
        assert {c.ro for c in sub} == set(nm.NORM_RO)
        assert {(c.rms, c.bias) for c in sub} == set(nm.NORM_KINDS)
        assert {c.ro_dtype for c in sub} == {None, F32, BF16}
        # every form (vec and scalar) sees every residual and every residual_out choice
        for form in ("vec", "scalar"):
            f = [c for c in sub if nm.add_norm_instance(c)[0] == form]
            assert {c.res for c in f} == {None, F32, BF16} and {c.ro for c in f} == set(nm.NORM_RO)
            assert {c.out for c in f} == {F32, BF16} and {c.rms for c in f} == {True, False}
    # the write-through pair at cols 8, the misaligned case on the scalar form
    pair = [c for c in cases if c.cols == 8 and c.rows in nm.WT_PAIR
            and nm.add_norm_instance(c)[0] == "fast"]
    assert {nm.add_norm_instance(c)[4] for c in pair} == {True, False}
    assert nm.MISALIGNED in cases and nm.add_norm_instance(nm.MISALIGNED) == ("scalar", 16)
    assert nm.add_norm_instance(nm.MISALIGNED._replace(offset=0))[0] == "fast"
    # every fast column count with every (residual, residual_out) form
    fast = {(c.cols, c.res, c.ro) for c in cases if nm.add_norm_instance(c)[0] == "fast"}
    assert fast >= {(cols, r, ro) for cols in nm.FAST_COLS for r, ro in nm.FAST_FORMS}
    # nothing above the size cap but the three no-write-through cases
    over = [c for c in cases if c.rows * c.cols > max(32769 * 8, 257 * 2048)]
    assert sorted(c.cols for c in over) == list(nm.BIG_COLS)
    assert all(nm.add_norm_instance(c) == ("fast", i + 2, True, True, False)
               for i, c in enumerate(sorted(over, key=lambda c: c.cols)))
    assert len({c.id for c in cases}) == len(cases)


def test_pool_cases_reach_every_instance_and_every_axis_value():
    cases = nm.POOL_CASES
    reached = {nm.pool_instance(c) for c in cases}
    assert len(nm.POOL_INSTANCES) == 8 and reached == set(nm.POOL_INSTANCES)
    assert {c.cols for c in cases} == set(nm.POOL_COLS)
    assert {(c.x, c.out, c.res) for c in cases} == set(nm.POOL_DTYPES)
    assert {(c.rms, c.bias) for c in cases} == set(nm.NORM_KINDS)
    assert {c.head for c in cases} == set(nm.POOL_HEADS) and max(nm.POOL_HEADS) == nm.HEAD_LIMIT
    impl = [c for c in cases if c.implicit]
    assert {(c.groups, c.sizes[0][0]) for c in impl} >= {(g, gr) for g in nm.POOL_GROUPS
                                                         for gr in nm.POOL_GROUP_ROWS}
    bnd = [c for c in cases if not c.implicit]
    assert {(c.sizes, c.mgr) for c in bnd} == set(nm.POOL_BOUNDS)
    for c in bnd:
        flat = [n for s in c.sizes for n in s]
        assert 1 in flat and len(set(flat)) > 2 and c.mgr > max(flat)
        assert len({sum(s) for s in c.sizes}) == 1
    assert {c.sums for c in cases} == {True, False}
    rev = [c for c in cases if c.rev_frame]
    assert {c.head for c in rev} == {0, 1} and {c.head for c in cases if not c.rev_frame} >= {0, 1}
    assert all((c.rows - c.head) % c.rev_frame == 0 for c in rev)
    assert any(1 < c.rev_frame < c.rows - c.head for c in rev)   # a real permutation
    for kind in ("fast", "generic"):
        sub = [c for c in cases if nm.pool_instance(c)[0] == kind]
        assert {c.head for c in sub} == set(nm.POOL_HEADS), kind
        assert {c.sums for c in sub} == {True, False} and {c.implicit for c in sub} == {True, False}
        assert any(c.rev_frame and c.head == 1 for c in sub) and {c.rms for c in sub} == {True, False}
        # the head rows outnumber every group's slices, with sums requested
        assert any(c.sums and -(-c.head // nm.POOL_RB) > c.slices for c in sub), kind
    for dts in nm.POOL_DTYPES:
        sub = [c for c in cases if (c.x, c.out, c.res) == dts]
        assert {c.cols for c in sub} == set(nm.POOL_COLS) and {c.sums for c in sub} == {True, False}
    assert len({c.id for c in cases}) == len(cases)
    assert max(c.rows * c.cols for c in cases) <= 257 * 2048


def test_finish_cases_cover_every_axis_value():
    cases = nm.FINISH_CASES
    assert {c.cols for c in cases} == set(nm.FINISH_COLS)
    assert {c.slices for c in cases} == set(nm.FINISH_SLICES)
    for xp in (F32, BF16):
        sub = [c for c in cases if c.xp == xp]
        assert {c.mode for c in sub} == set(nm.POOL_MODES) and {c.cols for c in sub} == set(nm.FINISH_COLS)
        assert {c.keep_temporal for c in sub} == {True, False}
        assert {c.implicit for c in sub} == {True, False}
        assert {(c.lnw, c.lnb) for c in sub} == {(a, b) for a in (True, False) for b in (True, False)}
        assert {c.cls for c in sub} == {F32, BF16}
    for mode in nm.POOL_MODES:
        sub = [c for c in cases if c.mode == mode]
        assert {c.cols for c in sub} == set(nm.FINISH_COLS) and {c.slices for c in sub} == set(nm.FINISH_SLICES)
        assert {c.keep_temporal for c in sub} == {True, False} and {c.implicit for c in sub} == {True, False}
    # the four-at-a-time slice loop runs (with a tail and without) and is skipped
    def loop(c):
        P = 1024 // (c.cols // 4)
        nrow = (1 if c.keep_temporal else c.groups) * c.slices
        full, tail = 0, 0
        r = 0
        while r + 3 * P < nrow:
            full, r = full + 1, r + 4 * P
        while r < nrow:
            tail, r = tail + 1, r + P
        return full > 0, tail > 0
    seen = {loop(c) for c in cases if c.mode != "cls"}
    assert seen >= {(True, True), (True, False), (False, True)}
    assert len({c.id for c in cases}) == len(cases)


def test_step_cases_cover_every_axis_value():
    cases = nm.STEP_CASES
    assert {c.batch for c in cases} == set(nm.STEP_BATCH) and {c.dim for c in cases} == set(nm.STEP_DIM)
    assert {c.n for c in cases} == set(nm.STEP_N)
    assert {(c.x, c.state) for c in cases} == set(nm.STEP_DTYPES)
    for k in ("D", "z", "dt_bias", "softplus"):
        assert {getattr(c, k) for c in cases} == {True, False}, k
    for dts in nm.STEP_DTYPES:
        sub = [c for c in cases if (c.x, c.state) == dts]
        assert {c.softplus for c in sub} == {True, False}, dts
        for k in ("D", "z", "dt_bias"):
            assert {getattr(c, k) for c in sub} == {True, False}, (dts, k)
    assert any(c.batch == 3 and c.dim == 257 for c in cases)
    conv = nm.CONV_STEP_CASES
    assert {c.batch for c in conv} == set(nm.STEP_BATCH) and {c.dim for c in conv} == set(nm.STEP_DIM)
    assert {c.width for c in conv} == set(nm.STEP_W)
    for dts in nm.STEP_DTYPES:
        sub = [c for c in conv if (c.x, c.state) == dts]
        assert {c.bias for c in sub} == {True, False} and {c.silu for c in sub} == {True, False}, dts
    for w in nm.STEP_W:
        assert {c.silu for c in conv if c.width == w} == {True, False}, w
    assert len({c.id for c in cases}) == len(cases) and len({c.id for c in conv}) == len(conv)


# --------------------------------------------------------------------------- the host plan
def _host_program(tmp_path, name):
    """tests/host/<name>.cpp built as a program of its own with the host compiler under
    ASan + UBSan; nothing is loaded into Python."""
    rocm_clang = "/opt/rocm/llvm/bin/clang++"
    cxx = [rocm_clang] if os.path.exists(rocm_clang) else \
        [shutil.which("g++") or "g++", "-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / name)
    subprocess.run(cxx + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all", "-I",
                          os.path.join(ROOT, "videomamba_amd", "csrc"),
                          os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe],
                   check=True, timeout=120)
    return exe


def test_norm_fwd_plan_check_program_passes_under_sanitizers(tmp_path):
    """tests/host/norm_fwd_plan_check.cpp walks plan_add_norm, plan_norm_pool and
    plan_pool_finish over their grids and exits non-zero on a cpl / vpl that is not the smallest
    of its family's set, a fast family chosen off its documented conditions, a grid that misses
    rows, part regions that overlap, leave a gap or end off workspace_bytes (max_group_rows == 0
    included), a query that differs from the plan, a refusal out of order or a 2^31 switch at
    another row count."""
    run = subprocess.run([_host_program(tmp_path, "norm_fwd_plan_check")], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout


def test_every_case_reaches_the_instance_the_plan_names(tmp_path):
    """tests/host/norm_fwd_instance_of.cpp feeds every case's plan input to plan_add_norm /
    plan_norm_pool and prints the instance: it must be the one add_norm_instance /
    pool_instance restate, all 28 + 8 instances must appear in the program's own output, and
    the two constants the tables are built around must be the header's."""
    exe = _host_program(tmp_path, "norm_fwd_instance_of")
    pools = nm.POOL_CASES + [nm.HEAD_ONLY]
    text = "0\n" + "".join(c.plan_line() + "\n" for c in nm.NORM_CASES + pools)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [ln.split() for ln in run.stdout.splitlines()]
    assert len(got) == 1 + len(nm.NORM_CASES) + len(pools)
    assert got[0] == ["consts", str(nm.SMALL_STORE_ROWS), str(nm.POOL_RB)]
    norm_got = [(g[0], int(g[1])) + tuple(bool(int(v)) for v in g[2:])
                for g in got[1:1 + len(nm.NORM_CASES)]]
    wrong = [(c.id, g) for c, g in zip(nm.NORM_CASES, norm_got) if g != nm.add_norm_instance(c)]
    assert not wrong, wrong[:8]
    assert set(norm_got) == set(nm.ADD_NORM_INSTANCES) and len(set(norm_got)) == 28
    pool_got = [(g[0], int(g[1]), int(g[2])) for g in got[1 + len(nm.NORM_CASES):]]
    wrong = [(c.id, g) for c, g in zip(pools, pool_got)
             if g != nm.pool_instance(c) + (c.slices,)]
    assert not wrong, wrong[:8]
    assert {g[:2] for g in pool_got} == set(nm.POOL_INSTANCES) and len(nm.POOL_INSTANCES) == 8
    assert pool_got[-1] == ("fast", 1, 1)     # the head-only case: one slice per empty group
