"""The encoder's two ends against float64 (tests/norm_fwd_matrix.py): ``vm_add_norm_fwd``
through ``kernels.add_norm_raw`` (all 28 kernel instances), ``vm_norm_pool_fwd`` through
``kernels.norm_pool`` (all 8), ``vm_pool_finish_fwd`` on a workspace the test writes, and the
one-token steps ``kernels.selective_state_update`` / ``causal_conv1d_update``.

Bounds: ``|got - ref| <= tol (rms(ref) + |ref|)``, tol 1e-4 for values stored in fp32 and 2e-2
for values stored in bf16 against the reference rounded once (``train_bwd_ref``).
``residual_out`` and the conv state's shift are exact (``torch.equal``); a fast-path add + norm
has the bits of the vector kernel; the pooling sums are held at 1e-4 to the fp64 sums of the
GPU's own stored features.  Every output lies between sentinel margins that must keep their
bits, padding rows of a padded output included.

Shapes (the tables and their coverage assertions are in norm_fwd_matrix.py and
test_norm_fwd_matrix_cpu.py): add + norm rows 1, 3, 4, 5, 257 with every column count either
side of a CPL / VPL step up to 2048, odd ones for the scalar kernel, 32768 / 32769 rows at 8
columns around the write-through switch, and one x that starts 2 bytes off alignment.  Three
cases are larger than 32769 x 8: ``add_rms_bf16_kernel<CPL, true, true>`` without write-through
exists for CPL 2, 3, 4 only above 32768 rows, so 32769 x 260 / 516 / 772 run once each, with
the float64 reference on their first and last 261 rows and the vector kernel's bits on all.
Norm + pool: batch 2, head 0 to 17, groups either side of the 16-row slice, unequal ``bounds``,
``rev_frame``, padded batch strides in and out, and one head-only call (two groups of no rows)
on a workspace of exactly the query's size.  Pool finish: cols 4 to 2048, 1 / 5 / 13
slices, all four modes.  Steps: batch 1 / 3, D 1 / 24 / 257, N 1 / 16 / 17, W 1 to 8.

A head of more than 16 rows (``h17`` cases) left rows [16, head) of the features unwritten
before ``vm_norm_pool_fwd`` gave the head rows slices of their own: those cases fail on the
earlier kernel (worst 38 x the bound) and hold here.

Worst |got - ref| / (tol (rms + |ref|)) of the MI355X run over all cases (1.0 = the bound;
0.000 in a bf16 row: every element is the reference's own rounding):

    stored  y      residual_out  features  sums   x_pool  x_pool(chained)  step out  step state  conv out
    fp32    0.002  exact         0.002     0.003  0.002   0.002            0.011     0.002       0.002
    bf16    0.248  exact         0.164     -      0.000   0.000            0.000     0.000       0.000

(sums are always fp32 and are held to the fp64 sums of the GPU's own features; the conv state's
shift is exact in both dtypes.)
"""

import pytest
import torch

import norm_fwd_matrix as nm
from videomamba_amd import _lib
from videomamba_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = nm.EPS
VM_E_INVALID = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(got, ref64, what, worst):
    """The comparator at the bound of ``got``'s storage dtype; keeps the worst ratio per
    (output, stored dtype)."""
    tol, ref = nm.tol_and_ref(ref64, got.dtype)
    if not ref.any():   # LayerNorm of one column without bias: the bound is 0, so equality
        assert torch.equal(got.cpu().float(), ref), f"{what}: not the exact zeros of the reference"
        r = 0.0
    else:
        r = nm.assert_within_rms(got, ref, tol, what)
    key = (what, "bf16" if got.dtype == BF16 else "fp32")
    worst[key] = max(worst.get(key, 0.0), r)


def _report(tag, cid, worst):
    print(f"\nnorm fwd matrix {tag} {cid}: " +
          " ".join(f"{k}/{d}={v:.3f}" for (k, d), v in sorted(worst.items())))


# --------------------------------------------------------------------------- a. add + norm
def _launch_add_norm(c, ops, ro_kind):
    """One vm_add_norm_fwd launch of case ``c`` with ``residual_out`` of kind ``ro_kind``.
    Returns (y, residual_out or None), both guarded; with "alias" residual_out is the (guarded)
    residual itself."""
    n = c.rows * c.cols
    if c.offset:
        xb = torch.zeros(n + 16, dtype=c.x, device=DEV)
        x = xb[c.offset:c.offset + n].view(c.rows, c.cols)
        x.copy_(ops["x"])
        assert xb.data_ptr() % 16 == 0 and x.data_ptr() % 16 == c.offset * xb.element_size()
    else:
        x = _dev(ops["x"])
    ro, res_t = None, _dev(ops["residual"])
    if ro_kind == "alias":
        ro = nm.Guarded((c.rows, c.cols), c.res, DEV, fill=res_t)
        res_t = ro.t
    elif ro_kind != "none":
        ro = nm.Guarded((c.rows, c.cols), {"fp32": F32, "bf16": BF16}[ro_kind], DEV)
    y = nm.Guarded((c.rows, c.cols), c.out, DEV)
    K.add_norm_raw(x, res_t, _dev(ops["weight"]), _dev(ops["bias"]), y.t,
                   None if ro is None else ro.t, c.rows, c.cols, EPS, c.rms, _stream())
    torch.cuda.synchronize()
    return y, ro


@pytest.mark.parametrize("case", nm.NORM_CASES, ids=lambda c: c.id)
def test_add_norm_forward_matches_float64(case):
    c = case
    ops = nm.norm_inputs(c)
    inst = nm.add_norm_instance(c)
    y, ro = _launch_add_norm(c, ops, c.ro)
    assert y.intact(), "y: sentinel margin overwritten"
    assert ro is None or ro.intact(), "residual_out: sentinel margin overwritten"
    worst = {}
    sel = nm.norm_ref_rows(c)
    ref = nm.add_norm_ref64(ops, c.rms, sel)
    _check(y.t if sel is None else y.t[sel.to(DEV)], ref, "y", worst)
    if ro is not None:
        want = nm.sum_exact(_dev(ops["x"]), _dev(ops["residual"]), ro.t.dtype)
        assert torch.equal(ro.t, want), "residual_out is not the one rounded fp32 add"
        worst[("residual_out", "bf16" if ro.t.dtype == BF16 else "fp32")] = 0.0
    if inst[0] == "fast":
        # the same call with a bf16 residual_out takes add_norm_vec_kernel: same bits
        assert nm.add_norm_instance(c._replace(ro="bf16"))[0] == "vec"
        yv, rov = _launch_add_norm(c, ops, "bf16")
        assert yv.intact() and rov.intact()
        assert torch.equal(y.t, yv.t), "fast path and vector kernel disagree in y"
        if ro is not None:
            assert torch.equal(ro.t.to(BF16), rov.t)
        if sel is not None:   # the rows the reference skipped are held by the vector kernel
            assert torch.equal(rov.t, nm.sum_exact(_dev(ops["x"]), _dev(ops["residual"]), BF16))
    _report("add_norm", c.id + " " + str(inst), worst)


def _raw_add_norm(x, res, w, y, ro, rows, cols, x_code=None, out_code=None, ro_code=None):
    lib = _lib.load()
    code = K.dtype_code
    return lib.vm_add_norm_fwd(
        x.data_ptr(), code(x.dtype) if x_code is None else x_code,
        None if res is None else res.data_ptr(), K.dtype_code_of(res), w.data_ptr(), None,
        y.data_ptr(), code(y.dtype) if out_code is None else out_code,
        None if ro is None else ro.data_ptr(),
        K.dtype_code_of(ro) if ro_code is None else ro_code, rows, cols, EPS, 1, _stream())


@pytest.mark.parametrize("what", ["cols0", "cols2049", "x_dtype", "out_dtype", "ro_dtype",
                                  "rows_negative"])
def test_add_norm_refusals_write_nothing(what):
    rows = 4
    x = torch.randn(rows, 2052, device=DEV).to(BF16)
    res = torch.randn(rows, 2052, device=DEV)
    w = torch.ones(2052, device=DEV)
    y = nm.Guarded((rows, 2052), BF16, DEV)
    ro = nm.Guarded((rows, 2052), F32, DEV)
    kw = {"cols0": dict(cols=0), "cols2049": dict(cols=2049), "x_dtype": dict(cols=8, x_code=7),
          "out_dtype": dict(cols=8, out_code=2), "ro_dtype": dict(cols=8, ro_code=-1),
          "rows_negative": dict(cols=8, rows=-1)}[what]
    rc = _raw_add_norm(x, res, w, y.t, ro.t, kw.pop("rows", rows), **kw)
    torch.cuda.synchronize()
    assert rc == VM_E_INVALID
    assert _lib.load().vm_last_error()
    assert y.unchanged() and ro.unchanged()


def test_add_norm_of_no_rows_is_ok_and_writes_nothing():
    x = torch.randn(4, 8, device=DEV).to(BF16)
    w = torch.ones(8, device=DEV)
    y = nm.Guarded((4, 8), BF16, DEV)
    ro = nm.Guarded((4, 8), F32, DEV)
    assert _raw_add_norm(x, None, w, y.t, ro.t, 0, 8) == 0
    torch.cuda.synchronize()
    assert y.unchanged() and ro.unchanged()


# --------------------------------------------------------------------------- b. norm + pool
def _launch_norm_pool(c, ops):
    """K.norm_pool of case ``c`` into a guarded (B, rows + POOL_OUT_PAD, C) buffer, with a
    guarded workspace of exactly the bytes the library asks for.  Returns (out, ws or None)."""
    out = nm.Guarded((nm.POOL_BATCH, c.rows + nm.POOL_OUT_PAD, c.cols), c.out, DEV,
                     region=lambda t: t[:, :c.rows])
    bounds = None if c.implicit else c.bounds().to(DEV)
    ws = None
    kw = dict(head=c.head, groups=c.groups, group_rows=c.sizes[0][0] if c.implicit else 0,
              bounds=bounds, max_group_rows=c.mgr, sums=c.sums, out=out.full,
              rev_frame=c.rev_frame)
    args = (_dev(ops["x"]), _dev(ops["residual"]), c.rows, _dev(ops["weight"]), _dev(ops["bias"]),
            EPS, c.rms)
    if c.sums:
        nbytes = K.norm_pool_workspace_bytes(nm.POOL_BATCH, c.groups, c.mgr, c.cols)
        assert nbytes == nm.POOL_BATCH * c.groups * c.slices * c.cols * 4
        ws = nm.Guarded((nm.POOL_BATCH, c.groups, c.slices, c.cols), F32, DEV)
        with K.scratch_override(ws.buf[nm.MARGIN:nm.MARGIN + nbytes]):
            feats, got_ws = K.norm_pool(*args, **kw)
        assert got_ws.data_ptr() == ws.t.data_ptr()
    else:
        feats, got_ws = K.norm_pool(*args, **kw)
        assert got_ws is None
    torch.cuda.synchronize()
    assert feats.data_ptr() == out.full.data_ptr()
    return out, ws


@pytest.mark.parametrize("case", nm.POOL_CASES, ids=lambda c: c.id)
def test_norm_pool_matches_float64(case):
    c = case
    ops = nm.pool_inputs(c)
    assert ops["x"].stride(0) > c.rows * c.cols        # in_batch_stride padded
    out, ws = _launch_norm_pool(c, ops)
    assert out.intact(), "out: a sentinel (margin or padding row) was overwritten"
    worst = {}
    _check(out.t, nm.norm_pool_ref64(ops, c), "features", worst)
    if c.sums:
        assert ws.intact(), "workspace: sentinel margin overwritten"
        bounds = c.bounds()
        ref = nm.slice_sums64(out.t, bounds, c.slices)
        worst[("sums", "fp32")] = nm.assert_within_rms(ws.t, ref.float(), 1e-4, "sums")
        dead = ~nm.live_slices(bounds, c.slices)
        assert bool((ws.t.cpu()[dead] == 0).all()), "a slice past its group's end is not zero"
    _report("norm_pool", c.id + " " + str(nm.pool_instance(c)), worst)


def _raw_norm_pool(x, out, rows, cols, head, groups, group_rows, w):
    return _lib.load().vm_norm_pool_fwd(
        x.data_ptr(), K.dtype_code(x.dtype), None, 0, x.stride(0), w.data_ptr(), None, EPS, 1,
        out.data_ptr(), K.dtype_code(out.dtype), out.stride(0), x.shape[0], rows, cols, head,
        groups, group_rows, None, group_rows, 0, None, 0, _stream())


@pytest.mark.parametrize("what", ["head_past_rows", "cols_odd", "cols2052", "groups_do_not_tile"])
def test_norm_pool_refusals_write_nothing(what):
    x = torch.randn(2, 20, 8, device=DEV).to(BF16)
    w = torch.ones(2052, device=DEV)
    out = nm.Guarded((2, 20, 8), BF16, DEV)
    rows, cols, head, groups, gr = {"head_past_rows": (18, 8, 19, 1, 0), "cols_odd": (4, 6, 1, 1, 3),
                                    "cols2052": (1, 2052, 0, 1, 1),
                                    "groups_do_not_tile": (18, 8, 1, 3, 5)}[what]
    assert _raw_norm_pool(x, out.t, rows, cols, head, groups, gr, w) == VM_E_INVALID
    torch.cuda.synchronize()
    assert out.unchanged()


def test_head_only_norm_pool_stays_inside_the_workspace_the_query_sizes():
    """Head rows only (rows = head = 3, two implicit groups of no rows, max_group_rows 0) with
    sums requested: the query sizes one slice per group, the forward fills exactly that region
    with zeros and leaves both margins alone, and the features match float64 as elsewhere.  The
    same call with one byte less of workspace is refused and writes nothing.  (The query used
    to answer 0 bytes here while every group block stored cols floats.)"""
    c = nm.HEAD_ONLY
    assert c.rows == c.head == 3 and c.groups == 2 and c.mgr == 0 and c.slices == 1
    nbytes = K.norm_pool_workspace_bytes(nm.POOL_BATCH, c.groups, 0, c.cols)
    assert nbytes == 4 * nm.POOL_BATCH * c.groups * c.cols
    ops = nm.pool_inputs(c)
    out, ws = _launch_norm_pool(c, ops)
    assert out.intact(), "out: a sentinel (margin or padding row) was overwritten"
    assert ws.intact(), "workspace: sentinel margin overwritten"
    assert ws.nbytes == nbytes and bool((ws.t == 0).all()), "the empty groups' sums are not zeros"
    worst = {}
    _check(out.t, nm.norm_pool_ref64(ops, c), "features", worst)
    _report("norm_pool", c.id + " " + str(nm.pool_instance(c)), worst)
    # one byte less: refused, nothing written
    x, res, w = _dev(ops["x"]), _dev(ops["residual"]), _dev(ops["weight"])
    out2 = nm.Guarded((nm.POOL_BATCH, c.rows, c.cols), c.out, DEV)
    ws2 = nm.Guarded((nm.POOL_BATCH, c.groups, 1, c.cols), F32, DEV)
    lib = _lib.load()
    rc = lib.vm_norm_pool_fwd(
        x.data_ptr(), K.dtype_code(x.dtype), res.data_ptr(), K.dtype_code(res.dtype), x.stride(0),
        w.data_ptr(), None, EPS, 1, out2.t.data_ptr(), K.dtype_code(c.out), out2.t.stride(0),
        nm.POOL_BATCH, c.rows, c.cols, c.head, c.groups, 0, None, 0, 0, ws2.t.data_ptr(),
        nbytes - 1, _stream())
    torch.cuda.synchronize()
    assert rc == VM_E_INVALID and b"workspace smaller" in lib.vm_last_error()
    assert out2.unchanged() and ws2.unchanged()


# --------------------------------------------------------------------------- c. pool finish
def _launch_finish(c, ops, ws_dev):
    """vm_pool_finish_fwd into a guarded x_pool; the CLS rows are row 0 of a (B, 3, C) tensor, so
    their batch stride is 3 cols."""
    cls3 = torch.full((nm.POOL_BATCH, 3, c.cols), 1.0e3, dtype=c.cls, device=DEV)
    cls3[:, 0] = _dev(ops["cls"])
    xp = nm.Guarded((nm.POOL_BATCH, c.prow, c.cols), c.xp, DEV)
    bounds = None if c.implicit else c.bounds().to(DEV)
    lnw, lnb = _dev(ops["lnw"]), _dev(ops["lnb"])
    rc = _lib.load().vm_pool_finish_fwd(
        ws_dev.data_ptr(), nm.POOL_BATCH, c.groups, c.counts[0][0] if c.implicit else 0,
        None if bounds is None else bounds.data_ptr(),
        c.counts[0][0] if c.implicit else c.mgr, cls3.data_ptr(),
        K.dtype_code(c.cls), cls3.stride(0), K.POOL_MODES[c.mode], int(c.keep_temporal),
        None if lnw is None else lnw.data_ptr(), None if lnb is None else lnb.data_ptr(), 1e-6,
        xp.t.data_ptr(), K.dtype_code(c.xp), c.cols, _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().vm_last_error()
    return xp


@pytest.mark.parametrize("case", nm.FINISH_CASES, ids=lambda c: c.id)
def test_pool_finish_matches_float64(case):
    c = case
    ops = nm.finish_inputs(c)
    xp = _launch_finish(c, ops, _dev(ops["ws"]))
    assert xp.intact(), "x_pool: sentinel margin overwritten"
    ref = nm.pool_finish_ref64(ops["ws"], c.counts, ops["cls"], c.mode, c.keep_temporal,
                               ops["lnw"], ops["lnb"], 1e-6, c.xp)
    worst = {}
    _check(xp.t, ref, "x_pool", worst)
    _report("pool_finish", c.id, worst)


@pytest.mark.parametrize("dts", [(BF16, BF16, F32), (F32, F32, F32)], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode", nm.POOL_MODES)
def test_norm_pool_hands_its_sums_to_pool_finish(mode, dts):
    """K.norm_pool's workspace straight into K.pool_finish (unequal groups through bounds,
    per-frame means for two modes): x_pool against the reference finish of the fp64 sums of the
    GPU's own features."""
    keep = mode in ("avg", "cls_cat_avg")
    c = nm.PoolCase(576, *dts, True, False, 1, *nm.POOL_BOUNDS[0][:1], False, nm.POOL_BOUNDS[0][1],
                    0, True)
    ops = nm.pool_inputs(c)
    g = torch.Generator().manual_seed(17)
    lnw, lnb = 1.0 + 0.2 * torch.randn(576, generator=g), 0.2 * torch.randn(576, generator=g)
    bounds = c.bounds()
    feats, ws = K.norm_pool(_dev(ops["x"]), _dev(ops["residual"]), c.rows, _dev(ops["weight"]),
                            None, EPS, True, head=1, groups=c.groups, bounds=bounds.to(DEV),
                            max_group_rows=c.mgr, sums=True)
    xp = K.pool_finish(ws, feats, mode=mode, keep_temporal=keep, groups=c.groups,
                       bounds=bounds.to(DEV), max_group_rows=c.mgr, has_cls=True, lnw32=_dev(lnw),
                       lnb32=_dev(lnb), ln_eps=1e-6)
    torch.cuda.synchronize()
    assert xp.dtype == dts[1]
    ref = nm.pool_finish_ref64(nm.slice_sums64(feats, bounds, c.slices),
                               bounds[:, 1:] - bounds[:, :-1], feats[:, 0].cpu(), mode, keep, lnw,
                               lnb, 1e-6, xp.dtype)
    worst = {}
    _check(xp, ref, "x_pool_chained", worst)
    _report("chain", f"{mode}-{nm._name(dts[0])}", worst)


# --------------------------------------------------------------------------- d. one-token steps
@pytest.mark.parametrize("case", nm.STEP_CASES, ids=lambda c: c.id)
def test_ssm_step_matches_float64(case):
    c = case
    ops = nm.step_inputs(c)
    # the state: a view with padded batch and row strides inside a sentinel buffer
    st = nm.Guarded((c.batch + 1, c.dim + 2, c.n + 3), c.state, DEV,
                    region=lambda t: t[:c.batch, :c.dim, :c.n], fill=_dev(ops["state"]))
    assert st.t.stride() == ((c.dim + 2) * (c.n + 3), c.n + 3, 1)
    d = {k: _dev(v) for k, v in ops.items()}
    out = K.selective_state_update(st.t, d["x"], d["dt"], d["A"], d["B"], d["C"], d["D"], d["z"],
                                   d["dt_bias"], dt_softplus=c.softplus)
    torch.cuda.synchronize()
    assert st.intact(), "state: a sentinel (margin or padding) was overwritten"
    assert out.dtype == c.x and out.shape == (c.batch, c.dim)
    ref_out, ref_state = nm.ssm_step_ref64(softplus=c.softplus, **ops)
    worst = {}
    _check(out, ref_out, "step_out", worst)
    _check(st.t, ref_state, "step_state", worst)
    _report("ssm_step", c.id, worst)


@pytest.mark.parametrize("case", nm.CONV_STEP_CASES, ids=lambda c: c.id)
def test_conv_step_matches_float64(case):
    c = case
    ops = nm.conv_step_inputs(c)
    cs = nm.Guarded((c.batch + 1, c.dim + 2, c.width + 3), c.state, DEV,
                    region=lambda t: t[:c.batch, :c.dim, :c.width], fill=_dev(ops["conv_state"]))
    out = K.causal_conv1d_update(_dev(ops["x"]), cs.t, _dev(ops["weight"]), _dev(ops["bias"]),
                                 activation="silu" if c.silu else None)
    torch.cuda.synchronize()
    assert cs.intact(), "conv_state: a sentinel (margin or padding) was overwritten"
    assert out.dtype == c.x and out.shape == (c.batch, c.dim)
    ref_out, ref_state = nm.conv_step_ref64(ops["x"], ops["conv_state"], ops["weight"],
                                            ops["bias"], c.silu)
    assert torch.equal(cs.t.cpu(), ref_state), "the conv state's shift is not exact"
    worst = {}
    _check(out, ref_out, "conv_step_out", worst)
    _report("conv_step", c.id, worst)
