"""Records the arguments every launcher of ``videomamba_amd.kernels`` hands to the C ABI, into
launch_args.json.

    python tests/golden/gen_launch_args.py <commit>

Run at the commit the table is to name (the last one before kernels.py got its one launch
layer).  No device is needed: ``_lib.load()`` is replaced by a :class:`Recorder` that forwards
the pure host queries (``*_bytes``, ``*_fits``, ``*_chunk_steps``, ``*_slice_rows``) to the real
library and writes every other call down instead of launching it, ``kernels._stream`` answers a
constant and ``require_gpu`` nothing, and the operands are small seeded CPU tensors.  Integers
and floats are recorded as they are; a pointer as null, as ``[name, byte offset]`` when it
lies inside a tensor the case named (so a launcher's slicing shows), as ``"stream"``, or as
``"nonnull"`` (a buffer the launcher allocated itself).  tests/test_api_cpu.py replays every
case below against the launchers of the tree it runs in.
"""

import contextlib
import ctypes
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

STREAM = 0x5EED0
QUERY = re.compile(r"(_bytes|_fits|_chunk_steps|_slice_rows|_status)$|^vm_abi_version$|"
                   r"^vm_last_error$")
BF, F32 = torch.bfloat16, torch.float32
CPU = torch.device("cpu")


class Recorder:
    """Stands in for the loaded library: queries go to ``real``, launches into ``calls``."""

    def __init__(self, real, signatures):
        self.real, self.signatures = real, signatures
        self.calls, self.named = [], {}

    def name(self, label, t):
        self.named[label] = t
        return t

    def _pointer(self, p):
        if p is None or p == 0:
            return None
        if p == STREAM:
            return "stream"
        for label, t in self.named.items():
            base = t.untyped_storage().data_ptr()
            if base <= p < base + max(t.untyped_storage().nbytes(), 1):
                return [label, p - base]
        return "nonnull"

    def __getattr__(self, entry):
        if QUERY.search(entry):
            return getattr(self.real, entry)
        types = self.signatures[entry][0]

        def launch(*args):
            assert len(args) == len(types), (entry, len(args), len(types))
            row = []
            for a, ty in zip(args, types):
                if ty is ctypes.c_void_p:
                    row.append(self._pointer(a))
                elif ty is ctypes.c_float:
                    row.append(float(a))
                else:
                    assert isinstance(a, int) and not isinstance(a, bool), (entry, a)
                    row.append(a)
            self.calls.append([entry, row])
            return 0

        return launch


@contextlib.contextmanager
def recording():
    from videomamba_amd import _lib
    from videomamba_amd import kernels as K
    rec = Recorder(_lib.load(), _lib._SIGNATURES)
    saved = _lib.load, K._stream, K.require_gpu
    _lib.load, K._stream, K.require_gpu = (lambda: rec), (lambda t: STREAM), (lambda *a, **k: None)
    try:
        yield rec
    finally:
        _lib.load, K._stream, K.require_gpu = saved


def rnd(*shape, dtype=BF):
    return torch.randn(*shape).to(dtype)


def s2(t):
    return (t.stride(0), t.stride(1)) if t is not None else (0, 0)


def s3(t):
    return (t.stride(0), t.stride(1), t.stride(2)) if t is not None else (0, 0, 0)


def tm(b, ch, l, dtype=BF):
    """A token-major (b, ch, l) view: unit channel stride."""
    return rnd(b, l, ch, dtype=dtype).transpose(1, 2)


def u8(n):
    return torch.zeros(n, dtype=torch.uint8)


# ------------------------------------------------------------------------------- the scans
SEG = dict(b=2, d=64, l=100, n=16, segments=4)  # takes the segmented token-major form


def _scan_operands(rec, K, full, b=2, d=64, l=100, n=16):
    o = dict(u=tm(b, d, l), delta=tm(b, d, l), A=rnd(d, n, dtype=F32), B=tm(b, n, l),
             C=tm(b, n, l), out=tm(b, d, l))
    optional = dict(D=rnd(d, dtype=F32), z=tm(b, d, l), bias=rnd(d, dtype=F32),
                    h0=rnd(b, d, n, dtype=F32), hl=rnd(b, d, n, dtype=F32))
    o.update(optional if full else dict.fromkeys(optional))
    for k, v in o.items():
        if v is not None:
            rec.name(k, v)
    return o


def _scan_raw(K, o, b=2, d=64, l=100, n=16, **kw):
    K.scan_raw(o["u"], s3(o["u"]), o["delta"], s3(o["delta"]), o["A"], o["B"], s3(o["B"]),
               o["C"], s3(o["C"]), o["D"], o["z"], s3(o["z"]), o["bias"], True, o["h0"],
               s2(o["h0"]), o["hl"], s2(o["hl"]), o["out"], s3(o["out"]), l, b, d, l, n,
               K.dtype_code(BF), STREAM, **kw)


def case_scan_segmented(rec, K, options):
    with options.override(scan_segments=SEG["segments"], scan_one_launch=True):
        _scan_raw(K, _scan_operands(rec, K, True))


def case_scan_segmented_plain(rec, K, options):
    with options.override(scan_segments=SEG["segments"], scan_one_launch=True):
        _scan_raw(K, _scan_operands(rec, K, False))


def case_scan_small_sync_override(rec, K, options):
    with options.override(scan_segments=SEG["segments"], scan_one_launch=True), \
            K.sync_override(rec.name("sync_ov", u8(8))):
        _scan_raw(K, _scan_operands(rec, K, True))


def case_scan_overrides(rec, K, options):
    need = K.scan_sync_bytes(SEG["b"], SEG["d"], SEG["l"], SEG["n"], SEG["segments"])
    ws = K.scan_workspace_bytes(SEG["b"], SEG["d"], SEG["l"], SEG["n"], SEG["segments"])
    with options.override(scan_segments=SEG["segments"], scan_one_launch=True), \
            K.sync_override(rec.name("sync_ov", u8(need))), \
            K.scratch_override(rec.name("ws_ov", u8(ws + 64))):
        _scan_raw(K, _scan_operands(rec, K, True))


def case_scan_two_launch(rec, K, options):
    with options.override(scan_segments=SEG["segments"], scan_one_launch=False):
        _scan_raw(K, _scan_operands(rec, K, True))


def case_scan_workspace(rec, K, options):
    ws = K.scan_workspace_bytes(SEG["b"], SEG["d"], SEG["l"], SEG["n"], SEG["segments"])
    with options.override(scan_segments=SEG["segments"], scan_one_launch=True):
        _scan_raw(K, _scan_operands(rec, K, True), workspace=rec.name("ws", u8(ws + 32)))


def case_scan_single_pass(rec, K, options):
    with options.override(scan_segments=1):
        _scan_raw(K, _scan_operands(rec, K, True))


def case_scan_channel_major(rec, K, options):
    b, d, l, n = 2, 8, 24, 16
    o = dict(u=rnd(b, d, l), delta=rnd(b, d, l), A=rnd(d, n, dtype=F32), B=rnd(b, n, l),
             C=rnd(b, n, l), out=rnd(b, d, l), D=rnd(d, dtype=F32), z=rnd(b, d, l), bias=None,
             h0=None, hl=rnd(b, d, n, dtype=F32))
    for k, v in o.items():
        if v is not None:
            rec.name(k, v)
    _scan_raw(K, o, b, d, l, n)


def case_scan_bidir(rec, K, options):
    o = _scan_operands(rec, K, True, b=4)
    pair = (2, rec.name("A_b", rnd(64, 16, dtype=F32)), rec.name("D_b", rnd(64, dtype=F32)),
            rec.name("bias_b", rnd(64, dtype=F32)), rec.name("h_b", rnd(2, 64, 16, dtype=F32)),
            rec.named["h_b"], 25)
    with options.override(scan_segments=SEG["segments"]):
        _scan_raw(K, o, b=4, pair=pair)


def case_scan_bidir_plain(rec, K, options):
    o = _scan_operands(rec, K, False, b=4)
    pair = (2, rec.name("A_b", rnd(64, 16, dtype=F32)), None, None, None, None, 0)
    with options.override(scan_segments=1):
        _scan_raw(K, o, b=4, pair=pair)


def _scan_dtproj(rec, K, full, **kw):
    b, d, l, n, r = 2, 64, 100, 16, 4
    e = r + 2 * n
    o = _scan_operands(rec, K, full)
    xd = rec.name("x_dbl", rnd(b * l, e))
    wdt = rec.name("wdt_pad", rnd(d, 32))
    z = o["z"] if o["z"] is not None else rec.name("z", tm(b, d, l))
    bias = o["bias"] if o["bias"] is not None else rec.name("bias", rnd(d, dtype=F32))
    s_bc = (l * e, 1, e)
    K.scan_dtproj_raw(o["u"], s3(o["u"]), xd, (l * e, e), r, wdt, o["A"], xd[:, r:r + n], s_bc,
                      xd[:, r + n:], s_bc, o["D"], z, s3(z), bias, o["h0"], s2(o["h0"]),
                      o["hl"], s2(o["hl"]), o["out"], s3(o["out"]), l, b, d, l, n, STREAM, **kw)


def case_scan_dtproj(rec, K, options):
    with options.override(scan_segments=SEG["segments"]):
        _scan_dtproj(rec, K, True)


def case_scan_dtproj_plain_workspace(rec, K, options):
    ws = K.scan_workspace_bytes(SEG["b"], SEG["d"], SEG["l"], SEG["n"], SEG["segments"])
    with options.override(scan_segments=SEG["segments"]):
        _scan_dtproj(rec, K, False, workspace=rec.name("ws", u8(ws)))


def _scan_bwd(rec, K, full, **kw):
    b, d, l, n = 2, 64, 40, 16
    o = _scan_operands(rec, K, full, b, d, l, n)
    g = dict(dout=tm(b, d, l), du=tm(b, d, l), ddelta=tm(b, d, l), dB=tm(b, n, l),
             dC=tm(b, n, l), dA=rnd(d, n, dtype=F32))
    optional = dict(dh_last=rnd(b, d, n, dtype=F32), dz=tm(b, d, l), dD=rnd(d, dtype=F32),
                    dbias=rnd(d, dtype=F32), dh0=rnd(b, d, n, dtype=F32))
    g.update(optional if full else dict.fromkeys(optional))
    for k, v in g.items():
        if v is not None:
            rec.name(k, v)
    K.selective_scan_bwd_raw(
        o["u"], s3(o["u"]), o["delta"], s3(o["delta"]), o["A"], o["B"], s3(o["B"]), o["C"],
        s3(o["C"]), o["D"], o["z"], s3(o["z"]), o["bias"], True, o["h0"], s2(o["h0"]),
        g["dout"], s3(g["dout"]), g["dh_last"], s2(g["dh_last"]), g["du"], s3(g["du"]),
        g["ddelta"], s3(g["ddelta"]), g["dz"], s3(g["dz"]), g["dB"], s3(g["dB"]), g["dC"],
        s3(g["dC"]), g["dA"], g["dD"], g["dbias"], g["dh0"], s2(g["dh0"]), b, d, l, n,
        K.dtype_code(BF), STREAM, **kw)


def case_scan_bwd(rec, K, options):
    _scan_bwd(rec, K, True)


def case_scan_bwd_plain_workspace(rec, K, options):
    ws = K.scan_bwd_workspace_bytes(2, 64, 40, 16)
    _scan_bwd(rec, K, False, workspace=rec.name("ws", u8(ws + 16)))


def case_selective_scan_fn(rec, K, options):
    b, d, l, n = 2, 64, 40, 16
    o = _scan_operands(rec, K, True, b, d, l, n)
    with torch.no_grad():
        K.selective_scan_fn(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"],
                            True, True, o["h0"], last_state_out=o["hl"])
        K.selective_scan_fn(o["u"], o["delta"], o["A"], o["B"], o["C"])
        cm = rec.name("u_cm", rnd(b, d, l))
        K.selective_scan_fn(cm, o["delta"], o["A"], o["B"], o["C"], z=o["z"],
                            return_last_state=True)


def case_selective_scan_fn_grad(rec, K, options):
    b, d, l, n = 2, 64, 40, 16
    for full in (True, False):
        o = _scan_operands(rec, K, full, b, d, l, n)
        for k in ("u", "delta", "A", "B", "C", "D", "z", "bias", "h0"):
            if o[k] is not None:
                o[k].requires_grad_(True)
        out, last = K.selective_scan_fn(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"],
                                        o["z"], o["bias"], True, True, o["h0"])
        if full:
            (out.float().sum() + last.sum()).backward()
        else:
            out.float().sum().backward()


def case_state_update(rec, K, options):
    b, d, n = 3, 16, 16
    state = rec.name("state", rnd(b, d, n, dtype=F32))
    x, dt = rec.name("x", rnd(b, d)), rec.name("dt", rnd(b, d))
    A, Bm, Cm = rnd(d, n, dtype=F32), rec.name("B", rnd(b, n)), rec.name("C", rnd(b, n))
    K.selective_state_update(state, x, dt, A, Bm, Cm, rnd(d, dtype=F32), z=rec.name("z", rnd(b, d)),
                             dt_bias=rnd(d, dtype=F32), dt_softplus=True)
    K.selective_state_update(rec.name("state16", rnd(b, d, n)), x, dt, A, Bm, Cm)


# ------------------------------------------------------------------------------- the convs
def _conv_operands(rec, full, b=2, d=64, l=24, w=4):
    o = dict(x=tm(b, d, l), w32=rnd(d, w, dtype=F32), out=tm(b, d, l))
    optional = dict(b32=rnd(d, dtype=F32), cs_in=rnd(b, d, w), cs_out=rnd(b, d, w, dtype=F32))
    o.update(optional if full else dict.fromkeys(optional))
    for k, v in o.items():
        if v is not None:
            rec.name(k, v)
    return o


def case_conv(rec, K, options):
    b, d, l, w = 2, 64, 24, 4
    for full in (True, False):
        o = _conv_operands(rec, full)
        K.conv_raw(o["x"], s3(o["x"]), o["w32"], o["b32"], o["cs_in"], s2(o["cs_in"]),
                   o["cs_out"], s2(o["cs_out"]), o["out"], s3(o["out"]), l, b, d, l - 3, w,
                   full, K.dtype_code(BF), STREAM)


def case_conv_bwd(rec, K, options):
    b, d, l, w = 2, 64, 24, 4
    for full in (True, False):
        o = _conv_operands(rec, full)
        dout, dx = rec.name("dout", tm(b, d, l)), rec.name("dx", tm(b, d, l))
        dcs = rec.name("dcs", rnd(b, d, w, dtype=F32)) if full else None
        dw = rec.name("dw", rnd(d, w, dtype=F32))
        db = rec.name("db", rnd(d, dtype=F32)) if full else None
        ws = None if full else rec.name("ws", u8(K.conv_bwd_workspace_bytes(b, d, l, w) + 8))
        K.conv_bwd_raw(o["x"], s3(o["x"]), o["w32"], o["b32"], o["cs_in"], s2(o["cs_in"]), dout,
                       s3(dout), dx, s3(dx), dcs, s2(dcs), dw, db, b, d, l, w, full,
                       K.dtype_code(BF), STREAM, workspace=ws)


def case_causal_conv1d_fn(rec, K, options):
    b, d, l, w = 2, 64, 24, 4
    x, wt = rec.name("x", tm(b, d, l)), rec.name("w", rnd(d, w, dtype=F32))
    bias, cs = rec.name("b", rnd(d, dtype=F32)), rec.name("cs", rnd(b, d, w))
    with torch.no_grad():
        K.causal_conv1d_fn(x, wt, bias, "silu", conv_state=cs, return_conv_state=True)
        K.causal_conv1d_fn(x, wt.view(d, 1, w))
        K.causal_conv1d_fn(rec.name("x_cm", rnd(b, d, l)), wt, None, None, return_conv_state=True)
        K.causal_conv1d_update(rec.name("x1", rnd(b, d)), cs, wt, bias, "silu")
        K.causal_conv1d_update(rec.named["x1"], rec.name("cs32", rnd(b, d, w, dtype=F32)), wt)


def case_causal_conv1d_fn_grad(rec, K, options):
    b, d, l, w = 2, 64, 24, 4
    x, wt = rec.name("x", tm(b, d, l)).requires_grad_(True), rec.name("w", rnd(d, w, dtype=F32))
    bias, cs = rec.name("b", rnd(d, dtype=F32)), rec.name("cs", rnd(b, d, w))
    wt.requires_grad_(True), bias.requires_grad_(True), cs.requires_grad_(True)
    out, new = K.causal_conv1d_fn(x, wt, bias, "silu", conv_state=cs, return_conv_state=True)
    (out.float().sum() + new.float().sum()).backward()
    K.causal_conv1d_fn(x, wt).float().sum().backward()


# ------------------------------------------------------------------------------- mixer middle
def _conv_proj_operands(rec, full, b=2, lp=24, d=128, n=16, r=4, w=4):
    e = r + 2 * n
    o = dict(xz=rnd(b * lp, 2 * d), cw=rnd(d, w, dtype=F32), wx_pad=rnd((e + 15) // 16 * 16, d),
             wdt_pad=rnd(d, 32), u=rnd(b * lp, d), x_dbl=rnd(b * lp, e), dt=rnd(b * lp, d))
    optional = dict(cb=rnd(d, dtype=F32), cs_in=rnd(b, d, w), cs_out=rnd(b, d, w))
    o.update(optional if full else dict.fromkeys(optional))
    for k, v in o.items():
        if v is not None:
            rec.name(k, v)
    return o, e


def case_conv_proj(rec, K, options):
    b, lp, d, r, w = 2, 24, 128, 4, 4
    o, e = _conv_proj_operands(rec, True)
    K.conv_proj_raw(o["xz"], (lp * 2 * d, 2 * d), o["cw"], o["cb"], o["cs_in"], s2(o["cs_in"]),
                    o["cs_out"], s2(o["cs_out"]), o["wx_pad"], e, o["wdt_pad"], r, o["u"],
                    (lp * d, d), o["x_dbl"], (lp * e, e), o["dt"], (lp * d, d), lp, b, d, lp - 3,
                    w, STREAM, dt_bias32=rec.name("dt_bias", rnd(d, dtype=F32)), dt_softplus=True)
    o, e = _conv_proj_operands(rec, False)
    with K.scratch_override(rec.name("ws_ov", u8(K.conv_proj_workspace_bytes(b, lp, d, e) + 8))):
        K.conv_proj_raw(o["xz"], (lp * 2 * d, 2 * d), o["cw"], o["cb"], o["cs_in"],
                        s2(o["cs_in"]), o["cs_out"], s2(o["cs_out"]), o["wx_pad"], e, None, r,
                        o["u"], (lp * d, d), o["x_dbl"], (lp * e, e), None, (lp * d, d), lp, b, d,
                        lp, w, STREAM)


def case_in_proj_conv_proj(rec, K, options):
    b, lp, d, r, w, c = 1, 64, 128, 4, 4, 64
    for full in (True, False):
        o, e = _conv_proj_operands(rec, full, b, lp)
        hn, w_in = rec.name("hn", rnd(b * lp, c)), rec.name("w_in", rnd(2 * d, c))
        K.in_proj_conv_proj_raw(hn, w_in, o["xz"][:, d:], o["cw"], o["cb"], o["cs_in"],
                                s2(o["cs_in"]), o["cs_out"], s2(o["cs_out"]), o["wx_pad"], e,
                                o["wdt_pad"], r, o["u"], o["x_dbl"], o["dt"] if full else None,
                                lp, b, d, lp - 1, w, STREAM)


def case_conv_proj_cm(rec, K, options):
    b, lp, d, n, r, w = 2, 24, 128, 16, 4, 4
    e, cols = r + 2 * n, b * lp
    for full in (True, False):
        o, _ = _conv_proj_operands(rec, full)
        xz, u = rec.name("xz", rnd(2 * d, cols)), rec.name("u", rnd(d, cols))
        xd, dt = rec.name("x_dbl", rnd(e, cols)), rec.name("dt", rnd(d, cols))
        K.conv_proj_cm_raw(xz, cols, o["cw"], o["cb"], o["cs_in"], s2(o["cs_in"]), o["cs_out"],
                           s2(o["cs_out"]), o["wx_pad"], e, o["wdt_pad"], r, u, cols, xd, cols,
                           dt, cols, lp, b, d, lp - 2, w, STREAM)


# ------------------------------------------------------------------------------- norms, pool
def case_add_norm(rec, K, options):
    rows, cols = 6, 48
    x, res = rec.name("x", rnd(rows, cols)), rec.name("res", rnd(rows, cols, dtype=F32))
    w32, b32 = rec.name("w32", rnd(cols, dtype=F32)), rec.name("b32", rnd(cols, dtype=F32))
    y, ro = rec.name("y", rnd(rows, cols)), rec.name("ro", rnd(rows, cols, dtype=F32))
    K.add_norm_raw(x, res, w32, b32, y, ro, rows, cols, 1e-5, False, STREAM)
    K.add_norm_raw(x, None, w32, None, y, None, rows, cols, 1e-6, True, STREAM)


def case_add_norm_bwd(rec, K, options):
    rows, cols = 6, 48
    s, dy = rec.name("s", rnd(rows, cols, dtype=F32)), rec.name("dy", rnd(rows, cols))
    w32, b32 = rec.name("w32", rnd(cols, dtype=F32)), rec.name("b32", rnd(cols, dtype=F32))
    dro, dx = rec.name("dres_out", rnd(rows, cols, dtype=F32)), rec.name("dx", rnd(rows, cols))
    dres = rec.name("dres", rnd(rows, cols, dtype=F32))
    dw, db = rec.name("dw", rnd(cols, dtype=F32)), rec.name("db", rnd(cols, dtype=F32))
    K.add_norm_bwd_raw(s, w32, b32, dy, dro, dx, dres, dw, db, rows, cols, 1e-5, False, STREAM)
    ws = rec.name("ws", u8(K.add_norm_bwd_workspace_bytes(rows, cols) + 8))
    K.add_norm_bwd_raw(s, w32, None, dy, None, dx, None, dw, None, rows, cols, 1e-6, True, STREAM,
                       workspace=ws)


class _Owner:
    pass


def case_norm_fns(rec, K, options):
    x, res = rec.name("x", rnd(2, 3, 48)), rec.name("res", rnd(2, 3, 48, dtype=F32))
    w, b = rec.name("w", rnd(48, dtype=F32)), rec.name("b", rnd(48, dtype=F32))
    with torch.no_grad():
        K.rms_norm_fn(x, w, None, eps=1e-5)
        K.layer_norm_fn(x, w, b, residual=res, prenorm=True, residual_in_fp32=True, eps=1e-6)
        K.layer_norm_fn(x[:, :, :32], w[:32], None, prenorm=True, is_rms_norm=True)
        K._norm(x, w, b, res, True, True, 1e-5, False, out=rec.name("y", rnd(2, 3, 48)),
                residual_out=rec.name("ro", rnd(2, 3, 48, dtype=F32)), owner=_Owner())


def case_norm_fns_grad(rec, K, options):
    x, res = rec.name("x", rnd(2, 3, 48)), rec.name("res", rnd(2, 3, 48, dtype=F32))
    w, b = rec.name("w", rnd(48, dtype=F32)), rec.name("b", rnd(48, dtype=F32))
    for t in (x, res, w, b):
        t.requires_grad_(True)
    y, s = K.layer_norm_fn(x, w, b, residual=res, prenorm=True, eps=1e-6)
    (y.float().sum() + s.sum()).backward()
    K.rms_norm_fn(x, w, None, eps=1e-5).float().sum().backward()


def case_norm_pool(rec, K, options):
    b, lp, c = 2, 16, 32
    h, res = rec.name("h", rnd(b, lp, c)), rec.name("res", rnd(b, lp, c, dtype=F32))
    w32, b32 = rec.name("w32", rnd(c, dtype=F32)), rec.name("b32", rnd(c, dtype=F32))
    feats, ws = K.norm_pool(h, res, 13, w32, b32, 1e-5, False, head=1, groups=3, group_rows=4,
                            sums=True)
    K.pool_finish(ws, rec.name("feats", feats), mode="cls+avg", keep_temporal=True, groups=3,
                  group_rows=4, has_cls=True, lnw32=w32, lnb32=b32, ln_eps=1e-5)
    K.norm_pool(h, None, 12, w32, None, 1e-6, True, head=0, groups=1, group_rows=12,
                out=rec.name("out", rnd(b, lp, c)), rev_frame=4)
    bounds = rec.name("bounds", torch.tensor([[1, 5, 13], [1, 9, 13]], dtype=torch.int32))
    with K.scratch_override(rec.name("ws_ov", u8(K.norm_pool_workspace_bytes(b, 2, 8, c) + 8))):
        feats, ws = K.norm_pool(h, None, 13, w32, None, 1e-6, True, head=1, groups=2,
                                bounds=bounds, max_group_rows=8, sums=True)
    K.pool_finish(ws, rec.name("feats", feats), mode="avg", keep_temporal=False, groups=2,
                  bounds=bounds, max_group_rows=8, has_cls=False, lnw32=None, lnb32=None,
                  ln_eps=1e-6)


# ------------------------------------------------------------------------------- the GEMMs
def case_linear(rec, K, options):
    m, n, k = 24, 64, 64
    x, w = rec.name("x", rnd(m, k)), rec.name("w", rnd(n, k))
    K.linear(x, w)
    out = rec.name("out", rnd(m, 2 * n))
    K.linear(x, w, rec.name("b32", rnd(n, dtype=F32)), out=out[:, n:], form="dma")
    K.linear(x[:, :32], w[:, 32:], form="persistent")


def case_linear_add_norm(rec, K, options):
    m, n, k = 24, 64, 128
    x, w = rec.name("x", rnd(m, k)), rec.name("w", rnd(n, k))
    res, nw = rec.name("res", rnd(m, n, dtype=F32)), rec.name("nw", rnd(n, dtype=F32))
    hn = rec.name("hn", rnd(m, n))
    K.linear_add_norm(x, w, res, nw, 1e-5, hn)
    with K.counter_override(rec.name("cnt_ov", u8(K.linear_add_norm_counter_bytes(m) + 8))):
        K.linear_add_norm(x, w, res, nw, 1e-6, hn, h=rec.name("h", rnd(m, n)))


def case_linear_bwd(rec, K, options):
    m, n, k = 24, 64, 128
    dy, x = rec.name("dy", rnd(m, 2 * n)), rec.name("x", rnd(m, k))
    dw = rec.name("dw", rnd(n, k, dtype=F32))
    K.linear_wgrad_raw(dy[:, n:], x, dw, m, n, k, STREAM)
    ws = rec.name("ws", u8(max(K.linear_wgrad_workspace_bytes(m, n, k), 8) + 24))
    K.linear_wgrad_raw(dy[:, :n], x, rec.name("dw16", rnd(n, k)), m, n, k, STREAM, workspace=ws)
    wT = rec.name("wT", rnd(k, n))
    K.linear_dgrad(dy[:, :n], wT)
    K.linear_dgrad(dy[:, n:], wT, out=rec.name("dx", rnd(m, k)))


def case_linear_autograd(rec, K, options):
    m, n, k = 24, 64, 128
    x = rec.name("x", rnd(m, k)).requires_grad_(True)
    w = rec.name("w", rnd(n, k)).requires_grad_(True)
    K._Linear.apply(x, w).float().sum().backward()


# ------------------------------------------------------------------------------- patch embed
def case_patch_embed(rec, K, options):
    b, cin, t, hw, p, c = 2, 3, 2, 8, 4, 16
    video = rec.name("video", rnd(b, cin, t, hw, hw))
    w, bias = rec.name("w", rnd(c, cin, 1, p, p)), rec.name("bias", rnd(c))
    spos, tpos = rec.name("spos", rnd(4, c)), rec.name("tpos", rnd(t, c))
    rows = 1 + t * 4 + 3
    out = rec.name("out", rnd(b, rows, c))
    K.patch_embed(video, w, bias, spos, tpos, out, 1, rows * c, cls=rec.name("cls", rnd(1, 1, c)),
                  cls_pos=rec.name("cls_pos", rnd(1, 1, c)), pad_rows=3,
                  bias32=rec.name("bias32", bias.float()))
    K.patch_embed(video.float(), w, bias, spos, tpos, out, 0, rows * c)


CASES = [v for k, v in list(globals().items()) if k.startswith("case_")]
# every entry of the ABI that is no host query, but the form-less GEMM entry Python never calls
NOT_LAUNCHED = {"vm_linear_fwd"}


def launched_entries():
    from videomamba_amd import _lib
    return {e for e in _lib._SIGNATURES if not QUERY.search(e)} - NOT_LAUNCHED


def run_case(case):
    from videomamba_amd import kernels as K
    from videomamba_amd import options
    torch.manual_seed(0)
    with recording() as rec:
        case(rec, K, options)
    return rec.calls


def main():
    commit = sys.argv[1]
    seen, launches = set(), 0
    with open(os.path.join(HERE, "launch_args.json"), "w") as f:
        f.write("{\n")
        f.write(f' "commit": {json.dumps(commit)},\n')
        f.write(' "note": "what every launcher of kernels.py passed to the C ABI in the tree at '
                '`commit` (gen_launch_args.py): per case, [entry, arguments] of each launch",\n')
        f.write(' "cases": {\n')
        blocks = []
        for case in CASES:
            calls = run_case(case)
            seen.update(c[0] for c in calls)
            launches += len(calls)
            print(case.__name__, len(calls), "launches")
            rows = ",\n".join("   " + json.dumps(c, separators=(",", ":")) for c in calls)
            blocks.append(f'  "{case.__name__}": [\n{rows}\n  ]')
        f.write(",\n".join(blocks))
        f.write("\n },\n")
        f.write(f' "launches": {launches}\n')
        f.write("}\n")
    missing = launched_entries() - seen
    assert not missing, f"no case launches {sorted(missing)}"
    print(launches, "launches of", len(seen), "entries")


if __name__ == "__main__":
    main()
