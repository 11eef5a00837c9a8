"""The training mixer on the HIP projection GEMMs (``options.train_gemm = "hip"``): one ``Block``
and one mixer at d_model 192 (d_inner 384, the VideoMamba-Ti projections: in_proj 192 -> 768 and
out_proj 384 -> 192, all four GEMM shapes of forward, dgrad and wgrad inside the HIP sets), bf16,
batch 2, L = 24, with and without ``state``, in ``.train()`` mode.  The existing training tests
run d_model 64, whose K = 64 / 128 the HIP GEMM does not take: they stay on the library path
under either option.

Bound: test_gpu_train_model.py's rule for bf16 models — outputs and every gradient (relative
L2 per tensor) within max(1e-2, 3 d_k) of autograd through the fp32 CPU oracle
(``oracle.block_forward`` / ``oracle.mamba_mixer``), d_k being the oracle's own bf16-vs-fp32
distance computed here.  ``train_gemm = "library"`` is held to the same bounds: the two rounded
computations are independent.  d_k and the achieved distance are printed.

Under ``"hip"`` the mixer's xz and output carry the bits of the ``.eval()`` forward's in_proj /
out_proj (``mamba_simple._linear``: the HIP GEMM); under ``"library"`` they are ``F.linear``'s.

Measured on the MI355X (relative L2): hip and library alike 3.5e-5 (new_ssm) - 6.6e-3
(x_proj.weight), each equal to its d_k to two or three digits — the GPU run sits as far from the
fp32 oracle as the oracle's own bf16 run does; the closest to its bound is the stateful block's
dnorm.weight, 5.03e-3 at d_k 4.99e-3: 0.34 of max(1e-2, 3 d_k).  The SGD step: 1.0080 -> 1.0076.
"""

import pytest
import torch
import torch.nn.functional as F

from oracle import videomamba_oracle as orc
from videomamba_amd import kernels as K
from videomamba_amd import mamba_simple as ms
from videomamba_amd import options
from videomamba_amd.videomamba import create_block

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
D, DI, N, W, B, L = 192, 384, 16, 4, 2, 24


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _block():
    torch.manual_seed(7)
    blk = create_block(D, norm_epsilon=EPS, rms_norm=True, residual_in_fp32=True,
                       fused_add_norm=True, layer_idx=0)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for prm in blk.parameters():
            prm.add_(0.02 * torch.randn(prm.shape, generator=g))
    return blk.to(BF16).to(DEV).train()


def _inputs(stateful):
    g = torch.Generator().manual_seed(3)
    ins = {"hidden": torch.randn(B, L, D, generator=g).to(BF16),
           "residual": torch.randn(B, L, D, generator=g)}
    if stateful:
        ins["conv_state"] = torch.randn(B, DI, W, generator=g).to(BF16)
        ins["ssm_state"] = torch.randn(B, DI, N, generator=g)
    gs = {"hidden": torch.randn(B, L, D, generator=g), "residual": torch.randn(B, L, D, generator=g),
          "ssm": torch.randn(B, DI, N, generator=g)}
    return ins, gs


def _oracle(params, ins, gs, dt, mixer_only):
    """Autograd through the CPU oracle in ``dt``: outputs and gradients by name."""
    p = {k: v.detach().cpu().to(dt).requires_grad_(True) for k, v in params.items()}
    lv = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in ins.items()}
    state = (lv["conv_state"], lv["ssm_state"]) if "ssm_state" in lv else None
    if mixer_only:
        res = orc.mamba_mixer(p, "", lv["hidden"], d_state=N, d_conv=W, state=state,
                              return_state=state is not None)
        h, st = res if state is not None else (res, None)
        loss, outs = (h.float() * gs["hidden"]).sum(), {"hidden_out": h}
    else:
        h, r, st = orc.block_forward(p, "", lv["hidden"], lv["residual"], fused=True,
                                     residual_in_fp32=True, is_rms=True, eps=EPS, d_state=N,
                                     d_conv=W, state=state)
        loss = (h.float() * gs["hidden"]).sum() + (r.float() * gs["residual"]).sum()
        outs = {"hidden_out": h, "residual_out": r}
    if st is not None:
        loss = loss + (st[1].float() * gs["ssm"]).sum()
        outs["new_ssm"] = st[1]
    leaves = {**{"d" + k: v for k, v in p.items()}, **{"d" + k: v for k, v in lv.items()}}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return {**outs, **dict(zip(leaves, grads))}


def _check(what, got, ref32, ref_bf):
    assert set(got) == set(ref32), (set(got) ^ set(ref32))
    bad, lines = {}, []
    for k in got:
        e, d = _rel(got[k], ref32[k]), _rel(ref_bf[k], ref32[k])
        bound = max(1e-2, 3.0 * d)
        lines.append(f"{k}={e:.2e}(d={d:.2e})")
        if not e <= bound:
            bad[k] = (e, bound)
    print(f"\n{what}: " + " ".join(lines))
    assert not bad, bad


@pytest.fixture(scope="module")
def references():
    """The oracle's fp32 and bf16 autograd per (mixer_only, stateful): computed once, shared by
    the hip and library runs, never modified."""
    blk = _block()
    out = {}
    for mixer_only in (False, True):
        mod = blk.mixer if mixer_only else blk
        params = {k: v.detach().cpu().float() for k, v in mod.state_dict().items()}
        for stateful in (False, True):
            ins, gs = _inputs(stateful)
            if mixer_only:
                ins.pop("residual")
            ins32 = {k: v.float() for k, v in ins.items()}
            out[mixer_only, stateful] = (_oracle(params, ins32, gs, F32, mixer_only),
                                         _oracle(params, ins, gs, BF16, mixer_only))
    return out


@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "state"])
@pytest.mark.parametrize("mode,mixer_only", [("hip", False), ("hip", True), ("library", False)],
                         ids=["hip-block", "hip-mixer", "library-block"])
def test_training_block_and_mixer_match_the_oracle(references, mode, mixer_only, stateful):
    blk = _block()
    mod = blk.mixer if mixer_only else blk
    ins, gs = _inputs(stateful)
    if mixer_only:
        ins.pop("residual")
    lv = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}
    state = (lv["conv_state"], lv["ssm_state"]) if stateful else None
    with options.override(train_gemm=mode):
        if mixer_only:
            res = mod(lv["hidden"], state=state, return_state=stateful)
            h, st = res if stateful else (res, None)
            r = None
        elif stateful:
            h, r, st = mod(lv["hidden"], lv["residual"], state=state, return_state=True)
        else:
            (h, r), st = mod(lv["hidden"], lv["residual"]), None
        assert h.requires_grad and h.dtype == BF16
        loss = (h.float() * gs["hidden"].to(DEV)).sum()
        got = {"hidden_out": h}
        if r is not None:
            loss = loss + (r.float() * gs["residual"].to(DEV)).sum()
            got["residual_out"] = r
        if st is not None:
            loss = loss + (st[1] * gs["ssm"].to(DEV)).sum()
            got["new_ssm"] = st[1]
        leaves = {**{"d" + k: v for k, v in mod.named_parameters()},
                  **{"d" + k: v for k, v in lv.items()}}
        grads = torch.autograd.grad(loss, list(leaves.values()))
    for (k, leaf), gr in zip(leaves.items(), grads):
        assert gr.shape == leaf.shape and gr.dtype == leaf.dtype, k
        got[k] = gr
    ref32, ref_bf = references[mixer_only, stateful]
    _check(f"{'mixer' if mixer_only else 'block'} {mode} stateful={stateful}", got, ref32, ref_bf)


def _is_hip(fn):
    """Whether the HIP ``Function`` is on the graph below ``fn``."""
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == "_LinearBackward":
            return True
        todo += [g for g, _ in f.next_functions]
    return False


def _record_projections(mixer, hs, mode):
    """The (input, weight, output) of the mixer's two projection calls in training mode."""
    calls = []
    real_fn, real_lin = K.linear_fn, F.linear

    def spy(which):
        def f(x, w, b=None):
            y = which(x, w, b)
            if w is mixer.in_proj.weight or w is mixer.out_proj.weight:
                calls.append((x.detach(), w.detach(), y.detach(), y.grad_fn))
            return y
        return f

    K.linear_fn, ms.F.linear = spy(real_fn), spy(real_lin)
    try:
        with options.override(train_gemm=mode):
            out = mixer(hs)
    finally:
        K.linear_fn, ms.F.linear = real_fn, real_lin
    return out, calls


def test_training_projections_carry_the_inference_bits_under_hip():
    mixer = _block().mixer
    hs = _inputs(False)[0]["hidden"].to(DEV)
    out, calls = _record_projections(mixer, hs, "hip")
    assert [tuple(c[1].shape) for c in calls] == [(2 * DI, D), (D, DI)]
    for x, w, y, fn in calls:
        assert _is_hip(fn)
        with torch.no_grad():
            ref = ms._linear(x.reshape(-1, x.shape[-1]).contiguous(), w)  # the .eval() projection
        assert torch.equal(y.reshape(ref.shape), ref)
    assert torch.equal(out, calls[1][2])
    # the library path: F.linear's bits (and its grad_fn, not the HIP Function's)
    out_l, calls_l = _record_projections(mixer, hs, "library")
    assert len(calls_l) == 2
    for x, w, y, fn in calls_l:
        assert torch.equal(y, F.linear(x, w)) and not _is_hip(fn)
    # the .eval() mixer's output rows use the same out_proj kernel: same shape and dtype
    with torch.no_grad():
        ev = mixer.eval()(hs)
    mixer.train()
    assert ev.shape == out.shape and ev.dtype == out.dtype


def test_one_sgd_step_lowers_the_loss():
    blk = _block()
    ins, _ = _inputs(False)
    x, r = ins["hidden"].to(DEV), ins["residual"].to(DEV)
    g = torch.Generator().manual_seed(4)
    target = torch.randn(B, L, D, generator=g).to(DEV)
    # bf16 parameters: the step has to survive their rounding (half an ulp of a 0.07 weight is
    # 1.4e-4), so the rate is far above what an fp32 model would take
    opt = torch.optim.SGD(blk.parameters(), lr=0.3)
    with options.override(train_gemm="hip"):
        loss0 = F.mse_loss(blk(x, r)[0].float(), target)
        opt.zero_grad()
        loss0.backward()
        for name, prm in blk.named_parameters():
            assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
        opt.step()
        with torch.no_grad():
            loss1 = F.mse_loss(blk(x, r)[0].float(), target)
    print(f"\nSGD step: loss {float(loss0.detach()):.4f} -> {float(loss1):.4f}")
    assert float(loss1) < float(loss0.detach()), (float(loss0.detach()), float(loss1))
