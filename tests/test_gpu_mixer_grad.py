"""The Mamba mixer in training mode is differentiable end to end: output, every parameter
gradient, the input gradient and the state gradients against autograd through the CPU oracle
(``oracle.videomamba_oracle.mamba_mixer``) on fp32 copies of the same parameter values.

fp32 model (TF32 off): relative L2 <= 1e-4 — the fp32 oracle's own autograd sits 1.7e-7 to
5.4e-7 from a float64 restatement at these shapes.  bf16 model: relative L2 <= 1e-2 against
the fp32 oracle on the bf16-valued parameters, the project's bf16 relative-norm tolerance —
the oracle's own bf16 autograd sits at 4.5e-4 to 4.5e-3.

An ``.eval()`` mixer under the same call keeps today's behaviour (no graph, bits of the
``no_grad`` output), and one SGD step on the training mixer lowers an MSE loss.
"""

import warnings

import pytest
import torch

from oracle import videomamba_oracle as orc
from videomamba_amd.mamba_simple import Mamba

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-4, BF16: 1e-2}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _mixer(dt):
    torch.manual_seed(11)
    m = Mamba(d_model=64, d_state=16, d_conv=4, expand=2, layer_idx=0)
    with torch.no_grad():
        for prm in m.parameters():
            prm.add_(0.01 * torch.randn_like(prm))
    return m.to(dt).to(DEV).train()


def _oracle_grads(m, x, state, g_out, g_h):
    """Loss <out, g> + <ssm_state_out, g_h> through the oracle in fp32 on the CPU: returns
    out, the new states (or None) and the gradients of the parameters, x and the states."""
    p = {k: v.detach().cpu().float().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.detach().cpu().float().requires_grad_(True)
    leaves = dict(p)
    leaves["x"] = xr
    if state is None:
        out = orc.mamba_mixer(p, "", xr, d_state=16, d_conv=4)
        new = None
        loss = (out * g_out).sum()
    else:
        conv, ssm = (s.detach().cpu().float().requires_grad_(True) for s in state)
        leaves["conv_state"], leaves["ssm_state"] = conv, ssm
        out, new = orc.mamba_mixer(p, "", xr, d_state=16, d_conv=4, state=(conv, ssm),
                                   return_state=True)
        loss = (out * g_out).sum() + (new[1] * g_h).sum()
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return out, new, dict(zip(names, grads))


@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "state"])
@pytest.mark.parametrize("L", [24, 150])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_training_mixer_gradients_match_the_oracle(dt, L, stateful):
    prev = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        m = _mixer(dt)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, L, 64, generator=g).to(dt)
        g_out = torch.randn(2, L, 64, generator=g)
        g_h = torch.randn(2, m.d_inner, 16, generator=g)
        state = None
        if stateful:
            state = (torch.randn(2, m.d_inner, 4, generator=g).to(dt),
                     torch.randn(2, m.d_inner, 16, generator=g))
        ref_out, ref_new, ref = _oracle_grads(m, x, state, g_out, g_h)

        xd = x.to(DEV).requires_grad_(True)
        leaves = dict(m.named_parameters())
        leaves["x"] = xd
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            if stateful:
                conv, ssm = (s.to(DEV).requires_grad_(True) for s in state)
                leaves["conv_state"], leaves["ssm_state"] = conv, ssm
                out, (new_conv, new_ssm) = m(xd, state=(conv, ssm), return_state=True)
                assert new_ssm is not ssm and new_ssm.requires_grad and new_conv.requires_grad
                assert new_ssm.dtype == F32 and new_conv.shape == conv.shape
                loss = (out.float() * g_out.to(DEV)).sum() + (new_ssm * g_h.to(DEV)).sum()
            else:
                out = m(xd)
                loss = (out.float() * g_out.to(DEV)).sum()
        # the differentiable path does not raise the no-autograd warning
        assert not [w for w in caught if "not differentiable" in str(w.message)]
        assert out.requires_grad and out.dtype == dt and out.shape == x.shape
        names = list(leaves)
        grads = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names])))

        tol = TOL[dt]
        worst = {"out": _rel(out, ref_out)}
        if stateful:
            worst["new_ssm"] = _rel(new_ssm, ref_new[1])
            worst["new_conv"] = _rel(new_conv, ref_new[0])
        assert set(grads) == set(ref)
        for k in names:
            assert grads[k].shape == leaves[k].shape and grads[k].dtype == leaves[k].dtype, k
            worst["d" + k] = _rel(grads[k], ref[k])
        print(f"\nmixer grad {dt} L={L} stateful={stateful}: " +
              " ".join(f"{k}={v:.2e}" for k, v in worst.items()))
        bad = {k: v for k, v in worst.items() if not v <= tol}
        assert not bad, (tol, bad)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = prev


def test_eval_mixer_keeps_the_inference_path():
    """.eval() with grad enabled and parameters that require grad: no graph, and the bits of
    the no_grad call (the path every existing caller runs)."""
    m = _mixer(F32).eval()
    x = torch.randn(2, 24, 64, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m(x)
    with torch.no_grad():
        ref = m(x)
    assert not out.requires_grad and torch.equal(out, ref)
    m.train()
    with torch.no_grad():
        assert torch.equal(m(x), ref)  # training mode without autograd: the same path
    assert m(x).requires_grad


def test_one_sgd_step_lowers_the_loss():
    m = _mixer(F32)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 24, 64, generator=g).to(DEV)
    target = torch.randn(2, 24, 64, generator=g).to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    loss0 = torch.nn.functional.mse_loss(m(x), target)
    opt.zero_grad()
    loss0.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    opt.step()
    with torch.no_grad():
        loss1 = torch.nn.functional.mse_loss(m.train()(x), target)
    assert float(loss1) < float(loss0.detach()), (float(loss0.detach()), float(loss1))
