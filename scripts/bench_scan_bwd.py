"""Selective-scan backward microbenchmark at VideoMamba-M / 8 frames geometry (D = 1152,
L = 1569, N = 16, bf16 token-major operands, D / z / bias / softplus on); prints one JSON line.

Times, per batch (default 8 and 32), with device events after a warm-up:
  fwd       the forward call (``kernels.selective_scan_fn`` under ``no_grad``)
  fwd_bwd   the forward + backward pair through the autograd Function
and, at batch 8 only, autograd through a per-step torch-op recurrence on the same device as a
baseline.  Every measurement runs in a child process of its own under a time limit, so a slow
leg cannot hold the device for minutes.

    python scripts/bench_scan_bwd.py [--batches 8 32] [--reps 20] > profiles/scan_bwd_<tag>.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, SEQLEN, NSTATE = 1152, 1569, 16


def _operands(batch, dev, grad):
    import torch
    g = torch.Generator(device="cpu").manual_seed(batch)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    tok = lambda ch, scale=1.0: (scale * rn(batch, SEQLEN, ch)).to(torch.bfloat16).to(dev) \
        .transpose(1, 2).requires_grad_(grad)  # noqa: E731  token-major (b, ch, l) views
    A = (-torch.exp(torch.log(torch.arange(1, NSTATE + 1).float()).repeat(DIM, 1)))
    ops = dict(u=tok(DIM), delta=tok(DIM, 0.5), A=A.to(dev).requires_grad_(grad), B=tok(NSTATE),
               C=tok(NSTATE), D=rn(DIM).to(dev).requires_grad_(grad), z=tok(DIM),
               bias=(rn(DIM) - 3.0).to(dev).requires_grad_(grad))
    dout = rn(batch, SEQLEN, DIM).to(torch.bfloat16).to(dev).transpose(1, 2)
    return ops, dout


def _time(fn, warmup, reps):
    """Per-call device-event times in microseconds."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    us = [1e3 * a.elapsed_time(b) for a, b in pairs]
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1),
                max=round(max(us), 1), mean=round(statistics.fmean(us), 1))


def child_kernel(batch, warmup, reps):
    import torch
    from videomamba_amd import kernels as K
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    ops, dout = _operands(batch, dev, True)
    call = lambda: K.selective_scan_fn(ops["u"], ops["delta"], ops["A"], ops["B"], ops["C"],  # noqa: E731
                                       ops["D"], ops["z"], ops["bias"], True)
    leaves = list(ops.values())

    def fwd():
        with torch.no_grad():
            call()

    def pair():
        torch.autograd.grad(call(), leaves, dout)

    f = _time(fwd, warmup, reps)
    p = _time(pair, warmup, reps)
    return dict(batch=batch, fwd_us=f, fwd_bwd_us=p,
                bwd_us_median=round(p["median"] - f["median"], 1),
                bwd_over_fwd=round((p["median"] - f["median"]) / f["median"], 2),
                workspace_bytes=K.scan_bwd_workspace_bytes(batch, DIM, SEQLEN, NSTATE))


def child_torch(batch, warmup, reps):
    """Autograd through the recurrence written step by step in torch ops (fp32 math on the
    same bf16 operands), forward + backward."""
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    ops, dout = _operands(batch, dev, True)
    leaves = list(ops.values())

    def pair():
        u, dl, z = ops["u"].float(), ops["delta"].float(), ops["z"].float()
        Bm, Cm, A = ops["B"].float(), ops["C"].float(), ops["A"]
        dl = F.softplus(dl + ops["bias"][None, :, None])
        du = dl * u
        h = torch.zeros(batch, DIM, NSTATE, device=dev)
        ys = []
        for t in range(SEQLEN):
            h = torch.exp(dl[:, :, t, None] * A) * h + du[:, :, t, None] * Bm[:, None, :, t]
            ys.append((h * Cm[:, None, :, t]).sum(-1))
        y = (torch.stack(ys, 2) + u * ops["D"][None, :, None]) * F.silu(z)
        torch.autograd.grad(y.to(torch.bfloat16), leaves, dout)

    return dict(batch=batch, fwd_bwd_us=_time(pair, warmup, reps))


def _run_child(mode, batch, a, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
           "--child", mode, "--batch", str(batch), "--reps", str(a.reps),
           "--warmup", str(a.warmup)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        return dict(batch=batch, error=f"exit {run.returncode}", stderr=run.stderr[-400:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-limit", type=int, default=150, help="seconds per kernel child")
    ap.add_argument("--baseline-limit", type=int, default=240, help="seconds for the torch-op child")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--child", choices=["kernel", "torch"])
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        fn = child_kernel if a.child == "kernel" else child_torch
        print(json.dumps(fn(a.batch, a.warmup, a.reps)), flush=True)
        return 0
    out = dict(bench="scan_bwd", dim=DIM, seqlen=SEQLEN, dstate=NSTATE, dtype="bf16",
               layout="token-major", reps=a.reps, warmup=a.warmup, timer="device events",
               results=[])
    failed = False
    for b in a.batches:
        r = _run_child("kernel", b, a, a.kernel_limit)
        out["results"].append(r)
        if "error" in r:  # a faulted or hung leg: start nothing more on the device
            failed = True
            break
    if not failed and not a.no_baseline:
        out["torch_op_baseline"] = _run_child("torch", 8, a, a.baseline_limit)
        base = out["torch_op_baseline"]
        ours = next((r for r in out["results"] if r.get("batch") == 8), None)
        if ours and "error" not in base:
            out["baseline_over_kernel_b8"] = round(
                base["fwd_bwd_us"]["median"] / ours["fwd_bwd_us"]["median"], 1)
        failed = "error" in base
    print(json.dumps(out), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
