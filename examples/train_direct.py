#!/usr/bin/env python3
"""The scripts' training loop on the MI355X-native path, end to end:

    npz dataset -> ResidentDataset/ResidentLoader (batches formed on the device)
                -> ODE_Model / DAE_Model (fused integrator; direct_encode variants with the row kernels)
                -> the script's loss on the fused loss kernel (--loss: the scripts' `Loss_func`, line 49) -> fused backward kernels -> Adam
                -> evaluation (the scripts' per-sample, per-dimension table on the fused kernel) -> TorchScript export (save_model)

It is the body of neural_00_ODE_01_no_encode.py:339-400 / neural_01_DAE_01_no_encode.py:405-470 without the logging,
plotting and replay-buffer bookkeeping.  With --synthetic it writes a small dataset in the scripts' npz format first
(SURVEY.md App. C), so it runs anywhere a GPU and the built library are present:

    python examples/train_direct.py --model ode01 --synthetic --epochs 3
    python examples/train_direct.py --model dae02 --train-data training.npz --test-data testing.npz --solver euler
    python examples/train_direct.py --model dae02 --synthetic --loss huber --loss-param 0.05
    python examples/train_direct.py --model dae01 --synthetic --scattered-events      # every sample's fault at its own step
    python examples/train_direct.py --model dae01 --synthetic --segment 25            # multiple shooting: restart from the data every 25 steps
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from py_psnode_amd import datapath, loss as L, models  # noqa: E402
from py_psnode_amd import neural_dae as nd  # noqa: E402
from py_psnode_amd.neural_dae.neural_base import DAE_Curves_Sample, ODE_Curves_Sample  # noqa: E402

HIDDEN = {"ode01": 64, "ode02": 16, "dae01": 64, "dae02": 64}      # what the scripts ship with (their debug override)


def write_synthetic(path, n, T, dae, seed, scattered=False):
    """Damped oscillators driven by a piecewise-constant input: enough structure for the loss to go down.  scattered: every sample's
    input steps at a grid point drawn on its own (between T / 4 and 3 T / 4) instead of at T / 2 for all -- the dataset a model whose event
    object is per-trajectory is for."""
    r = np.random.default_rng(seed)
    t = np.tile((np.arange(T, dtype=np.float32) * 0.01).reshape(1, T, 1), (n, 1, 1))
    z = np.repeat(r.standard_normal((n, 1, 2)).astype(np.float32) * 0.3, T, axis=1)
    k = r.integers(T // 4, max(3 * T // 4, T // 4 + 1), n) if scattered else np.full(n, T // 2)          # the fault step of each sample
    z += np.float32(0.2) * (np.arange(T).reshape(1, T, 1) >= k.reshape(n, 1, 1)).astype(np.float32)
    at = lambda a: a[np.arange(n), k][:, None].copy()          # [n, 1, D]: row k[s] of sample s
    w = 2.0 + r.random((n, 1, 8)).astype(np.float32) * 3.0
    ph = r.random((n, 1, 8)).astype(np.float32) * 6.28
    x = (0.3 * np.exp(-0.5 * t) * np.sin(w * t + ph) + 0.1 * z.sum(-1, keepdims=True)).astype(np.float32)
    d = dict(name=np.array([[f"x{k}", "pu"] for k in range(8)], dtype=object), t=t, x=x, z=z,
             event_t=at(t) if scattered else np.full((n, 1, 1), 0.01 * (T // 2), dtype=np.float32), z_jump=at(z))
    if dae:
        v = (0.5 * z + 0.05 * r.standard_normal((n, T, 2))).astype(np.float32)
        d.update(v=v, i=(x[:, :, :2] * 0.5 + v * 0.2).astype(np.float32), v_jump=at(v),
                 mask=np.ones((n, T, 1), dtype=np.float32))
    np.savez(path, **d)


def build(model, solver, segment=None):
    s = {"euler": nd.Euler, "midpoint": nd.Midpoint, "rk4": nd.RK4}[solver](segment=segment)
    H = HIDDEN[model]
    if model.startswith("ode"):
        return models.ODE_Model(8, 2, H, direct_encode=model.endswith("02"), solver=s)
    return models.DAE_Model(8, 2, 2, 2, H, direct_encode=model.endswith("02"), solver=s)


def step_loss(model_name, model, batch, loss_func=None):
    """forward + THAT script's training loss -- the four differ (py_psnode_amd/loss.py): ODE_01 masked term only
    (neural_00_ODE_01_no_encode.py:353-355), ODE_02 + x0 term + reconstruction (neural_00_ODE_02_direct_encode.py:267-270),
    DAE_01 with the 9x extra weight on x column 1 (neural_01_DAE_01_no_encode.py:414-419), DAE_02 without it and with both
    reconstruction terms (neural_01_DAE_02_direct_encode.py:359-365)."""
    if model_name.startswith("ode"):
        t, x, z, event_t, z_jump, mask = batch
        out = model(t=t, x=x, z=z, event_t=event_t, z_jump=z_jump)
        if model_name == "ode01":
            return L.ode01_loss(out, x, mask, loss_func=loss_func)[0]
        return L.ode02_loss(out[0], out[1], x, mask, loss_func=loss_func)[0]
    t, x, z, v, i, event_t, z_jump, v_jump, mask = batch
    out = model(t=t, x=x, z=z, v=v, i=i, event_t=event_t, z_jump=z_jump, v_jump=v_jump)
    if model_name == "dae01":
        return L.dae01_loss(out[0], x, out[1], i, mask, loss_func=loss_func)[0]
    return L.dae02_loss(out[0], out[1], out[2], out[3], x, i, mask, loss_func=loss_func)[0]


@torch.no_grad()
def evaluate(model_name, model, loader, loss_func=None):
    """evalute_model (neural_00_ODE_01_no_encode.py:104-129): the per-sample table
    `torch.sum(Loss_func(x_pred * mask, x * mask, reduction='none'), dim=1)` of every batch, summed over the samples and divided by the
    mask count -> (x_loss_dim_i for every column, x_loss_total).  Always the FREE rollout: a solver that trains with multiple-shooting
    segments (--segment) is evaluated with segment = None, so the test loss is the one every other run reports."""
    dev = loader.dataset.device
    num, den = None, torch.zeros((), device=dev)
    segment, model.solver.segment = model.solver.segment, None
    try:
        return _evaluate(model_name, model, loader, loss_func, dev, num, den)
    finally:
        model.solver.segment = segment


def _evaluate(model_name, model, loader, loss_func, dev, num, den):
    for batch in loader:
        x, mask = batch[1], batch[-1]
        if model_name.startswith("ode"):
            out = model(t=batch[0], x=x, z=batch[2], event_t=batch[3], z_jump=batch[4])
        else:
            out = model(t=batch[0], x=x, z=batch[2], v=batch[3], i=batch[4], event_t=batch[5], z_jump=batch[6], v_jump=batch[7])
        pred = out[0] if isinstance(out, tuple) else out
        table = L.per_sample_loss(pred, x, mask.expand_as(x).contiguous() if mask.shape[-1] not in (1, x.shape[-1]) else mask, loss_func)
        num = table.sum(0) if num is None else num + table.sum(0)
        den += mask.sum()
    dims = (num / den).tolist()
    return dims, float(num.sum() / den)


def report(epoch, dims, total):
    for k, v in enumerate(dims):
        print(f"epoch {epoch}: x_loss_dim_{k} {v:.6e}")
    print(f"epoch {epoch}: test x_loss_total {total:.6e}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="ode01", choices=sorted(HIDDEN))
    ap.add_argument("--solver", default="euler", choices=["euler", "midpoint", "rk4"], help="the scripts hard-code Euler()")
    ap.add_argument("--train-data")
    ap.add_argument("--test-data")
    ap.add_argument("--synthetic", action="store_true", help="write a small synthetic dataset first")
    ap.add_argument("--scattered-events", action="store_true",
                    help="the synthetic dataset draws each sample's fault step on its own, and the model's event object applies the events per "
                         "trajectory (model.event.per_trajectory = True: the generic kernels K0 / K5; ode01 / dae01 -- the latent integrators of "
                         "the direct_encode models have no generic backward at every width)")
    ap.add_argument("--segment", type=int, default=None, metavar="W",
                    help="multiple shooting (default off): every W-th grid point the rollout restarts from the dataset row x[k], free inside a "
                         "segment (solver.segment = W: the generic kernels K0 / K5, one launch each way; training only -- the test loss is always the free rollout's; ode01 / dae01 -- the latent state "
                         "of the direct_encode models is an encoder output, which the restarts cannot read as data)")
    ap.add_argument("--num", type=int, default=320)
    ap.add_argument("--step", type=int, default=201, help="grid points per sample (cut_length)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--loss", default="mse", choices=["mse", "l1", "smooth_l1", "huber"], help="the scripts' Loss_func (line 49 of each)")
    ap.add_argument("--loss-param", type=float, default=None, help="beta of smooth_l1 / delta of huber (torch's default: 1)")
    ap.add_argument("--save", default=None, help="directory for the TorchScript export (save_model)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    dae = args.model.startswith("dae")
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory()
        args.train_data, args.test_data = os.path.join(tmp.name, "training.npz"), os.path.join(tmp.name, "testing.npz")
        write_synthetic(args.train_data, args.num, args.step, dae, 0, args.scattered_events)
        write_synthetic(args.test_data, max(args.num // 4, 8), args.step, dae, 1, args.scattered_events)
    cls = DAE_Curves_Sample if dae else ODE_Curves_Sample
    train = datapath.ResidentDataset(cls(args.train_data, dev, num_sample=args.num, cut_length=args.step), dev)
    test = datapath.ResidentDataset(cls(args.test_data, dev), dev)
    train_loader = datapath.ResidentLoader(train, batch_size=args.batch, shuffle=True)
    test_loader = datapath.ResidentLoader(test, batch_size=max(len(test) // 10, 1), shuffle=False)
    model = build(args.model, args.solver, args.segment).to(dev)
    model.solver.fused = "require"           # fail loudly rather than walk the time loop in Python
    model.event.per_trajectory = args.scattered_events      # a sample jumps where ITS clock meets ITS event time, not where sample 0's does
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    loss_func = L.loss_kind_of(args.loss if args.loss_param is None else (args.loss, args.loss_param))
    dims, total = evaluate(args.model, model, test_loader, loss_func)
    history = [total]
    report(0, dims, total)
    for epoch in range(1, args.epochs + 1):
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        for batch in train_loader:
            opt.zero_grad()
            loss = step_loss(args.model, model, batch, loss_func)
            loss.backward()
            opt.step()
            steps += batch[0].shape[0] * (batch[0].shape[1] - 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        model.eval()
        dims, total = evaluate(args.model, model, test_loader, loss_func)
        history.append(total)
        report(epoch, dims, total)
        print(f"epoch {epoch}: train loss {float(loss.detach()):.6e}  test x_loss_total {history[-1]:.6e}  {steps / dt / 1e6:.1f} M state-steps/s")
    if args.save:
        model.save_model(args.save)
        print("exported:", sorted(os.listdir(args.save)))
    if tmp is not None:
        tmp.cleanup()
    return history


if __name__ == "__main__":
    main()
