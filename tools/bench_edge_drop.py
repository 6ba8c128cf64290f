#!/usr/bin/env python3
"""Times the interval GNN stack with and without edge dropout, in one process:
  - the batched stack (forward + backward) on the Gowalla-shaped synthetic set (U = 48,653, I = 52,619, 3 intervals x
    600 k edges, d = 64, 2 layers);
  - one per-interval SpMM on a quarter-scale synthetic graph of the roofline workload (250 k x 250 k, 25 M edges).
Each is run three ways, alternated round by round so that all see the same machine state: keep 1.0 (the existing entry,
no dropout), keep 0.5, and keep_threshold = 2^32 - 1 with scale 1 (every edge kept: the cost of the draw alone).
Numbers of different machines or builds are not comparable; run the parent commit's build with --baseline-only on the
same machine for the undropped entry's time there."""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import graph, ops, synthetic      # noqa: E402


def timed(fn, rounds, inner):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e3)
    return out


def report(title, runs, rounds, inner, out):
    times = {name: [] for name, _ in runs}
    for name, fn in runs:                      # warm-up
        timed(fn, 1, 3)
    for _ in range(rounds):                    # alternated
        for name, fn in runs:
            times[name] += timed(fn, 1, inner)
    base = float(np.median(times[runs[0][0]]))
    for name, _ in runs:
        v = times[name]
        line = (f"{title}: {name:<28} median {np.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
                f"ratio to undropped {np.median(v) / base:5.3f}  ({rounds} rounds of {inner})")
        print(line)
        out.append(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--baseline-only", action="store_true", help="time the undropped entries only (a build without the drop entries)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    drops = [] if opt.baseline_only else [("keep 0.5", ops.EdgeDrop(12345, 7, 0.5)),
                                          ("all kept (draw only)", ops.EdgeDrop.raw(12345, 7, 2 ** 32 - 1, 1.0))]

    # ---- the batched stack, Gowalla-shaped
    np.random.seed(100)
    U, I, T, L, d = 48653, 52619, 3, 2, 64
    mats = synthetic.make_trn_mat_time(U, I, [600000] * T)[1]
    pairs = [graph.interval_pair(m, dev) for m in mats]
    batch = ops.SpmmBatch([a.plan for a, _ in pairs], [t.plan for _, t in pairs])
    g = torch.Generator(device="cpu").manual_seed(0)
    ue = (torch.randn((T, U, d), generator=g) * 0.1).to(dev)
    ie = (torch.randn((T, I, d), generator=g) * 0.1).to(dev)
    gu, gi = torch.randn((T, U, d), generator=g).to(dev), torch.randn((T, I, d), generator=g).to(dev)
    ou, oi, du, di = (torch.empty_like(x) for x in (ue, ie, ue, ie))
    mu = torch.empty((T, L, U, d // 4), dtype=torch.uint8, device=dev)
    mi = torch.empty((T, L, I, d // 4), dtype=torch.uint8, device=dev)
    su, si = torch.empty(4 * T * U * d, device=dev), torch.empty(4 * T * I * d, device=dev)

    def stack(drop):
        kw = {} if drop is None else {"drop": drop}
        def run():
            ops.gnn_stack(batch, ue, ie, L, 0.5, ou, oi, su, si, mask_u=mu, mask_i=mi, **kw)
            ops.gnn_stack_bwd(batch, gu, gi, L, 0.5, mu, mi, du, di, su, si, **kw)
        return run

    report("stack fwd+bwd (Gowalla-shaped, d=64, L=2)", [("undropped (existing entry)", stack(None))] +
           [(n, stack(dr)) for n, dr in drops], opt.rounds, 10, lines)
    del batch, pairs, ue, ie, gu, gi, ou, oi, du, di, mu, mi, su, si

    # ---- one per-interval SpMM, quarter-scale roofline graph (power-law degrees: all three row classes)
    n, nnz = 250_000, 25_000_000
    eu, ei = synthetic.powerlaw_edges(n, n, nnz, seed=3, device=dev)
    (rp, ci), _ = synthetic.csr_pair_from_edges(eu, ei, n, n)
    plan = ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False)
    del eu, ei
    x = torch.randn((n, d), generator=g).to(dev)
    res = torch.randn((n, d), generator=g).to(dev)
    out = torch.empty((n, d), device=dev)

    def one(drop):
        if drop is None:
            return lambda: ops.spmm_ex(plan, x, 0.5, residual=res, out=out)
        return lambda: ops.spmm_drop(plan, x, 0.5, drop, ops.edge_tag(1, 1, 0), True, residual=res, out=out)

    report(f"one SpMM ({n} rows, {plan.nnz} edges, d=64)", [("undropped (existing entry)", one(None))] +
           [(nm, one(dr)) for nm, dr in drops], opt.rounds, 5, lines)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
