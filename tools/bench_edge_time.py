#!/usr/bin/env python3
"""Times the interval SpMM with and without time-aware messages, in one process:
  - the batched stack (forward + backward) on the Gowalla-shaped synthetic set (U = 48,653, I = 52,619, 3 intervals x
    600 k edges, d = 64, 2 layers): time off (the existing entries on plans without buckets), time on (the time
    entries; the backward includes the dTE reduction), and the dTE reduction of one layer alone;
  - one per-interval SpMM on a quarter-scale synthetic graph of the roofline workload (250 k x 250 k, 25 M edges), time
    off and on.
Bucket ids are drawn uniformly from --buckets ids (default 90: three months of day buckets), so the time-adjoint plans
have a few very long rows: each of the 90 buckets of an interval holds about 6,700 edges, 27 chunks per fix-up wave.
The forms are alternated round by round so that all see the same machine state. Median of --rounds rounds and each
form's min - max.

--parent-lib PATH: afterwards the time-off entries are timed on the library at PATH (a build of the parent commit) and
on this build, in child processes alternated --pairs times in the same job (--baseline-only does this; a library from
before the time entries is loaded without their symbols).

Numbers of different machines are not comparable."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import _lib      # noqa: E402


def timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def report(title, runs, rounds, inner, out):
    times = {name: [] for name, _ in runs}
    for name, fn in runs:                      # warm-up
        timed(fn, 3)
    for _ in range(rounds):                    # alternated
        for name, fn in runs:
            times[name].append(timed(fn, inner))
    base = float(np.median(times[runs[0][0]]))
    for name, _ in runs:
        v = times[name]
        line = (f"{title}: {name:<32} median {np.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
                f"ratio to time off {np.median(v) / base:5.3f}  ({rounds} rounds of {inner})")
        print(line, flush=True)
        out.append(line)


def bench(opt, lines):
    from sa_gnn_amd import graph, ops, synthetic
    dev = torch.device("cuda:0")
    timed_forms = not opt.baseline_only
    M = opt.buckets
    rng = np.random.default_rng(5)

    # ---- the batched stack, Gowalla-shaped
    np.random.seed(100)
    U, I, T, L, d = 48653, 52619, 3, 2, 64
    mats = synthetic.make_trn_mat_time(U, I, [600000] * T)[1]
    plain = [graph.interval_pair(m, dev) for m in mats]
    batch_off = ops.SpmmBatch([a.plan for a, _ in plain], [t.plan for _, t in plain])
    g = torch.Generator(device="cpu").manual_seed(0)
    ue = (torch.randn((T, U, d), generator=g) * 0.1).to(dev)
    ie = (torch.randn((T, I, d), generator=g) * 0.1).to(dev)
    gu, gi = torch.randn((T, U, d), generator=g).to(dev), torch.randn((T, I, d), generator=g).to(dev)
    ou, oi, du, di = (torch.empty_like(x) for x in (ue, ie, ue, ie))
    mu = torch.empty((T, L, U, d // 4), dtype=torch.uint8, device=dev)
    mi = torch.empty((T, L, I, d // 4), dtype=torch.uint8, device=dev)
    su, si = torch.empty(4 * T * U * d, device=dev), torch.empty(4 * T * I * d, device=dev)

    def stack(batch, te=None, dte=None):
        def run():
            ops.gnn_stack(batch, ue, ie, L, 0.5, ou, oi, su, si, mask_u=mu, mask_i=mi, time=te)
            ops.gnn_stack_bwd(batch, gu, gi, L, 0.5, mu, mi, du, di, su, si, time=te, grad_time=dte)
        return run

    runs = [("time off (existing entries)", stack(batch_off))]
    if timed_forms:
        def with_buckets(adj):
            p = adj.plan
            return ops.SpmmPlan(p.rowptr, p.colidx, p.n_rows, p.n_src, device=dev, validate=False,
                                buckets=rng.integers(0, M, p.nnz).astype(np.uint16), n_buckets=M)
        batch_on = ops.SpmmBatch([with_buckets(a) for a, _ in plain], [with_buckets(t) for _, t in plain])
        te = (torch.randn((T, L, 2, M, d), generator=g) * 0.1).to(dev)
        dte = torch.empty_like(te)
        adj = batch_on.time_adjoint
        info = adj.plans_user[0].info
        lines.append(f"time adjoint of interval 0, user side: {info.n_rows} rows, {info.nnz} edges, {info.n_long_rows} long rows, "
                     f"{info.n_chunks} chunks")
        print(lines[-1], flush=True)
        gm_u, gm_i = gu.contiguous(), gi.contiguous()
        dte_l = torch.empty((T, M, d), device=dev), torch.empty((T, M, d), device=dev)

        reduction = lambda: _dte_alone(ops, adj, gm_u, gm_i, dte_l)      # noqa: E731
        runs += [("time on (fwd + bwd + dTE)", stack(batch_on, te, dte)), ("dTE reduction alone, one layer", reduction)]
    report("stack fwd+bwd (Gowalla-shaped, d=64, L=2)", runs, opt.rounds, 10, lines)
    del runs, ue, ie, gu, gi, ou, oi, du, di, mu, mi, su, si
    torch.cuda.empty_cache()

    # ---- one per-interval SpMM, quarter-scale roofline graph (power-law degrees: all three row classes)
    n, nnz = 250_000, 25_000_000
    eu, ei = synthetic.powerlaw_edges(n, n, nnz, seed=3, device=dev)
    (rp, ci), _ = synthetic.csr_pair_from_edges(eu, ei, n, n)
    del eu, ei
    x = torch.randn((n, d), generator=g).to(dev)
    res = torch.randn((n, d), generator=g).to(dev)
    out = torch.empty((n, d), device=dev)
    off = ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False)
    runs = [("time off (existing entry)", lambda: ops.spmm_ex(off, x, 0.5, residual=res, out=out))]
    if timed_forms:
        on = ops.SpmmPlan(rp, ci, n, n, device=dev, validate=False, buckets=rng.integers(0, M, off.nnz).astype(np.uint16),
                          n_buckets=M)
        te1 = (torch.randn((M, d), generator=g) * 0.1).to(dev)
        runs.append(("time on (spmm_time)", lambda: ops.spmm_time(on, x, 0.5, te1, residual=res, out=out)))
    report(f"one SpMM ({n} rows, {off.nnz} edges, d=64)", runs, opt.rounds, 5, lines)


def _dte_alone(ops, adj, gm_u, gm_i, dte_l):
    """The dTE reduction of one layer through the per-plan entry of every time-adjoint plan (the batched launch is
    reachable through the backward entry only): 2 T products whose rows are buckets."""
    for k in range(adj.T):
        ops.spmm_ex(adj.plans_user[k], gm_u[k], 1.0, out=dte_l[0][k])
        ops.spmm_ex(adj.plans_item[k], gm_i[k], 1.0, out=dte_l[1][k])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--baseline-only", action="store_true", help="time the time-off entries only")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit to time the time-off entries on")
    ap.add_argument("--pairs", type=int, default=3, help="alternated (parent, this build) child runs for --parent-lib")
    ap.add_argument("--buckets", type=int, default=90, help="bucket ids drawn per edge (the table has this many rows)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    opt = ap.parse_args()
    lines = []
    if opt.baseline_only:
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:      # a library from before the time entries
            _lib.SIGNATURES.pop(name)
    bench(opt, lines)
    if opt.parent_lib:
        torch.cuda.empty_cache()
        me = os.path.abspath(__file__)
        for r in range(opt.pairs):
            for name, lib in (("parent library", opt.parent_lib), ("this build", None)):
                env = dict(os.environ)
                env.pop("SAGNN_LIB", None)
                if lib:
                    env["SAGNN_LIB"] = lib
                res = subprocess.run([sys.executable, me, "--baseline-only", "--rounds", str(opt.rounds)], env=env,
                                     capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    raise SystemExit(f"{name} child failed ({res.returncode}): {res.stderr[-2000:]}")
                for line in res.stdout.splitlines():
                    line = f"[pair {r + 1}, {name}] {line}"
                    print(line, flush=True)
                    lines.append(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
