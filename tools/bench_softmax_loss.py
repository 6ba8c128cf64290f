"""Times the full-catalogue softmax loss (ops.softmax_loss / softmax_loss_bwd -> sagnn_softmax_loss_f32 and its
backward) at 512 queries, forward and forward + backward, beside the materialised torch form
cross_entropy(Q @ I.T / temp + mask) in the same process, and prints one JSON line per case. Needs a GPU.

  python tools/bench_softmax_loss.py [--iters 20] [--warmup 3] [--rounds 5] [--cases gowalla,movielens,synthetic]
                                     [--cand 4096] [--dist pop] [--d 64]

Cases: Gowalla-shaped (52,619 items, d 32), MovieLens-shaped (3,706 items, d 128), synthetic (5 M items, d 64). Every
user excludes 100 random items. The two forms alternate round by round; the figures are medians over the rounds. The
torch form runs where its [512, n_items] logits, mask and softmax fit (not at 5 M items). The per-kernel split comes
from sagnn_profile_read (kind 6: one record per entry) and, kernel by kernel, from a profiler's kernel trace.
--cand N adds the candidate mode (--softmaxNegs: ops.softmax_loss_cand and its backward over N candidates drawn by
ops.sample_strata, the backward followed by the assembly of the full-size dI as autograd.SoftmaxLossCandFn does it),
alternated with the full form in the same rounds; cases with fewer than N items skip it.
--dist pop (with --cand) adds the popularity-weighted form (--softmaxNegDist pop) to the same rounds: N candidates drawn
by ops.sample_strata_weighted over weights (degree + 1)^0.75 of Zipf(1.3) degrees, the entries with the per-position
offset, and the live rows scattered into the full-size dI (ops.softmax_cand_scatter); it also times the two draws.
Rates count 2 * queries * items * d flops per product: one product forward, four backward (the scores twice, dQ, dI)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sa_gnn_amd import ops  # noqa: E402

PEAK_TF = 155.0     # measured fp32-MFMA rate of the MI355X (v_mfma_f32_16x16x4_f32)
CASES = {"gowalla": (52_619, 32, 512), "movielens": (3_706, 128, 512), "synthetic": (5_000_000, 64, 512)}
N_EXCL = 100


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--cand", type=int, default=0, help="also time the candidate mode over this many sampled candidates")
    ap.add_argument("--dist", choices=("uniform", "pop"), default="uniform",
                    help="pop: also time the popularity-weighted candidate form beside the uniform one (needs --cand)")
    ap.add_argument("--d", type=int, default=0, help="override the cases' width (32, 64 or 128)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_softmax_loss: no GPU visible")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    inv_temp = 1.0 / a.temp
    for name in a.cases.split(","):
        n_items, d, B = CASES[name]
        d = a.d or d
        I = torch.randn((n_items, d), generator=g, device=dev) * 0.3
        Q = torch.randn((B, d), generator=g, device=dev) * 0.3
        tgt = torch.randint(0, n_items, (B,), generator=g, device=dev, dtype=torch.int32)
        lists = np.sort(rng.integers(0, n_items, (B, N_EXCL)), axis=1)
        ptr = torch.arange(0, (B + 1) * N_EXCL, N_EXCL, dtype=torch.int64, device=dev)
        items = torch.from_numpy(lists.reshape(-1).astype(np.int32)).to(dev)
        one = torch.ones(1, device=dev)
        excl = (ptr, items)

        def fwd():
            return ops.softmax_loss(Q, I, tgt, inv_temp, None, excl)

        def fwd_bwd():
            _, lse, _ = fwd()
            return ops.softmax_loss_bwd(Q, I, tgt, lse, one, inv_temp, None, excl)

        n_cand = a.cand if 0 < a.cand <= n_items else 0
        if n_cand:
            cand = ops.sample_strata(n_items, n_cand, 0, 0, dev)

            def c_fwd():
                return ops.softmax_loss_cand(Q, I, cand, tgt, inv_temp, None, excl)

            def c_fwd_bwd():
                _, lse, _ = c_fwd()
                dQ, dIc, dT = ops.softmax_loss_cand_bwd(Q, I, cand, tgt, lse, one, inv_temp, None, excl)
                dI = torch.zeros_like(I)
                dI.index_copy_(0, cand.long(), dIc)
                return dQ, ops.softmax_target_add(dI, dT, tgt)

            def c_kernels():     # the two entries alone, without the full-size dI
                _, lse, _ = c_fwd()
                return ops.softmax_loss_cand_bwd(Q, I, cand, tgt, lse, one, inv_temp, None, excl)

        pop = bool(n_cand) and a.dist == "pop"
        if pop:
            from sa_gnn_amd.model import pop_cum
            cum_h, total = pop_cum(np.minimum(rng.zipf(1.3, n_items), n_items), 0.75)
            cum = torch.from_numpy(cum_h).to(dev)
            pcand, pbias = ops.sample_strata_weighted(cum, total, n_cand, 0, 0)

            def p_fwd():
                return ops.softmax_loss_cand(Q, I, pcand, tgt, inv_temp, None, excl, bias=pbias)

            def p_kernels():
                _, lse, _ = p_fwd()
                return ops.softmax_loss_cand_bwd(Q, I, pcand, tgt, lse, one, inv_temp, None, excl, bias=pbias)

            def p_fwd_bwd():
                dQ, dIc, dT = p_kernels()
                dI = ops.softmax_cand_scatter(torch.zeros_like(I), dIc, pcand, pbias)
                return dQ, ops.softmax_target_add(dI, dT, tgt)

            def draw_u():
                return ops.sample_strata(n_items, n_cand, 0, 1, dev)

            def draw_p():
                return ops.sample_strata_weighted(cum, total, n_cand, 0, 1)

        torch_fits = B * n_items * 4 * 6 < (8 << 30)
        if torch_fits:
            mask = torch.zeros((B, n_items), device=dev)
            mask[torch.arange(B, device=dev).repeat_interleave(N_EXCL), items.long()] = float("-inf")
            mask[torch.arange(B, device=dev), tgt.long()] = 0.0
            Qt, It = Q.clone().requires_grad_(True), I.clone().requires_grad_(True)

            def t_fwd():
                with torch.no_grad():
                    return torch.nn.functional.cross_entropy(Q @ I.T * inv_temp + mask, tgt.long())

            def t_fwd_bwd():
                Qt.grad = It.grad = None
                torch.nn.functional.cross_entropy(Qt @ It.T * inv_temp + mask, tgt.long()).backward()

        res = {k: [] for k in ("fwd", "fwd_bwd", "torch_fwd", "torch_fwd_bwd", "cand_fwd", "cand_fwd_bwd", "cand_kernels",
                               "pop_fwd", "pop_fwd_bwd", "pop_kernels", "draw_uniform", "draw_pop")}
        for _ in range(a.rounds):          # alternated: both forms see the same machine state
            res["fwd"].append(timed(fwd, a.iters, a.warmup))
            res["fwd_bwd"].append(timed(fwd_bwd, a.iters, a.warmup))
            if n_cand:
                res["cand_fwd"].append(timed(c_fwd, a.iters, a.warmup))
                res["cand_fwd_bwd"].append(timed(c_fwd_bwd, a.iters, a.warmup))
                res["cand_kernels"].append(timed(c_kernels, a.iters, a.warmup))
            if pop:
                res["pop_fwd"].append(timed(p_fwd, a.iters, a.warmup))
                res["pop_fwd_bwd"].append(timed(p_fwd_bwd, a.iters, a.warmup))
                res["pop_kernels"].append(timed(p_kernels, a.iters, a.warmup))
                res["draw_uniform"].append(timed(draw_u, a.iters, a.warmup))
                res["draw_pop"].append(timed(draw_p, a.iters, a.warmup))
            if torch_fits:
                res["torch_fwd"].append(timed(t_fwd, a.iters, a.warmup))
                res["torch_fwd_bwd"].append(timed(t_fwd_bwd, a.iters, a.warmup))
        med = {k: float(np.median(v)) for k, v in res.items() if v}
        flop = 2.0 * B * n_items * d
        bwd_ms = med["fwd_bwd"] - med["fwd"]
        rec = {"case": name, "n_items": n_items, "d": d, "queries": B, "fwd_ms": round(med["fwd"], 4),
               "fwd_bwd_ms": round(med["fwd_bwd"], 4), "fwd_tflops": round(flop / med["fwd"] / 1e9, 2),
               "fwd_frac_of_155": round(flop / med["fwd"] / 1e9 / PEAK_TF, 4),
               "bwd_tflops": round(4 * flop / bwd_ms / 1e9, 2), "bwd_frac_of_155": round(4 * flop / bwd_ms / 1e9 / PEAK_TF, 4)}
        if n_cand:
            rec.update({"n_cand": n_cand, "cand_fwd_ms": round(med["cand_fwd"], 4),
                        "cand_fwd_bwd_entries_ms": round(med["cand_kernels"], 4),
                        "cand_fwd_bwd_with_full_dI_ms": round(med["cand_fwd_bwd"], 4),
                        "cand_fwd_speedup": round(med["fwd"] / med["cand_fwd"], 2),
                        "cand_fwd_bwd_speedup": round(med["fwd_bwd"] / med["cand_fwd_bwd"], 2),
                        "cand_loss": float(c_fwd()[0])})
        if pop:
            spread = lambda k: [round(min(res[k]), 4), round(max(res[k]), 4)]      # noqa: E731
            rec.update({"pop_fwd_ms": round(med["pop_fwd"], 4), "pop_fwd_bwd_entries_ms": round(med["pop_kernels"], 4),
                        "pop_fwd_bwd_with_full_dI_ms": round(med["pop_fwd_bwd"], 4),
                        "draw_uniform_ms": round(med["draw_uniform"], 4), "draw_pop_ms": round(med["draw_pop"], 4),
                        "pop_live": int(torch.isfinite(pbias).sum()), "pop_loss": float(p_fwd()[0]),
                        "min_max_over_rounds": {k: spread(k) for k in ("cand_fwd", "pop_fwd", "cand_kernels", "pop_kernels",
                                                                       "cand_fwd_bwd", "pop_fwd_bwd")}})
        if torch_fits:
            loss = float(fwd()[0])
            rec.update({"torch_fwd_ms": round(med["torch_fwd"], 4), "torch_fwd_bwd_ms": round(med["torch_fwd_bwd"], 4),
                        "fwd_speedup": round(med["torch_fwd"] / med["fwd"], 2),
                        "fwd_bwd_speedup": round(med["torch_fwd_bwd"] / med["fwd_bwd"], 2),
                        "loss": loss, "torch_loss": float(t_fwd())})
            del mask, Qt, It
        print(json.dumps(rec), flush=True)
        del I, Q


if __name__ == "__main__":
    main()
