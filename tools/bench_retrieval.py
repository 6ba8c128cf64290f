"""Times full-catalogue top-K retrieval (ops.score_topk -> sagnn_score_topk_f32) against torch.mm + torch.topk on
the same batch, and prints one JSON line per case. Needs a GPU; there is no CPU path.

  python tools/bench_retrieval.py [--iters 20] [--warmup 3] [--cases synthetic-k10,gowalla]

Cases: the synthetic 5 M-item table at d 64 / batch 512 for k = 10 and 100, a Gowalla-shaped table (52,619 items,
d 32) and a MovieLens-shaped one (3,706 items, d 128). The baseline cuts the item table into pieces whose score
block fits 2 GiB and merges the per-piece top-k."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sa_gnn_amd import ops  # noqa: E402

PEAK_TF = 155.0     # measured fp32-MFMA rate of the MI355X (v_mfma_f32_16x16x4_f32)
CASES = {
    "synthetic-k10": (5_000_000, 64, 512, 10),
    "synthetic-k100": (5_000_000, 64, 512, 100),
    "gowalla": (52_619, 32, 512, 10),
    "movielens": (3_706, 128, 512, 10),
}


def baseline(Q, I, k):
    rows = max(1, (1 << 31) // (4 * Q.shape[0]))
    best_s, best_i = None, None
    for st in range(0, I.shape[0], rows):
        s, i = torch.topk(Q @ I[st:st + rows].T, min(k, I.shape[0] - st), dim=1)
        i = i + st
        if best_s is not None:
            s, j = torch.topk(torch.cat([best_s, s], 1), k, dim=1)
            i = torch.gather(torch.cat([best_i, i], 1), 1, j)
        best_s, best_i = s, i
    return best_i, best_s


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
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_retrieval: no GPU visible")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for name in a.cases.split(","):
        n_items, d, B, k = CASES[name]
        I = torch.randn((n_items, d), generator=g, device=dev)
        Q = torch.randn((B, d), generator=g, device=dev)
        tgt = torch.randint(0, n_items, (B,), generator=g, device=dev, dtype=torch.int32)
        ms = timed(lambda: ops.score_topk(Q, I, k, target=tgt), a.iters, a.warmup)
        flop = 2.0 * B * n_items * d
        rec = {"case": name, "n_items": n_items, "d": d, "batch": B, "k": k, "ms_per_batch": round(ms, 4),
               "tflops": round(flop / ms / 1e9, 2), "frac_of_155": round(flop / ms / 1e9 / PEAK_TF, 4)}
        if not a.no_baseline:
            bms = timed(lambda: baseline(Q, I, k), max(3, a.iters // 4), 1)
            items, _, _ = ops.score_topk(Q, I, k, target=tgt)
            bi, _ = baseline(Q, I, k)
            rec.update({"torch_mm_topk_ms": round(bms, 4), "speedup": round(bms / ms, 2),
                        "top1_agree": float((items[:, 0] == bi[:, 0].int()).float().mean())})
        print(json.dumps(rec), flush=True)
        del I, Q


if __name__ == "__main__":
    main()
