"""Times the position-wise feed-forward block of the sequence head (--seqFFN), forward and backward, at
B = 512 slots, P = 200, d = 64, F in {64, 256} on the sequence lengths of the Gowalla-shaped synthetic set of
tools/time_train_epoch.py: the fused ragged entries (ops.seq_ffn, ops.seq_ffn_bwd) against the same function composed
from the existing entries over the whole slab (layernorm_td, dense_nn, leaky, dense_nn, leaky_add; backward dense_tn,
dense_nn, leaky_bwd, dense_tn, dense_nn, layernorm_td_bwd, leaky_add, with z, a and h kept from the forward, which the
fused backward recomputes). Both in one process, alternated round by round, so each sees the same machine state; the
figure is the median of the rounds (device time between two events around `--inner` back-to-back calls). Prints the
agreement of the two forms on the real rows first. DESIGN.md §30 quotes profiles/seq_ffn_bench.txt."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import ops      # noqa: E402
from bench_seq_attn import gowalla_shaped_lengths, timed      # noqa: E402


def composed_fwd(x, p, leaky):
    """(out, z, a, h) over every row of the slab: the padding is computed like the real rows."""
    R, d = x.shape
    z = ops.layernorm_td(x.view(R, 1, d), p[0], p[1]).view(R, d)
    a = ops.dense_nn(z, p[2], p[3])
    h = ops.leaky(a, leaky)
    return ops.leaky_add(ops.dense_nn(h, p[4], p[5]), x, 1.0), z, a, h


def composed_bwd(x, g, p, W1t, W2t, z, a, h, leaky):
    R, d = x.shape
    dev = x.device
    dW2, db2 = torch.zeros_like(p[4]), torch.zeros(d, dtype=torch.float32, device=dev)
    ops.dense_tn(h, g, dW2, db2)
    da = ops.leaky_bwd(a, ops.dense_nn(g, W2t, None), leaky)
    dW1, db1 = torch.zeros_like(p[2]), torch.zeros(p[2].shape[1], dtype=torch.float32, device=dev)
    ops.dense_tn(z, da, dW1, db1)
    dz = ops.dense_nn(da, W1t, None).view(R, 1, d)
    dy, dgamma, dbeta = ops.layernorm_td_bwd(x.view(R, 1, d), dz, p[0], out=dz)
    return ops.leaky_add(dy.view(R, d), g, 1.0), dgamma, dbeta, dW1, db1, dW2, db2


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, d, leaky = 512, 200, 64, 0.5
    lens = gowalla_shaped_lengths(B, P)
    print(f"B = {B}, P = {P}, d = {d}; lengths: mean {lens.mean():.1f}, median {int(np.median(lens))}, max {lens.max()}, "
          f"empty {int((lens == 0).sum())}; {int(lens.sum())} real rows of {B * P} ({100.0 * lens.sum() / (B * P):.1f} %)")
    g0 = torch.Generator(device="cpu").manual_seed(0)
    lens_d = torch.from_numpy(lens).to(dev)
    real = (torch.arange(P, device=dev)[None, :] < lens_d[:, None]).reshape(B * P, 1)
    x = torch.randn((B * P, d), generator=g0).to(dev) * real              # activation slabs hold zeros in the padding
    g = torch.randn((B * P, d), generator=g0).to(dev) * real              # the padding rule: zero gradient rows
    runs = {}
    for F in (64, 256):
        lim = float(np.sqrt(6.0 / (d + F)))
        rnd = lambda *s: torch.rand(s, generator=g0) * 2 - 1
        p = [t.to(dev).contiguous() for t in (1 + 0.1 * rnd(d), 0.1 * rnd(d), lim * rnd(d, F), 0.1 * rnd(F), lim * rnd(F, d),
                                              0.1 * rnd(d))]
        W1t, W2t = p[2].t().contiguous(), p[4].t().contiguous()
        out_c, z, a, h = composed_fwd(x, p, leaky)
        out_f = ops.seq_ffn(x, *p, lens_d, P, leaky)
        print(f"F = {F}: fused vs composed on the real rows, max |out diff| {float(((out_f - out_c) * real).abs().max()):.2e} "
              f"at scale {float(out_f.abs().max()):.2e}; padded rows of the fused out: {int(torch.count_nonzero(out_f * ~real))} non-zero")
        gf = ops.seq_ffn_bwd(x, g, *p, lens_d, P, leaky)
        gc = composed_bwd(x, g, p, W1t, W2t, z, a, h, leaky)
        names = ("dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2")
        diffs = [float(((u - v) * real).abs().max()) if n == "dx" else float((u - v).abs().max()) for n, u, v in zip(names, gf, gc)]
        print("         gradients, max |diff| (scale): " + ", ".join(f"{n} {e:.2e} ({float(v.abs().max()):.2e})"
                                                                      for n, e, v in zip(names, diffs, gc)))
        runs[f"F = {F:3d}"] = {
            "fused fwd": lambda p=p: ops.seq_ffn(x, *p, lens_d, P, leaky),
            "fused bwd": lambda p=p: ops.seq_ffn_bwd(x, g, *p, lens_d, P, leaky),
            "composed fwd": lambda p=p: composed_fwd(x, p, leaky),
            "composed bwd": lambda p=p, W1t=W1t, W2t=W2t, z=z, a=a, h=h: composed_bwd(x, g, p, W1t, W2t, z, a, h, leaky),
        }
    times = {n: {k: [] for k in r} for n, r in runs.items()}
    for n, r in runs.items():                          # warm-up
        for fn in r.values():
            timed(fn, 2)
    for _ in range(opt.rounds):                        # alternated: every configuration in every round
        for n, r in runs.items():
            for k, fn in r.items():
                times[n][k].append(timed(fn, opt.inner))
    print(f"median of {opt.rounds} rounds of {opt.inner} calls, ms per call (min .. max of the rounds)")
    for n, t in times.items():
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = ", ".join(f"{k} {med[k]:.3f} ({min(t[k]):.3f} .. {max(t[k]):.3f})" for k in t)
        print(f"[{n}] {spread}; composed / fused: fwd {med['composed fwd'] / med['fused fwd']:.1f}x, "
              f"bwd {med['composed bwd'] / med['fused bwd']:.1f}x")


if __name__ == "__main__":
    main()
