"""Times one call of the sequence attention, forward and backward, at B = 512 slots, P = 200, d = 64 on the sequence
lengths of the Gowalla-shaped synthetic set of tools/time_train_epoch.py: 16 heads on the VALU kernels (ops.seq_attn),
4, 2 and 1 heads on the matrix-core kernels (ops.seq_attn_wide, --seqHeads), with the mask off and on, and in the same
process the materialised torch form on the same slab: bmm -> masked softmax quotient -> bmm and its autograd backward.
The configurations alternate round by round, so each sees the same machine state; the figure is the median of the rounds
(device time between two events around `--inner` back-to-back calls). DESIGN.md §29 quotes profiles/seq_heads_bench.txt."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from sa_gnn_amd import ops, synthetic      # noqa: E402


def gowalla_shaped_lengths(B, P, seed=3):
    """The head's sequence lengths of B users of the Gowalla-shaped set: all items but the last, at most P."""
    np.random.seed(100)
    seq = synthetic.make_sequence(synthetic.make_trn_mat_time(48653, 52619, [600000] * 3))
    users = np.random.default_rng(seed).permutation(len(seq))[:B]
    return np.array([min(max(len(seq[u]) - 1, 0), P) for u in users], dtype=np.int32)


def torch_form(qkv, key_mask, tri, B, P, d, heads):
    """ctx [B * P, d] of the contract, every P x P score materialised: what the kernels are compared with."""
    dk = d // heads
    q, k, v = (qkv[:, i * d:(i + 1) * d].reshape(B, P, heads, dk).permute(0, 2, 1, 3).reshape(B * heads, P, dk) for i in range(3))
    s = torch.bmm(q, k.transpose(1, 2)) * (1.0 / np.sqrt(dk))
    mask = key_mask if tri is None else key_mask & tri                   # [B * heads, 1 or P, P]
    s = s.masked_fill(~mask, float("-inf"))
    m = s.detach().amax(-1, keepdim=True).clamp_min(-1e30)               # the shift leaves the quotient what it is: no gradient
    e = torch.exp(s - m)
    a = e / (e.sum(-1, keepdim=True) + 1e-8 * torch.exp(-m))
    return torch.bmm(a, v).reshape(B, heads, P, dk).permute(0, 2, 1, 3).reshape(B * P, d)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    B, P, d = 512, 200, 64
    lens = gowalla_shaped_lengths(B, P)
    print(f"B = {B}, P = {P}, d = {d}; lengths: mean {lens.mean():.1f}, median {int(np.median(lens))}, max {lens.max()}, "
          f"empty {int((lens == 0).sum())}; sum of n^2 {int((lens.astype(np.int64) ** 2).sum())} of B P^2 = {B * P * P}")
    g0 = torch.Generator(device="cpu").manual_seed(0)
    qkv = (0.5 * torch.randn((B * P, 3 * d), generator=g0)).to(dev)
    g = torch.randn((B * P, d), generator=g0).to(dev)
    lens_d = torch.from_numpy(lens).to(dev)
    real = (torch.arange(P, device=dev)[None, :] < lens_d[:, None])       # [B, P]
    g = g * real.reshape(B * P, 1)                                         # the padding rule: zero gradient rows
    tri = torch.tril(torch.ones((P, P), dtype=torch.bool, device=dev))[None]
    runs = {}
    for heads in (16, 4, 2, 1):
        wide = d // heads >= 16
        fwd_op, bwd_op = (ops.seq_attn_wide, ops.seq_attn_wide_bwd) if wide else (ops.seq_attn, ops.seq_attn_bwd)
        key_mask = real.repeat_interleave(heads, 0)[:, None, :]
        for causal in (False, True):
            leaf = qkv.clone().requires_grad_(True)
            out = torch_form(leaf, key_mask, tri if causal else None, B, P, d, heads)
            # the torch form computes what the kernel computes, on the real rows
            got = fwd_op(qkv, lens_d, P, heads, causal)
            err = float(((out.detach() - got) * real.reshape(B * P, 1)).abs().max())
            dq = bwd_op(qkv, g, lens_d, P, heads, causal)
            (dt,) = torch.autograd.grad(out, leaf, g, retain_graph=True)
            gerr = float((dt - dq).abs().max())
            print(f"heads {heads:2d} causal {int(causal)}: kernel vs torch form, max |ctx diff| {err:.2e}, max |dqkv diff| {gerr:.2e}")
            name = f"heads {heads:2d} (d_k {d // heads:2d}, {'MFMA' if wide else 'VALU'} kernels), causal {int(causal)}"
            runs[name] = {
                "kernel fwd": lambda f=fwd_op, h=heads, c=causal: f(qkv, lens_d, P, h, c),
                "kernel bwd": lambda f=bwd_op, h=heads, c=causal: f(qkv, g, lens_d, P, h, c),
                "torch fwd": lambda km=key_mask, h=heads, c=causal: torch_form(qkv, km, tri if c else None, B, P, d, h),
                "torch bwd": lambda o=out, lf=leaf: torch.autograd.grad(o, lf, g, retain_graph=True),
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
        print(f"[{n}] {spread}; torch / kernel: fwd {med['torch fwd'] / med['kernel fwd']:.1f}x, "
              f"bwd {med['torch bwd'] / med['kernel bwd']:.1f}x")


if __name__ == "__main__":
    main()
