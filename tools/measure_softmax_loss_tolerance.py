"""Measures the constants of the softmax-loss tolerances (tests/test_gpu_softmax_loss.py): the worst
ratio of plain float32 torch on the CPU (logsumexp of the masked product, gradients by autograd) against the float64
restatement, in the units of tests/softmax_loss_ref.tolerance_terms. Each K of the GPU suite is 4 x the worst ratio
found here, rounded up to a power of two (the 4: another summation order and the hardware's exp). No GPU needed.

    python tools/measure_softmax_loss_tolerance.py"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import softmax_loss_ref as R  # noqa: E402


def case(rng, nq, ni, d, amp, temp):
    Q = (rng.standard_normal((nq, d)) * amp).astype(np.float32)
    I = (rng.standard_normal((ni, d)) * amp).astype(np.float32)
    target = rng.integers(0, ni, nq)
    n_ex = max(1, ni // 50)
    lists = [np.sort(rng.integers(0, ni, n_ex)) for _ in range(nq)]          # duplicates allowed
    ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
    return Q, I, target, ptr, np.concatenate(lists), 1.0 / temp


def main():
    rng = np.random.default_rng(0)
    worst = {"lse": 0.0, "dQ": 0.0, "dI": 0.0}
    shapes = [(7, 17), (17, 4099), (40, 4099), (33, 52619)]
    for nq, ni in shapes:
        for d in (32, 64, 128):
            for amp in (0.5, 1.0, 2.0):
                for temp in (0.125, 0.25, 1.0, 4.0):
                    Q, I, target, ptr, items, inv_temp = case(rng, nq, ni, d, amp, temp)
                    scale = 1.0 / nq
                    ref = R.softmax_loss_np(Q, I, target, inv_temp, scale, ptr, items)
                    q32, i32 = torch.from_numpy(Q).requires_grad_(True), torch.from_numpy(I).requires_grad_(True)
                    z = (q32 @ i32.T) * np.float32(inv_temp)
                    mask = torch.zeros_like(z).masked_fill(~torch.from_numpy(ref["eligible"]), float("-inf"))
                    lse = torch.logsumexp(z + mask, dim=1)
                    t = torch.from_numpy(target)
                    (np.float32(scale) * (lse - z.gather(1, t[:, None])[:, 0]).sum()).backward()
                    terms = R.tolerance_terms(Q, I, target, ref, inv_temp, scale)
                    got = {"lse": lse.detach().numpy(), "dQ": q32.grad.numpy(), "dI": i32.grad.numpy()}
                    for k in worst:
                        r = R.worst_ratio(got[k], ref[k], *terms[k])
                        worst[k] = max(worst[k], r)
        print(f"after nq {nq}, n_items {ni}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()), flush=True)
    for k, v in worst.items():
        print(f"{k}: worst float32-CPU ratio {v:.2f} -> K = {2 ** math.ceil(math.log2(4 * v))}")


if __name__ == "__main__":
    main()
