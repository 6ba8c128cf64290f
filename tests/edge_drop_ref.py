"""numpy restatement of the edge-dropout contract of the interval SpMM (include/sagnn.h, "Edge dropout of the interval
graphs"), on the Philox4x32-10 of device_sampler_ref. The edge-dropout tests compare the kernels with it
bit for bit and build their float64 references from its masks."""
import math

import numpy as np

from device_sampler_ref import philox4x32_10


def threshold(keep: float) -> int:
    """min(floor(keep * 2^32), 2^32 - 1): the uint32 a draw must stay below for its edge to be kept."""
    return min(int(math.floor(float(keep) * 2.0 ** 32)), 2 ** 32 - 1)


def tag(k: int, l: int, direction: int) -> int:
    """direction 0: the user-side product A e_i of layer l, 1: the item-side product A^T e_u."""
    return (int(k) << 8) | (int(l) << 1) | int(direction)


def keep_mask(seed, step, k, l, direction, users, items, keep=None, thresh=None):
    """bool array: edge (users[j], items[j]) of interval k, layer l, direction is kept. Give `keep` or `thresh`."""
    t = threshold(keep) if thresh is None else int(thresh)
    w0 = philox4x32_10(np.asarray(users), np.asarray(items), tag(k, l, direction), int(step), seed)[0]
    return w0.astype(np.uint64) < np.uint64(t)


def dense_mask(seed, step, k, l, direction, n_users, n_items, keep=None, thresh=None):
    """[n_users, n_items] bool: keep_mask of every (user, item) pair."""
    u, i = np.meshgrid(np.arange(n_users), np.arange(n_items), indexing="ij")
    return keep_mask(seed, step, k, l, direction, u.ravel(), i.ravel(), keep, thresh).reshape(n_users, n_items)
