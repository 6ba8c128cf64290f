"""numpy restatement of the rows --fusion_rows batch fuses (model.Recommender._touched_rows): the user and item rows
a training batch's loss reads, per source list, and their ascending union (what sagnn_rows_compact_i32 returns)."""
import numpy as np


def _ids(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.int64).reshape(-1)


def segment_items(seq_items, seg_begin, seg_len, P):
    """The items of the device sampler's sequence segments, as sagnn_seq_sum_f32 reads them (j < min(len, P))."""
    flat, beg, ln = _ids(seq_items), _ids(seg_begin), _ids(seg_len)
    out = [flat[b:b + min(max(n, 0), P)] for b, n in zip(beg, ln)]
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def touched_sources(batch, P=None, seq_items=None):
    """{"users": {source: ids}, "items": {source: ids}} for a host batch (sequence / mask) or a device batch (seq_seg,
    with the sampler's seq_items and pos_length P)."""
    users = {"uids": _ids(batch["uids"])}
    items = {"iids": _ids(batch["iids"])}
    for k, (su, si) in enumerate(zip(batch["suids"], batch["siids"])):
        users[f"suids[{k}]"] = _ids(su)
        items[f"siids[{k}]"] = _ids(si)
    if "seq_seg" in batch:
        items["sequence"] = segment_items(seq_items, *batch["seq_seg"], P)
    else:
        seq, mask = np.asarray(batch["sequence"], dtype=np.int64), np.asarray(batch["mask"]) != 0
        items["sequence"] = seq[mask]
    if "cand" in batch:                                   # --softmaxNegs: the step's candidate rows
        items["cand"] = _ids(batch["cand"])
    return {"users": users, "items": items}


def touched_rows(batch, n_users, n_items, P=None, seq_items=None):
    """(users, items): ascending unique row ids inside the tables, and the host-known capacities (cap_u, cap_i)."""
    src = touched_sources(batch, P, seq_items)
    out, caps = [], []
    for side, n in (("users", n_users), ("items", n_items)):
        ids = np.concatenate(list(src[side].values()))
        out.append(np.unique(ids[(ids >= 0) & (ids < n)]))
        caps.append(min(n, sum(len(v) for v in src[side].values())))
    return out[0], out[1], tuple(caps)
