"""CPU side of the slab-shaped softmax-loss suite (test_softmax_slab_host.py, test_gpu_softmax_slab.py):
the input --seqTargets all hands sagnn_softmax_loss_f32 and its backward. No formula is restated: targets and excl_row
are seq_causal_ref.seq_targets_np's, the float64 references softmax_loss_ref.softmax_loss_np,
softmax_cand_ref.softmax_loss_cand_np and softmax_pop_ref.softmax_loss_pop_np, the bounds their tolerance_terms. This file
builds the slab, asserts its structure and evaluates a case in float32 on the CPU the way
tools/measure_softmax_loss_tolerance.py does (softmax_pop_ref.torch_softmax_loss_pop in the dtype of its inputs).

A slab is n_slots x P query rows, row b * P + j token j of slot b. A row is LIVE when it has a target: token j of an
active slot with j < its token count, unless the next token lies outside the catalogue (seq_targets_np's -1: the only way
a row of a slot lies skipped before a live one; the builder calls such a position a hole). Every row of a slot reads its
user's exclusion list. Q is 0.7 N(0, 1) on live rows and exact zeros elsewhere, what sagnn_seq_prefix_query_f32 writes.

The small slab, 11 slots x 24 positions = 264 rows (four 64-row groups and one of 8; 24 is no multiple of 16):

  slot  rows      tokens  user  live rows
   0      0- 23   24       3    all
   1     24- 47   10       5    24-33
   2     48- 71    1       3    48            tile 48-63: only its first row; the user of slot 0
   3     72- 95   12       7    none          inactive: tokens, no positive
   4     96-119    0       8    none
   5    120-143    0       9    none          49-143 skipped: tiles 4-8, pairs 64-95 and 96-127, group 64-127
   6    144-167   24       1    all           one item repeated: 24 rows share a target
   7    168-191   24       2    168-175, 191  holes at 8-22: tile 176-191 has only its last row
   8    192-215   17       4    192-208       slot 0's first tokens: targets shared across slots
   9    216-239    3       6    216-218       tile 224-239 skipped
  10    240-263   24 / 20 10    240-263 / 240-259: the slab's last row live, or skipped"""
import functools

import numpy as np
import torch

import seq_causal_ref as SC
import softmax_cand_ref as C
import softmax_loss_ref as R
import softmax_pop_ref as P

TILE, PAIR, GROUP = 16, 32, 64      # di_kernel's query tile, the chunk kernels' wavefront (kNT x 16 rows), di_kernel's lookup group
N_SLOTS, POS = 11, 24
N_LISTS = 13                        # users 0..12; 0, 11 and 12 own a list no row reads
LONG_SLOTS, LONG_POS = 40, 64

# (mode, n_items, n_cand): FULL at 3 chunks and at 33, CAND across the first chunk boundary, CAND_BIAS over a drawn list
# that repeats ids (softmax_pop_ref.draw over Zipf weights with a hub at id 300)
MODES = (("full", 300, 0), ("full", 4099, 0), ("cand", 4099, 130), ("bias", 700, 300))
CASES = [(mode, ni, nc, d, temp) for mode, ni, nc in MODES for d in (32, 64, 128) for temp in (1.0, 0.25)]
LONG_CASE = ("cand", 1200, 300, 64, 1.0)


def small_spec(last_live=True):
    """(tokens, active, user, holes, rule) per slot: the table above."""
    return [(24, True, 3, (), None), (10, True, 5, (), None), (1, True, 3, (), None), (12, False, 7, (), None),
            (0, True, 8, (), None), (0, True, 9, (), None), (24, True, 1, (), "repeat"), (24, True, 2, tuple(range(8, 23)), None),
            (17, True, 4, (), "copy0"), (3, True, 6, (), None), (24 if last_live else 20, True, 10, (), None)]


def long_spec(rng):
    """40 slots: token counts 0..19 of 64 positions (about 15 % of the rows), every eighth slot inactive, five slots a user."""
    return [(int(rng.integers(0, 20)) if b % 5 else 19, b % 8 != 3, b % 7, (), None) for b in range(LONG_SLOTS)]


def draw_list(mode, n_items, n_cand, seed):
    """(cand int64 [n_cand], bias float32 [n_cand] or None, the ids a row may count as candidates)."""
    if mode == "full":
        return None, None, np.zeros(0, np.int64)
    if mode == "cand":
        cand = C.strata(n_items, n_cand, seed, 1)
        return cand, None, cand
    rng = np.random.default_rng(5)
    deg = np.minimum(rng.zipf(1.3, n_items), 5000).astype(np.int64)
    deg[300] = 200_000                                     # the hub: a run of equal ids across tile boundaries
    _, cum, _ = P.weights(deg, 0.75)
    cand, m, live, bias = P.draw(cum, n_cand, seed, 3)
    assert int(m.max()) >= 20 and (~live).any(), "the drawn list repeats no id"
    return cand, bias, cand[live]


def tokens_and_targets(spec, pos, n_items, pool, rng):
    """The slots' token arrays and positives -> (target, excl_row) int64 [n_slots * pos] by seq_targets_np. Half of
    the tokens come from `pool` (the candidates) where there is one."""
    pick = lambda n: np.where(rng.random(n) < 0.5, pool[rng.integers(0, len(pool), n)], rng.integers(0, n_items, n)) \
        if len(pool) else rng.integers(0, n_items, n)
    seqs, positives = [], []
    for n, active, user, holes, rule in spec:
        s, t = pick(n), int(pick(1)[0])
        if rule == "repeat":
            s[:] = t = int(pool[len(pool) // 2]) if len(pool) else n_items // 2
        elif rule == "copy0":
            s, t = seqs[0][:n].copy(), int(seqs[0][n])
        for j in holes:
            s[j + 1] = n_items                             # row j's target: outside the catalogue
        seqs.append(s)
        positives.append(t if active else -1)
    seg_len = np.array([len(s) for s in seqs])
    seg_begin = np.concatenate([[0], np.cumsum(seg_len)[:-1]])
    users = np.array([u for _, _, u, _, _ in spec])
    return SC.seq_targets_np(np.concatenate(seqs), seg_begin, seg_len, users, np.array(positives), pos, n_items)


def exclusion_lists(rng, n_items, pool, target, excl_row):
    """test_gpu_softmax_negs.py's recipe: about 2 % of the items at random with duplicates, five candidate ids on every
    list, and up to three of the targets of the list's own rows."""
    from test_gpu_softmax_loss import _lists
    ptr, items = _lists(rng, N_LISTS, n_items)
    lists = []
    for u in range(N_LISTS):
        own = np.unique(target[(excl_row == u) & (target >= 0)])[:3]
        hit = pool[rng.integers(0, len(pool), 5)] if len(pool) else np.zeros(0, np.int64)
        lists.append(np.sort(np.concatenate([items[ptr[u]:ptr[u + 1]], hit, own])).astype(np.int64))
    return np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64), np.concatenate(lists)


def structure(target, excl_row, pos):
    """What the small slab promises, as facts about the live mask (full blocks only for the one-row tiles)."""
    live = target >= 0
    n = len(live)

    def skipped_between(w):
        return [k for k in range(0, n, w) if not live[k:k + w].any() and live[:k].any() and live[k + w:].any()]

    tiles = [live[k:k + TILE] for k in range(0, n - TILE + 1, TILE)]
    counts = np.bincount(target[live])
    slots_of = {int(t): set((np.flatnonzero(target == t) // pos).tolist()) for t in np.flatnonzero(counts > 1)}
    return {"live": live, "skipped_tiles": skipped_between(TILE), "skipped_pairs": skipped_between(PAIR),
            "skipped_groups": skipped_between(GROUP),
            "first_only": any(t[0] and not t[1:].any() for t in tiles), "last_only": any(t[-1] and not t[:-1].any() for t in tiles),
            "most_shared": int(counts.max()) if len(counts) else 0, "shared_across_slots": any(len(s) > 1 for s in slots_of.values()),
            "rows_per_list": {int(u): int((live & (excl_row == u)).sum()) for u in np.unique(excl_row[live])}}


def assert_small_structure(c):
    s, target, row = c["structure"], c["target"], c["excl_row"]
    assert len(target) == N_SLOTS * POS == 264 and s["skipped_tiles"] and s["skipped_pairs"] and s["skipped_groups"] == [64]
    assert any(k % GROUP for k in s["skipped_tiles"]) and 224 in s["skipped_tiles"]       # also one outside the skipped group
    assert s["first_only"] and s["last_only"] and bool(s["live"][-1]) == c["last_live"]
    assert s["most_shared"] >= 20 and s["shared_across_slots"] and min(s["rows_per_list"].values()) >= 3
    assert len(set(row[0:24])) == 1 and row[0] == row[48] and len(s["rows_per_list"]) < len(np.unique(row))   # many-to-one
    assert 0.3 < s["live"].mean() < 0.5 and not c["Q"][~s["live"]].any() and c["Q"][s["live"]].any(1).all()
    lists = C.row_lists(len(target), c["ptr"], c["items"], row)
    assert any(target[b] in lists[b] for b in np.flatnonzero(s["live"])), "no list holds a target of its rows"
    if c["cand"] is not None:
        assert all(np.isin(c["pool"], lists[b]).any() for b in np.flatnonzero(s["live"])), "a list hits no candidate"
        assert np.isin(target[s["live"]], c["pool"]).any() and not np.isin(target[s["live"]], c["pool"]).all()


def build(mode, n_items, n_cand, d, temp, last_live=True, long=False, ref=True):
    """One case with everything the float64 reference returns (p, the eligibility mask, the offsets); ref=False: the
    inputs alone. Deterministic."""
    rng = np.random.default_rng(7919 * d + n_items + 13 * n_cand + (1 if last_live else 0) + (2 if long else 0) + int(100 * temp))
    cand, bias, pool = draw_list(mode, n_items, n_cand, 31 + d)
    spec, pos = (long_spec(rng), LONG_POS) if long else (small_spec(last_live), POS)
    target, excl_row = tokens_and_targets(spec, pos, n_items, pool, rng)
    ptr, items = exclusion_lists(rng, n_items, pool, target, excl_row)
    live = target >= 0
    Q = np.where(live[:, None], rng.standard_normal((len(target), d)) * 0.7, 0.0).astype(np.float32)
    I = (rng.standard_normal((n_items, d)) * 0.7).astype(np.float32)
    inv_temp = 1.0 / temp
    c = {"mode": mode, "n_items": n_items, "d": d, "inv_temp": inv_temp, "last_live": last_live, "Q": Q, "I": I, "target": target,
         "excl_row": excl_row, "ptr": ptr, "items": items, "cand": cand, "bias": bias, "pool": pool, "pos": pos,
         "g": np.float32(1.0 / max(int(live.sum()), 1)),   # the upstream gradient of _softmax_pre_loss_all: 1 / count
         "structure": structure(target, excl_row, pos),
         "name": f"{mode} n_items {n_items} n_cand {n_cand} d {d} temp {temp}" + ("" if last_live else " last row skipped")
                 + (" long" if long else "")}
    if ref:
        c["ref"], c["terms"], c["plain"] = reference(c, Q, target, excl_row)
    return c


def reference(c, Q, target, excl_row):
    """(float64 dict, the mode's tolerance terms, softmax_loss_ref's own terms: the target's score takes no offset) for
    scale = 1 and an upstream gradient of 1, on the case's tables and these query rows."""
    args = (target, c["inv_temp"], 1.0, c["ptr"], c["items"], excl_row)
    if c["mode"] == "full":
        ref = R.softmax_loss_np(Q, c["I"], *args)
    elif c["mode"] == "cand":
        ref = C.softmax_loss_cand_np(Q, c["I"], c["cand"], *args)
    else:
        ref = P.softmax_loss_pop_np(Q, c["I"], c["cand"], c["bias"], *args)
    plain = R.tolerance_terms(Q, c["I"], target, ref, c["inv_temp"], 1.0)
    terms = P.tolerance_terms(Q, c["I"], target, ref, c["inv_temp"], 1.0) if c["mode"] == "bias" else plain
    return ref, terms, plain


@functools.lru_cache(maxsize=None)
def case(*key, **kw):
    """build() computed once per process and shared, without the [rows, n_items] arrays of the reference."""
    c = build(*key, **kw)
    c["ref"] = {k: v for k, v in c["ref"].items() if k not in ("p", "eligible", "off")}
    return c


def loss_tolerance(c, K_LSE):
    """test_gpu_softmax_negs._check's: |scale| sum_b 2 K_LSE unit_b + 4 eps32 |loss|, at scale = 1."""
    return float((2 * K_LSE * c["terms"]["lse"][0]).sum() + 4 * R.EPS32 * abs(c["ref"]["loss"]))


def needs(c, got):
    """The K each output of `got` needs against the case's reference: lse, tscore, dQ and the full-size dI, the
    gradients per unit of the upstream gradient (got holds them for g = 1)."""
    ref, terms = c["ref"], c["terms"]
    need = {k: R.worst_ratio(got[k], ref[k], *terms[k]) for k in ("lse", "dQ", "dI")}
    need["tscore"] = R.worst_ratio(got["tscore"], ref["tscore"], c["plain"]["lse"][0] / c["inv_temp"], 0.0)
    return need


def float32_eval(c):
    """The case in float32 torch on the CPU: logsumexp over the masked (and offset) logits, the gradients by autograd."""
    ref = c["ref"]
    el, off = ref["eligible"], ref.get("off", np.zeros(ref["eligible"].shape))
    q, i = torch.from_numpy(c["Q"]).requires_grad_(True), torch.from_numpy(c["I"]).requires_grad_(True)
    loss = P.torch_softmax_loss_pop(q, i, c["target"], c["inv_temp"], 1.0, el, off)
    assert loss.dtype == torch.float32
    loss.backward()
    ok = torch.as_tensor(el.any(1))
    with torch.no_grad():
        z = (q @ i.T) * np.float32(c["inv_temp"])
        shift = torch.as_tensor(off, dtype=torch.float32).masked_fill(~torch.as_tensor(el), float("-inf"))
        lse = torch.where(ok, torch.logsumexp(torch.where(ok[:, None], z + shift, torch.zeros_like(z)), dim=1), torch.zeros(len(q)))
        t = torch.as_tensor(np.where(el.any(1), c["target"], 0))
        tscore = torch.where(ok, (q * i[t]).sum(1), torch.zeros(len(q)))
    return {"loss": float(loss.detach()), "lse": lse.numpy(), "tscore": tscore.numpy(), "dQ": q.grad.numpy(), "dI": i.grad.numpy()}
