"""The float64 training objective under COMBINED opt-in flags, composed from the restatements the
per-flag tests use. Nothing here restates a formula: every piece is another module's, selected by the flags and wired
together. No GPU and no kernel of the package is touched; what the model itself must supply (its variables, the banned
table) comes in as arguments.

The non-default values, one letter each:

  G --rnnCell gru        N --adjNorm sym        T --edgeTime slot      E --edgeKeepRate 0.5    F --seqAtt full
  A --seqPool additive   S --predLoss softmax   B --fusion_rows batch  D output dropout with keep 0.5 (explicit masks)
  K --softmaxNegs 16     P --softmaxNegDist pop (softmaxNegPow 0.75)   C --seqAtt causal      L --seqTargets all

Refused by Recommender.prepareModel / train_loss: T with E, S with B unless K, A without F or C, K without S, P without K,
L without C or without S or with A. C and F are two values of one flag.

  GNN interval   one replacement for O.torch_gnn_interval: the dense terms of edge_time_ref through its stack (T), the
                 dense_sym weights of adj_norm_ref (N) or the oracle's index lists as counts, times the per-layer,
                 per-direction masks of edge_drop_ref scaled by float32(1) / float32(keep) (E)
  cell           gru_ref.torch_gru in place of O.torch_basic_lstm (G); the four leaves travel as the lstm_W tuple
  head           the oracle's collapsed head, seq_att_ref.torch_head_ragged (F), seq_causal_ref.torch_head_causal (C),
                 seq_pool_ref.torch_head_additive (FA) or seq_causal_ref.torch_head_slabs pooled by seq_pool_ref.pool_tokens_t (CA)
  loss           the oracle's hinge, seq_att_ref.torch_train_loss_full (F, C), softmax_loss_ref.torch_train_loss_softmax (S;
                 K: over the banned table augmented by softmax_cand_ref), softmax_pop_ref.torch_train_loss_pop (P) or
                 seq_causal_ref.torch_train_loss_all (L, with the step's candidates and offsets under K / P)
  candidates     the step's list under K / P: softmax_cand_ref.strata or softmax_pop_ref.draw over the model's own item
                 mass (model.pop_cum of model.item_degrees) under the fixed CAND_SEED; the GPU suite checks that the
                 device draws the same list
  dropout        batch["drop_u"] / batch["drop_i"], full-size {0, 1 / keep} scales, read by O.torch_train_loss (D)

The two patches of the oracle module are applied through the `patch` callable the caller hands in (a test's
monkeypatch.setattr): they stay run-time patches inside the tests."""
import itertools

import numpy as np
import torch

import adj_norm_ref as N
import edge_drop_ref as D
import edge_time_ref as ET
import fusion_rows_ref as FR
import gru_ref as G
import seq_att_ref as SA
import seq_causal_ref as SC
import seq_pool_ref as SP
import softmax_cand_ref as CAND
import softmax_loss_ref as SL
import softmax_pop_ref as POP
from oracle import selfgnn_oracle as O

LETTERS = "GNTEFASBDKPCL"
ON = {"G": {"rnnCell": "gru"}, "N": {"adjNorm": "sym"}, "T": {"edgeTime": "slot"}, "E": {"edgeKeepRate": 0.5},
      "F": {"seqAtt": "full"}, "A": {"seqPool": "additive"}, "S": {"predLoss": "softmax"}, "B": {"fusion_rows": "batch"},
      "D": {},                                            # D is not a flag of the model: the masks travel in the batch
      "K": {"softmaxNegs": 16}, "P": {"softmaxNegDist": "pop", "softmaxNegPow": 0.75}, "C": {"seqAtt": "causal"},
      "L": {"seqTargets": "all"}}
DEFAULTS = {"rnnCell": "lstm", "adjNorm": "none", "edgeTime": "none", "edgeKeepRate": 1.0, "seqAtt": "sum", "seqPool": "sum",
            "predLoss": "hinge", "fusion_rows": "all", "query_vector_dim": 32, "softmaxTemp": 0.5, "slot": 5.0,
            "softmaxNegs": 0, "softmaxNegDist": "uniform", "softmaxNegPow": 0.75, "seqTargets": "last"}
KEEP = 0.5                                                # E's edge keep rate and D's output keep rate
EDGE_SEED = (0x1234_5678_9ABC_DEF, 5)                     # test_gpu_edge_drop.py's (SEED, STEP)
CAND_SEED = (77, 3)                                       # test_gpu_seq_causal._compare_all's (seed, step) of the candidate draw
ADD_NAMES = ("additive_attention0_kernel", "additive_attention0_bias", "additive_attention0_query")
GRU_NAMES = ("rnn_gru_gates_kernel", "rnn_gru_gates_bias", "rnn_gru_candidate_kernel", "rnn_gru_candidate_bias")

# case -> (flags on, latdim): the pairwise cover of DESIGN.md §23
CASES = {1: ("GNTFASD", 64),     # fused GRU, weighted + time SpMM, softmax through the additive pool
         2: ("GNEFABD", 32),     # fused GRU, drop + weighted SpMM, compacted rows, hinge
         3: ("TBD", 32),         # LSTM, unweighted time form under compacted rows
         4: ("GSE", 128),        # per-step GRU route, softmax with edge drop, collapsed head
         # the four newer flags (K, P, C, L): every legal pair that holds one of them
         5: ("GNTCLSKPD", 64),   # every position against popularity candidates: the target scatter into the weighted + time SpMM
         6: ("ECLSKBD", 32),     # every position against uniform candidates under compacted rows and edge drop
         7: ("NFASKPB", 32),     # the candidate loss through the additive pool into compacted rows, LSTM
         8: ("GECASKP", 128)}    # causal attention under the additive pool, popularity draw next to edge drop

# case -> the leaves at which float32 on the CPU is itself not within a quarter of the gradient tolerance
# (test_flag_combo_host.py measures them; the GPU suite judges these, by name, at four times the float32 error)
F32_EXCEPTIONS = {1: (), 2: (), 4: (), 5: (), 6: (), 7: (), 8: (),
                  # the unnormalised time form on the x 20 embeddings feeds the LSTM values in the hundreds: the whole user
                  # side of the fusion (float32 at 0.29 .. 0.94 of the tolerance); the two SSL biases (0.21, 0.18) are
                  # named so that another machine's float32 rounding cannot fail the CPU check: a name widens nothing
                  # at a leaf that holds the quarter
                  3: ("uEmbed", "iEmbed", "timeEmbed", "defaultParamName1", "defaultParamName2", "defaultParamName3",
                      "defaultParamName5", "defaultParamName6", "defaultParamName7", "rnn_lstm_kernel", "rnn_lstm_bias",
                      "LayerNorm_gamma", "LayerNorm_beta", "mhsa1_q_kernel", "mhsa1_q_bias", "mhsa1_k_kernel", "mhsa1_v_kernel",
                      "mhsa1_v_bias", "meta2", "meta3", "meta2Bias", "meta3Bias")}


def illegal(letters) -> bool:
    """What Recommender.prepareModel refuses (and F with C, which one flag cannot say)."""
    on = set(letters)
    return ({"T", "E"} <= on or {"F", "C"} <= on or ("A" in on and not on & {"F", "C"})
            or ("K" in on and "S" not in on) or ("P" in on and "K" not in on)
            or ("L" in on and (not {"C", "S"} <= on or "A" in on))
            or ({"S", "B"} <= on and "K" not in on))


def legal_pairs():
    """Every pair of non-default values that some legal set holds (A's pairs come with the F or C it needs, K's with S, ...):
    the pair is legal when one of the sets around it is."""
    rest = lambda a, b: [c for c in LETTERS if c not in a + b]
    return [a + b for a, b in itertools.combinations(LETTERS, 2)
            if any(not illegal(a + b + "".join(extra)) for n in range(len(LETTERS) - 1) for extra in itertools.combinations(rest(a, b), n))]


def model_flags(letters, latdim) -> dict:
    """The args values of a flag set (every switch named, so that a default cannot leak in from an earlier test)."""
    flags = dict(DEFAULTS, latdim=latdim)
    for c in letters:
        flags.update(ON[c])
    return flags


def all_leaves(P_leaves, params, dtype=torch.float64) -> dict:
    """The leaves of an _oracle_params call, completed to one leaf per registered variable."""
    leaves = dict(P_leaves)
    for name, v in params.items():
        if name not in leaves:
            leaves[name] = v.detach().cpu().to(dtype).requires_grad_(True)
    return leaves


def time_names(rec, params):
    """["timeEmbed", the 2 T L time weights in registration order]."""
    return ["timeEmbed"] + [k for w in rec.time_weights for k, v in params.items() if v is w]


def output_drop(letters, batch, n_users, n_items, T, d, P=None, seq_items=None, seed=4):
    """D: (masks for the device side, the same values full-size for the oracle), {0, 1 / KEEP} float32 [rows, T, d]. Under
    B the device side gets the rows of the compacted slots, i.e. of the touched rows in ascending order
    (fusion_rows_ref.touched_rows): what train_loss draws for itself there; the oracle reads the full-size table, whose
    other rows no loss term reaches."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    full = {key: (torch.rand((n, T, d), generator=g) < KEEP).float() / KEEP for key, n in (("drop_u", n_users), ("drop_i", n_items))}
    dev = dict(full)
    if "B" in letters:
        users, items, _ = FR.touched_rows(batch, n_users, n_items, P, seq_items)
        assert len(users) and len(items)
        dev = {"drop_u": full["drop_u"][torch.from_numpy(users)], "drop_i": full["drop_i"][torch.from_numpy(items)]}
    return dev, full


def gnn_interval(letters, mats, te=None, slot_info=None, edge_seed=EDGE_SEED):
    """The replacement for O.torch_gnn_interval under N / T / E, or None where the oracle's own applies;
    torch_train_loss calls it for k = 0, 1, ... in order. te: the time tables [T, L, 2, M, d]; slot_info = (mi, slot, M)."""
    on = set(letters)
    if not on & set("NTE"):
        return None
    norm = "sym" if "N" in on else "none"
    calls = []

    def interval(u0, i0, adj_idx, tp_idx, n_layers, leaky):
        k = len(calls)
        calls.append(k)
        cast = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(u0.dtype)
        U, I = u0.shape[0], i0.shape[0]
        if "T" in on:
            mi, slot, M = slot_info
            terms = tuple(cast(x) for x in ET.dense_terms(mats[k], mi, slot, M, norm))
            ou, oi = ET.stack([terms], u0[None], i0[None], te[k][None], n_layers, leaky)
            return ou[0], oi[0]
        if norm == "sym":
            au = N.dense_sym(mats[k])
            ai = au.T
        else:
            au, ai = np.zeros((U, I)), np.zeros((I, U))
            np.add.at(au, (np.asarray(adj_idx)[:, 0], np.asarray(adj_idx)[:, 1]), 1.0)
            np.add.at(ai, (np.asarray(tp_idx)[:, 0], np.asarray(tp_idx)[:, 1]), 1.0)
        if "E" not in on:
            return N.torch_interval(cast(au), cast(ai), u0, i0, n_layers, leaky)
        seed, step = edge_seed
        scale = float(np.float32(1.0) / np.float32(KEEP))
        eu, ei = [u0], [i0]
        for l in range(n_layers):                         # the recurrence of adj_norm_ref.torch_interval, a mask per layer
            mu = cast(scale * au * D.dense_mask(seed, step, k, l, 0, U, I, keep=KEEP))
            mt = cast(scale * ai * D.dense_mask(seed, step, k, l, 1, U, I, keep=KEEP).T)
            nu, ni = ET.leaky_max(mu @ ei[-1], leaky) + eu[-1], ET.leaky_max(mt @ eu[-1], leaky) + ei[-1]
            eu.append(nu)
            ei.append(ni)
        return sum(eu[1:], eu[0]), sum(ei[1:], ei[0])

    interval.calls = calls
    return interval


def step_candidates(letters, handler, n_items):
    """(cand, bias) of the step under K / P as the restatements draw them (None, None without K; bias None without P)."""
    from sa_gnn_amd.model import item_degrees, pop_cum
    if "K" not in letters:
        return None, None
    n = ON["K"]["softmaxNegs"]
    if "P" not in letters:
        return CAND.strata(n_items, n, *CAND_SEED), None
    cum, _ = pop_cum(item_degrees(handler.trnMat, n_items), ON["P"]["softmaxNegPow"])
    cand, _, _, bias = POP.draw(cum, n, *CAND_SEED)
    return cand, bias


def head_causal_additive(add):
    """seq_causal_ref.torch_head_slabs ending in seq_pool_ref's additive pooling: a head= function (CA)."""
    def head(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky):
        slabs = SC.torch_head_slabs(fi, pos_embed, ln_params, att_params, sequence, mask, heads, leaky)
        return torch.stack([torch.zeros(fi.shape[1], dtype=fi.dtype) if x is None else SP.pool_tokens_t(x, *add) for x in slabs], 0)
    return head


def objective(letters, P, leaves, mats, batch, cfg, patch, names_time=None, slot_info=None, banned=None, cand=None, bias=None):
    """(preLoss, sslloss) of the flag set as differentiable torch in the dtype of the leaves. P / leaves: the oracle's
    parameter structure (test_gpu_train._oracle_params, or test_gpu_gru._oracle_params_gru under G) and one leaf per
    variable (all_leaves); mats: the interval matrices; batch: the host batch with full-size drop_u / drop_i under D;
    cfg: T, L, leaky, heads and temp; patch(module, name, value): the caller's monkeypatch.setattr; names_time:
    time_names(); slot_info = (mi, slot, M) under T; banned: banned_table(handler, n_items) under S; cand / bias:
    step_candidates() under K / P."""
    on = set(letters)
    assert not illegal(letters), letters
    dtype = leaves["uEmbed"].dtype
    batch = dict(batch)
    for key in ("drop_u", "drop_i"):
        if "D" in on:
            batch[key] = batch[key].to(dtype)
        else:
            batch.pop(key, None)
    te = None
    if "T" in on:
        T, L, d = cfg["T"], cfg["L"], leaves["timeEmbed"].shape[1]
        te = torch.matmul(leaves["timeEmbed"], torch.stack([leaves[n] for n in names_time[1:]]).view(T, L, 2, d, d))
    interval = gnn_interval(letters, mats, te, slot_info, batch.get("edge_seed", EDGE_SEED))
    if interval is not None:
        patch(O, "torch_gnn_interval", interval)
    if "G" in on:
        patch(O, "torch_basic_lstm", lambda x, W, b, forget_bias=1.0: G.torch_gru(x, *W))
    adj = [O.trans_to_lsts(m)[0] for m in mats]
    tp = [O.trans_to_lsts(O.transpose(m))[0] for m in mats]
    head = SL.torch_head_collapsed
    add = tuple(leaves[n] for n in ADD_NAMES) if "A" in on else None
    if "C" in on:
        head = head_causal_additive(add) if add else SC.torch_head_causal
    elif "A" in on:
        head = SP.torch_head_additive(add)
    elif "F" in on:
        head = SA.torch_head_ragged
    assert ("K" in on) == (cand is not None) and ("P" in on) == (bias is not None)
    if "L" in on:
        pre, ssl, _ = SC.torch_train_loss_all(P, adj, tp, batch, cfg, banned, cand, bias)
    elif "P" in on:
        pre, ssl, _, _ = POP.torch_train_loss_pop(P, adj, tp, batch, cfg, banned, cand, bias, head=head)
    elif "K" in on:             # eligibility = the candidates + the target: every other item on each user's list
        aug = CAND.augmented(len(banned[0]) - 1, mats[0].shape[1], cand, banned[0], banned[1], None)
        pre, ssl, _, _ = SL.torch_train_loss_softmax(P, adj, tp, batch, cfg, aug, head=head)
    elif "S" in on:
        pre, ssl, _, _ = SL.torch_train_loss_softmax(P, adj, tp, batch, cfg, banned, head=head)
    elif on & {"F", "C"}:
        pre, ssl, _, _ = SA.torch_train_loss_full(P, adj, tp, batch, cfg, head=head)
    else:
        pre, ssl, _, _ = O.torch_train_loss(P, adj, tp, batch, cfg)
    assert interval is None or interval.calls == list(range(cfg["T"]))
    return pre, ssl


def grad_tolerance(want, floor_extra=0.0):
    """test_gpu_seq_att._grad_close's bound as an array: 2e-4 |want| + max(5e-5 max|want|, 2e-5, floor_extra)."""
    return 2e-4 * np.abs(want) + max(5e-5 * np.abs(want).max(), 2e-5, floor_extra)


def k_bias_floor(name, grads64) -> float:
    """The sibling tests' floor of a key bias (analytically ~0): 1e-3 max|d k_kernel|; 0 for every other leaf."""
    if not name.endswith("k_bias"):
        return 0.0
    return 1e-3 * float(np.abs(grads64[name.replace("k_bias", "k_kernel")]).max())
