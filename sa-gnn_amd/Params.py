"""Flag system with the reference's names and defaults (reference Params.py:3-53).

Differences, all host-side: flags are declared from one table; `args` is built from defaults at
import and main.py applies the command line through `parse_args(argv)` — the reference parses
sys.argv at import time (Params.py:52), which breaks any importer that owns argv (pytest,
torchrun). Flags the reference never reads are still accepted so its *.sh lines run unchanged.
"""
from __future__ import annotations

import argparse

# name, type, default, help[, choices]
_FLAGS = [
    ("lr", float, 1e-3, "learning rate"),
    ("batch", int, 512, "batch size"),
    ("testbatch", int, 64, "unused by the reference"),
    ("reg", float, 1e-5, "weight decay regularizer"),
    ("epoch", int, 100, "number of epochs"),
    ("graphNum", int, 8, "T: number of time-interval graphs"),
    ("decay", float, 0.96, "learning-rate decay"),
    ("save_path", str, "tem", "checkpoint / history name"),
    ("latdim", int, 64, "d: embedding size"),
    ("ssldim", int, 32, "SSL meta-net width"),
    ("rank", int, 4, "unused"),
    ("memosize", int, 2, "unused"),
    ("sampNum", int, 40, "unused"),
    ("testSize", int, 100, "candidates per test user"),
    ("sslNum", int, 20, "SSL pairs per user"),
    ("query_vector_dim", int, 64, "AdditiveAttention width: read under --seqPool additive (a multiple of 32 in [32, 256]); constructed "
                                   "and never applied in the reference and under --seqPool sum"),
    ("num_attention_heads", int, 16, "MHSA heads"),
    ("hyperNum", int, 128, "unused"),
    ("gnn_layer", int, 2, "L: GNN layers per interval"),
    ("trnNum", int, 10000, "training users per epoch"),
    ("load_model", str, None, "checkpoint to resume"),
    ("shoot", int, 10, "K of top-K"),
    ("data", str, "yelp", "dataset directory name"),
    ("target", str, "buy", "unused"),
    ("deep_layer", int, 0, "unused"),
    ("mult", float, 100, "unused"),
    ("keepRate", float, 0.5, "dropout keep probability"),
    ("slot", float, 1, "days per time bucket of --edgeTime slot: an interaction at time t falls in bucket "
                       "(t - earliest) // (86400 * slot); unread under --edgeTime none, as in the reference, whose "
                       "timeProcess call is commented out"),
    ("graphSampleN", int, 15000, "dead code only"),
    ("divSize", int, 10000, "unused"),
    ("tstEpoch", int, 3, "test every N epochs"),
    ("subUsrSize", int, 10, "unused"),
    ("subUsrDcy", float, 0.9, "unused"),
    ("leaky", float, 0.5, "leaky-ReLU slope"),
    ("hyperReg", float, 1e-4, "unused"),
    ("temp", float, 1, "unused"),
    ("ssl_reg", float, 1e-4, "SSL loss weight"),
    ("percent", float, 0.0, "noise percentage"),
    ("pos_length", int, 200, "max sequence length"),
    ("att_size", int, 12000, "unused"),
    ("att_layer", int, 4, "sequence attention layers"),
    ("pred_num", int, 5, "prediction targets sampled in training"),
    ("nfs", bool, False, "unused"),
    ("test", bool, True, "test (True) or validation"),
    ("ssl", bool, True, "unused"),
    ("uid", int, 0, "debug print index"),
    ("full_rank", int, 0, "also report HR / NDCG over the full item catalogue (not in the reference)"),
    ("sampler", str, "host", "where training batches are drawn: host (numpy) or device (seeded HIP kernels; not in "
                             "the reference)", ("host", "device")),
    ("evaluator", str, "host", "where test epochs score and rank: host (numpy ranking per batch) or device (tables "
                               "built once, ranks copied back once per epoch; not in the reference)", ("host", "device")),
    ("fusion_rows", str, "all", "rows the training step's interval fusion runs on: all (every user and item) or batch "
                                "(only the rows the loss reads; the same loss and gradients, but dropout masks are drawn "
                                "for those rows only, so a seeded run reproduces within a mode, not across modes; not in "
                                "the reference)", ("all", "batch")),
    ("edgeKeepRate", float, 1.0, "keep probability of the edge dropout on the interval graphs in training steps, in "
                                 "(0, 1]; 1 = off. Not in the reference: its edgeDropout rewrites edge values that "
                                 "messagePropagate never reads, so the op is dead there and --keepRate only reaches the "
                                 "LSTM's output dropout"),
    ("adjNorm", str, "none", "normalisation of the interval adjacencies: none (the unweighted sum the reference's graph "
                             "computes) or sym (edge (u, i) weighs 1 / sqrt(deg_u * deg_i), on every entry point, "
                             "training and inference). Not in the reference's graph: transToLsts(norm=True) computes "
                             "these values (DataHandler.py:53-59) but they are cast to int32 and never read",
     ("none", "sym")),
    ("seqAtt", str, "sum", "what the head's attention layers see of the user's item sequence: sum (the masked sum "
                           "collapses the sequence into one token, as the reference's graph computes) or full (every "
                           "item of the sequence is a token and the layers attend over the real items, padding masked; "
                           "same variables; needs latdim / num_attention_heads in {2, 4, 8} and pos_length <= 256; "
                           "--seqHeads gives these layers a head count of their own, up to a head width of 64). Not "
                           "in the reference's graph: it multiplies the mask in before the attention layers "
                           "(model.py:161-162) and never passes attn_mask (Utils/attention.py:35-45). The causal form of full "
                           "is chosen with --seqMask causal",
     ("sum", "full")),
    ("seqMask", str, "none", "the mask of --seqAtt full's attention: none (every token of a slot attends to every token of "
                             "the slot) or causal (a token attends to itself and the tokens before it only, what training "
                             "on every position, --seqTargets all, needs; same variables and limits as full). --seqAtt "
                             "full --seqMask causal selects the head form the model knows, stores in checkpoints and "
                             "checks on load as seqAtt causal (args.seqAtt == \"causal\"), so a full checkpoint is "
                             "refused under it and the reverse; it needs --seqAtt full. Not in the reference, which "
                             "never passes an attention mask",
     ("none", "causal")),
    ("seqHeads", int, 0, "the head count of --seqAtt full's attention layers: 0 follows --num_attention_heads, H > 0 gives "
                         "the sequence head H heads of its own while the interval fusion keeps --num_attention_heads "
                         "(SASRec-style heads: 1 or 2 at latdim 64); needs --seqAtt full (with or without --seqMask "
                         "causal), H a divisor of latdim and latdim / H in {2, 4, 8, 16, 32, 64}; widths 16 to 64 run on the "
                         "fp32 matrix cores; same variables; part of the model (stored in checkpoints, checked on load). "
                         "Not in the reference"),
    ("seqFFN", int, 0, "the hidden width F of a position-wise feed-forward block after each of --seqAtt full's attention "
                       "layers: x + act(LN(x) W1 + b1) W2 + b2 per real token, the second half of a SASRec block (0 = off, "
                       "the head as it was); six more variables per attention layer (seq_ffn{i}_*), none L2-regularised; "
                       "part of the model (stored in checkpoints, checked on load); needs --seqAtt full (with or without "
                       "--seqMask causal), latdim in {32, 64, 128}, F a multiple of 16 in [16, 256] with latdim * F <= "
                       "16384 and pos_length <= 256; one fused ragged kernel family on the fp32 matrix cores; no dropout "
                       "inside the block. Not in the reference"),
    ("seqTargets", str, "last", "which next-item events of a slot's sequence the head trains on: last (the slot's pooled row "
                                "against its one sampled positive, as the reference's graph computes, model.py:161-168: one "
                                "collapsed token, one target) or all (every real token a query: the running sum of the "
                                "tokens up to it against the item that follows it, the sampled positive after the last; as "
                                "many loss terms as tokens, averaged; a slot with a positive and no tokens contributes "
                                "nothing, under last it contributes one term; needs --seqAtt full --seqMask causal, --seqPool sum and "
                                "--predLoss softmax; a training flag, not part of the model). Not in the reference",
     ("last", "all")),
    ("seqPool", str, "sum", "how the head pools the tokens of --seqAtt full into the user's row: sum (the plain sum over "
                            "the real tokens, as the reference's graph computes) or additive (the softmax-weighted sum of "
                            "additive attention, weights from <tanh(x Wa + ba), v>; three more variables of width "
                            "--query_vector_dim; part of the model; needs --seqAtt full and latdim, query_vector_dim "
                            "multiples of 32). Not in the reference's graph: it constructs the AdditiveAttention "
                            "(model.py:147) and comments its call out (model.py:168)", ("sum", "additive")),
    ("rnnCell", str, "lstm", "the recurrent cell of the interval fusion: lstm (BasicLSTMCell, what the reference's graph "
                             "runs) or gru (TF 1.14 GRUCell: kernels [2d, 2d] and [2d, d] in place of the LSTM's [2d, 4d], "
                             "one state; part of the model; exact fp32 under every engine; needs latdim a multiple of 32 up "
                             "to 256; not with the interval-parallel path). Not in the reference's graph: it builds the cell "
                             "in a function named gru_cell() that returns BasicLSTMCell (model.py:135-136)", ("lstm", "gru")),
    ("predLoss", str, "hinge", "the training loss of the prediction head: hinge (one positive against 40 sampled "
                               "negatives, the reference's loss) or softmax (cross-entropy of the user's next item "
                               "against every item the sampler may draw as its negative, over the whole catalogue; the "
                               "same variables, so checkpoints carry over; needs --fusion_rows all, or --softmaxNegs > 0, "
                               "and latdim in {32, 64, 128}). Not in the reference, which has the sampled hinge loss only "
                               "(model.py:241-246)", ("hinge", "softmax")),
    ("edgeTime", str, "none", "time inside the interval graphs: none (an edge's timestamp only decides which interval graph "
                              "holds it, as the reference's graph computes) or slot (every message adds the row of "
                              "timeEmbed @ W its edge's --slot-day bucket selects, W the [d, d] weight of that "
                              "messagePropagate call, on every entry point, training and inference; part of the model; "
                              "needs --edgeKeepRate 1). Not in the reference's graph: it defines timeEmbed and the "
                              "weights (model.py:81, :117) and comments the term out (model.py:86)", ("none", "slot")),
    ("softmaxTemp", float, 1.0, "temperature of --predLoss softmax: the logits are <q, item> / softmaxTemp, > 0 (not in "
                                "the reference)"),
    ("softmaxNegs", int, 0, "candidates of --predLoss softmax: 0 (the whole catalogue) or N > 0 (the softmax runs over N "
                            "items drawn per step on the device, one uniformly from each of N equal strata of the "
                            "catalogue and shared by the batch, minus the user's banned items, plus the slot's own "
                            "target; N <= the item count; lifts the need for --fusion_rows all; not part of the model). "
                            "Not in the reference, which has the sampled hinge loss only (model.py:241-246)"),
    ("softmaxNegDist", str, "uniform", "how the --softmaxNegs candidates are drawn: uniform (one from each of N equal strata "
                                       "of the catalogue; the reported loss is lower than the full-catalogue one by about "
                                       "ln(items / N)) or pop (N draws with replacement in proportion to (train degree + 1)"
                                       "^softmaxNegPow, each distinct item's logit corrected by ln(times drawn / expected "
                                       "draws), the logQ correction of sampled softmax: the loss estimates the "
                                       "full-catalogue one; needs --predLoss softmax and --softmaxNegs > 0; not part of "
                                       "the model). Not in the reference", ("uniform", "pop")),
    ("softmaxNegPow", float, 0.75, "exponent a of --softmaxNegDist pop, 0 <= a <= 1: 0 draws uniformly with replacement, 1 "
                                   "in proportion to the degree, 0.75 is word2vec's; read only under pop (not in the "
                                   "reference)"),
]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Model Params")
    for name, typ, default, text, *choices in _FLAGS:
        # type=bool keeps the reference's semantics: any non-empty string is True (Params.py:47-49)
        p.add_argument("--" + name, default=default, type=typ, help=text, choices=choices[0] if choices else None)
    return p


def parse_args(argv=None, namespace=None):
    parser = build_parser()
    ns = parser.parse_args([] if argv is None else argv, namespace)
    if ns.seqMask == "causal":                     # the causal form of full is the head form seqAtt "causal" (model.SEQ_ATT)
        if ns.seqAtt not in ("full", "causal"):
            parser.error(f"--seqMask causal needs --seqAtt full (got --seqAtt {ns.seqAtt})")
        ns.seqAtt = "causal"
    ns.decay_step = ns.trnNum // ns.batch          # reference Params.py:53
    return ns


args = parse_args([])
# args.user / args.item are injected by DataHandler.LoadData (reference DataHandler.py:126)
