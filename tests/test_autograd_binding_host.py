"""The checked wrappers autograd.py calls (ops.lstm_fwd_train ... ops.hinge), on the host: every one of them refuses host
tensors, wrong counts, wrong widths and half-given argument groups before it reaches the library, and autograd.py itself
holds no raw library call.

"Before it reaches the library" is tested, not assumed: `no_library` replaces _lib.load with a function that raises
Reached, so a wrapper that got past its checks ends in Reached and not in the expected TypeError / ValueError. The shape
cases run on host tensors of a subclass that answers is_cuda = True (the wrappers' device check is `t.is_cuda`): with it
a VALID call walks through every check and ends in Reached, which is the control that the rejections below come from the
argument under test and from nothing else."""
import pytest
import torch

from sa_gnn_amd import autograd as ag
from sa_gnn_amd import ops

N, T, D, HEADS = 3, 2, 8, 2          # nodes, intervals, width
NU, NI, NL, P = 7, 9, 4, 5           # user / item / slot table rows, pairs
K, KP = 5, 8                         # row-dot columns read / stored


class Reached(Exception):
    """The call got past the wrapper's checks and asked for the library."""


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise Reached
    monkeypatch.setattr(ops._lib, "load", load)


class _OnDevice(torch.Tensor):
    is_cuda = property(lambda self: True)


def on_device(t):
    return torch.Tensor._make_subclass(_OnDevice, t)


def host(t):
    return t


def calls(put):
    """A valid call of every new wrapper: name -> (function, positional arguments), tensors made through `put`."""
    f = lambda *shape: put(torch.zeros(shape))                       # noqa: E731
    i = lambda n: put(torch.zeros(n, dtype=torch.int32))             # noqa: E731
    attn = (f(D, D), f(D), f(D, D), f(D), f(D, D), f(D))
    return {
        "lstm_fwd_train": (ops.lstm_fwd_train, [f(N, T, D), f(2 * D, 4 * D), f(4 * D)]),
        "lstm_bwd": (ops.lstm_bwd, [f(N, T, D), f(N, T, D), f(N, T, 4 * D), f(N, T, D), f(N, T, D), f(N, T, D), f(2 * D, 4 * D),
                                    True]),
        "lstm_bwd_step": (ops.lstm_bwd_step, [f(N, T, 4 * D), f(N, T, D), f(N, T, D), f(N, T, D), f(N, D), f(N, D), f(N, 4 * D),
                                              f(N, D), 0]),
        "attn_bwd_front": (ops.attn_bwd_front, [f(N, T, D), f(D), f(D), *attn, HEADS, f(N, D)]),
        "attn_bwd": (ops.attn_bwd, [f(N * T, 3 * D), f(N, D), N, T, HEADS]),
        "attn_bwd_tail": (ops.attn_bwd_tail, [f(N * T, D), f(N * T, 3 * D), f(D, 3 * D), f(D, 3 * D), f(3 * D)]),
        "layernorm_td_bwd": (ops.layernorm_td_bwd, [f(N, T, D), f(N, T, D), f(D)]),
        "leaky": (ops.leaky, [f(N, D), 0.5]),
        "leaky_bwd": (ops.leaky_bwd, [f(N, D), f(N, D), 0.5]),
        "pair_score_bwd": (ops.pair_score_bwd, [f(NU, D), f(NI, D), i(P), i(P), f(P), f(NL, D), f(NI, D), i(P), 0.5]),
        "prod_leaky_sum": (ops.prod_leaky_sum, [f(NU, D), f(NI, D), i(P), i(P), 0.5]),
        "prod_leaky_sum_bwd": (ops.prod_leaky_sum_bwd, [f(NU, D), f(NI, D), i(P), i(P), 0.5, f(P)]),
        "meta_features": (ops.meta_features, [f(NU, D), f(NU, D), i(P)]),
        "meta_features_bwd": (ops.meta_features_bwd, [f(NU, D), f(NU, D), i(P), f(P, 3 * D)]),
        "rowdot_sigmoid": (ops.rowdot_sigmoid, [f(P, KP), f(K), f(1), K]),
        "rowdot_sigmoid_bwd": (ops.rowdot_sigmoid_bwd, [f(P, KP), f(K), f(P), f(P), K]),
        "hinge": (ops.hinge, [f(P), f(P), f(P), f(P), f(P), f(P), 1.0]),
    }


NAMES = sorted(calls(host))

f32 = lambda *shape: on_device(torch.zeros(shape))                   # noqa: E731
i32 = lambda n: on_device(torch.zeros(n, dtype=torch.int32))         # noqa: E731
i64 = lambda n: on_device(torch.zeros(n, dtype=torch.int64))         # noqa: E731

# (wrapper, position of the argument, what it is replaced by, the error, a word of its message)
BAD = [
    ("lstm_fwd_train", 0, f32(N, T, D + 1)[:, :, :D].transpose(1, 2), ValueError, "x"),           # feature stride not 1
    ("lstm_fwd_train", 1, f32(2 * D, 4 * D + 1), ValueError, "W"),
    ("lstm_fwd_train", 2, f32(2 * D), ValueError, "b"),
    ("lstm_bwd", 1, f32(N + 1, T, D), ValueError, "h"),
    ("lstm_bwd", 2, f32(N, T, D), ValueError, "gates"),
    ("lstm_bwd", 3, f32(N, T, 2 * D), ValueError, "cell"),
    ("lstm_bwd", 4, f32(T, N, D).permute(1, 0, 2), ValueError, "dh"),                             # (t, d) block not contiguous
    ("lstm_bwd", 4, f32(N, T + 1, D), ValueError, "dh"),
    ("lstm_bwd", 5, f32(N, T, D + 4), ValueError, "drop"),
    ("lstm_bwd", 6, f32(2 * D, 2 * D), ValueError, "W"),
    ("lstm_bwd_step", 0, f32(N, T, 4 * D + 2), ValueError, "gates"),
    ("lstm_bwd_step", 1, f32(N, T, 4 * D), ValueError, "cell"),
    ("lstm_bwd_step", 2, f32(N + 1, T, D), ValueError, "dh"),
    ("lstm_bwd_step", 4, None, ValueError, "go together"),
    ("lstm_bwd_step", 5, None, ValueError, "go together"),
    ("lstm_bwd_step", 4, f32(N, 2 * D), ValueError, "dh_rec"),
    ("lstm_bwd_step", 6, f32(N, D), ValueError, "dgates"),
    ("lstm_bwd_step", 7, f32(N + 1, D), ValueError, "dc_out"),
    ("attn_bwd_front", 1, None, ValueError, "go together"),
    ("attn_bwd_front", 1, f32(2 * D), ValueError, "gamma"),
    ("attn_bwd_front", 3, f32(D, 2 * D), ValueError, "Wq"),
    ("attn_bwd_front", 8, f32(2 * D), ValueError, "bv"),
    ("attn_bwd_front", 10, f32(N + 1, D), ValueError, "g_out"),
    ("attn_bwd_front", 10, f32(N, 2 * D), ValueError, "g_out"),
    ("attn_bwd", 0, f32(N * T, 3 * D + 1), ValueError, "qkv"),
    ("attn_bwd", 0, f32(N * T + 1, 3 * D), ValueError, "qkv"),
    ("attn_bwd", 1, f32(N, 2 * D), ValueError, "g_out"),
    ("attn_bwd_tail", 1, f32(N * T, 2 * D), ValueError, "dqkv"),
    ("attn_bwd_tail", 2, f32(D, D), ValueError, "Wqkv"),
    ("attn_bwd_tail", 3, f32(D, 3 * D)[:, ::2], ValueError, "dWqkv"),
    ("attn_bwd_tail", 4, f32(D), ValueError, "dbqkv"),
    ("layernorm_td_bwd", 0, f32(T, N, D).permute(1, 0, 2), ValueError, "x"),                      # one node stride only
    ("layernorm_td_bwd", 1, f32(N, T, 2 * D), ValueError, "g"),
    ("layernorm_td_bwd", 2, f32(2 * D), ValueError, "gamma"),
    ("leaky", 0, f32(N, 2 * D)[:, :D], ValueError, "a"),
    ("leaky_bwd", 1, f32(N + 1, D), ValueError, "g"),
    ("pair_score_bwd", 0, f32(NU, 2 * D)[:, ::2], ValueError, "U"),
    ("pair_score_bwd", 1, f32(NI, 2 * D), ValueError, "I"),
    ("pair_score_bwd", 3, i32(P + 1), ValueError, "iids"),
    ("pair_score_bwd", 4, f32(P + 1), ValueError, "g"),
    ("pair_score_bwd", 5, None, ValueError, "go together"),
    ("pair_score_bwd", 6, None, ValueError, "go together"),
    ("pair_score_bwd", 7, None, ValueError, "go together"),
    ("pair_score_bwd", 5, f32(NL, 2 * D), ValueError, "S"),
    ("pair_score_bwd", 2, i64(P), TypeError, "uids"),
    ("pair_score_bwd", 7, i32(2 * P)[::2], TypeError, "locs"),
    ("prod_leaky_sum", 1, f32(NI, 2 * D), ValueError, "Y"),
    ("prod_leaky_sum", 3, i32(P - 1), ValueError, "iids"),
    ("prod_leaky_sum", 2, i64(P), TypeError, "uids"),
    ("prod_leaky_sum_bwd", 0, f32(NU, D, 1), ValueError, "X"),
    ("prod_leaky_sum_bwd", 5, f32(P - 1), ValueError, "g"),
    ("prod_leaky_sum_bwd", 3, i64(P), TypeError, "iids"),
    ("meta_features", 1, f32(NU + 1, D), ValueError, "V"),
    ("meta_features", 1, f32(NU, 2 * D), ValueError, "V"),
    ("meta_features", 2, i64(P), TypeError, "uids"),
    ("meta_features_bwd", 3, f32(P, 2 * D), ValueError, "dm"),
    ("meta_features_bwd", 3, f32(P + 1, 3 * D), ValueError, "dm"),
    ("rowdot_sigmoid", 0, f32(P, K - 1), ValueError, "A"),
    ("rowdot_sigmoid", 1, f32(KP), ValueError, "w3"),
    ("rowdot_sigmoid", 2, f32(2), ValueError, "b3"),
    ("rowdot_sigmoid_bwd", 2, f32(P + 1), ValueError, "w"),
    ("rowdot_sigmoid_bwd", 3, f32(P - 1), ValueError, "dw"),
    ("hinge", 1, f32(P + 1), ValueError, "neg"),
    ("hinge", 2, None, ValueError, "go together"),
    ("hinge", 5, None, ValueError, "go together"),
    ("hinge", 4, f32(P + 1), ValueError, "sp"),
]


def test_every_wrapper_has_a_rejected_shape():
    assert {b[0] for b in BAD} == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_host_tensors_are_refused_before_the_library(no_library, name):
    fn, args = calls(host)[name]
    with pytest.raises(TypeError, match="device tensor"):
        fn(*args)


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_passes_every_check(no_library, name):
    """The control of the cases below: nothing else about these arguments stops a call short of the library."""
    fn, args = calls(on_device)[name]
    with pytest.raises(Reached):
        fn(*args)


@pytest.mark.parametrize("name,pos,value,error,word", BAD, ids=[f"{b[0]}-{b[1]}-{k}" for k, b in enumerate(BAD)])
def test_mismatches_are_refused_before_the_library(no_library, name, pos, value, error, word):
    fn, args = calls(on_device)[name]
    args[pos] = value
    with pytest.raises(error, match=word if " " in word else f"^{word}:"):        # the message names the argument
        fn(*args)


def test_operands_on_two_devices_are_refused(no_library):
    """`device` is what _one_device compares: a tensor that answers another one is refused by name."""
    class Elsewhere(_OnDevice):
        device = property(lambda self: torch.device("meta"))
    fn, args = calls(on_device)["pair_score_bwd"]
    args[4] = torch.Tensor._make_subclass(Elsewhere, torch.zeros(P))
    with pytest.raises(ValueError, match="g on meta"):
        fn(*args)


def test_the_support_queries_answer_on_the_host():
    assert ops.lstm_bwd_supported(64) and not ops.lstm_bwd_supported(128)
    assert ops.attn_bwd_tail_supported(32) and not ops.attn_bwd_tail_supported(128)
    assert ops.attn_bwd_front_supported(64, 2, 16) and not ops.attn_bwd_front_supported(64, 7, 16)
    assert ops.lstm_bwd_workspace_bytes(3, 2, 32) == 3 * 2 * 4 * 32 * 4


def test_autograd_holds_no_raw_library_call():
    with open(ag.__file__) as f:
        text = f.read()
    for word in ("sagnn_", "data_ptr", "ops._"):
        assert word not in text, f"autograd.py contains {word!r}: the library is called through ops' public wrappers only"
