"""CPU suite: the device sampler's argument checks (sagnn_sample_train_i32, sagnn_sample_ssl_i32, sagnn_seq_sum_f32,
sagnn_seq_sum_bwd_f32), its random stream and negative map restated in numpy, and the host-side table builder
(model.DeviceSampler). Every library call here is rejected before any device work, so no GPU is needed."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import device_sampler_ref as R
from sa_gnn_amd import _lib


def _train(lib, p, **over):
    a = dict(bat=p, nb=8, ns=16, seq_ptr=p, seq=p, ban_ptr=p, ban=p, nu=100, ni=50, tsn=40, pred=5, P=20, off=p, npairs=64,
             seed=1, step=0, uids=p, iids=p, locs=p, segb=p, segl=p)
    a.update(over)
    return lib.sagnn_sample_train_i32(*a.values(), None)


def _ssl(lib, p, **over):
    a = dict(bat=p, nb=8, T=3, sub_ptr=p, sub=p, nu=100, ssl=20, off=p, nout=64, seed=1, step=0, uids=p, iids=p, locs=p)
    a.update(over)
    return lib.sagnn_sample_ssl_i32(*a.values(), None)


def _fwd(lib, p, **over):
    a = dict(fi=p, ldf=64, ni=50, pe=p, ldp=64, P=20, seq=p, nflat=10, segb=p, segl=p, ns=16, d=64, st=p, pt=p, ldo=64)
    a.update(over)
    return lib.sagnn_seq_sum_f32(*a.values(), None)


def _bwd(lib, p, **over):
    a = dict(gs=p, gp=p, ldg=64, seq=p, nflat=10, segb=p, segl=p, ns=16, P=20, d=64, dfi=p, lddfi=64, ni=50, dpos=p,
             lddpos=64)
    a.update(over)
    return lib.sagnn_seq_sum_bwd_f32(*a.values(), None)


def _check(fn, lib, p, cases):
    for over, code, text in cases:
        assert fn(lib, p, **over) == code, over
        assert text in _lib.last_error().lower(), (over, _lib.last_error())


@pytest.fixture(scope="module")
def buf():
    b = (ctypes.c_float * 4096)()
    return b, ctypes.addressof(b)


def test_sample_train_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    null = [(dict(**{k: None}), -1, "null input") for k in ("bat", "seq_ptr", "seq", "ban_ptr", "ban", "off")]
    null += [(dict(**{k: None}), -1, "null output") for k in ("uids", "iids", "locs", "segb", "segl")]
    _check(_train, lib, p, null + [
        (dict(nb=-1), -5, "negative count"), (dict(ns=-1), -5, "negative count"), (dict(nu=-1), -5, "negative count"),
        (dict(npairs=-1), -5, "negative count"), (dict(tsn=-1), -5, "negative count"), (dict(pred=-1), -5, "negative count"),
        (dict(nb=17), -5, "n_batch = 17 > n_slots = 16"),
        (dict(ni=0), -5, "n_items = 0"), (dict(ni=-3), -5, "n_items = -3"), (dict(ni=1 << 31), -5, "n_items"),
        (dict(P=0), -5, "pos_length = 0"), (dict(P=-2), -5, "pos_length = -2"),
        (dict(step=-1), -5, "step = -1"), (dict(step=1 << 32), -5, "step"),
    ])


def test_sample_ssl_rejects_every_invalid_argument(buf):
    lib, p = _lib.load(), buf[1]
    null = [(dict(**{k: None}), -1, "null input") for k in ("bat", "sub_ptr", "sub", "off")]
    null += [(dict(**{k: None}), -1, "null output") for k in ("uids", "iids", "locs")]
    _check(_ssl, lib, p, null + [
        (dict(nb=-1), -5, "negative count"), (dict(T=-1), -5, "negative count"), (dict(nu=-1), -5, "negative count"),
        (dict(ssl=-1), -5, "negative count"), (dict(nout=-1), -5, "negative count"),
        (dict(step=-1), -5, "step = -1"), (dict(step=1 << 32), -5, "step"),
    ])


@pytest.mark.parametrize("fn,ptrs,lds", [(_fwd, ("fi", "pe", "seq", "segb", "segl", "st", "pt"), ("ldf", "ldp", "ldo")),
                                         (_bwd, ("gs", "gp", "seq", "segb", "segl", "dfi", "dpos"), ("ldg", "lddfi", "lddpos"))])
def test_seq_sum_entries_reject_every_invalid_argument(buf, fn, ptrs, lds):
    lib, p = _lib.load(), buf[1]
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ptrs]
    cases += [(dict(d=d), -2, f"d = {d}") for d in (0, 2, 66, 260)]
    cases += [(dict(P=0), -5, "pos_length = 0"), (dict(ni=0), -5, "n_items = 0"), (dict(ns=-1), -5, "negative count"),
              (dict(nflat=-1), -5, "negative count")]
    cases += [(dict(**{k: 66}), -3, "16-byte aligned") for k in lds]
    cases += [(dict(**{k: 60}), -5, "< d = 64") for k in lds]
    feats = [k for k in ptrs if k not in ("seq", "segb", "segl")]
    cases += [(dict(**{k: p + 4}), -3, "16-byte aligned") for k in feats]
    _check(fn, lib, p, cases)
    # a valid argument set gets past the checks only with a GPU: none of the above touched one


def test_philox_known_answers():
    """Philox4x32-10 answers of the Random123 known-answer vectors; key 0 / counter 0 is also rocRAND's first output
    for seed 0 (rocrand_init(0, 0, 0) + rocrand4)."""
    def words(c, key):
        return [int(w) for w in R.philox4x32_10(*c, seed=key)]
    assert words((0, 0, 0, 0), 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert words((0xFFFFFFFF,) * 4, 0xFFFFFFFFFFFFFFFF) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0x299F31D0 << 32) | 0xA4093822) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_uniform_is_the_high_half_of_the_product():
    rng = np.random.default_rng(0)
    n = rng.integers(1, 1 << 31, size=200)
    got = R.uniform(12345, np.arange(200), 3, 7, 1, n)
    w = R.philox4x32_10(np.arange(200), 3, 7, 1, 12345)
    want = [((int(a) << 32 | int(b)) * int(m)) >> 64 for a, b, m in zip(w[0], w[1], n)]
    assert got.tolist() == want and (got >= 0).all() and (got < n).all()


def test_rth_allowed_item_matches_enumeration():
    rng = np.random.default_rng(1)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        banned = np.sort(rng.choice(n, size=int(rng.integers(0, n)), replace=False))
        allowed = np.setdiff1d(np.arange(n), banned)
        assert R.rth_allowed(banned, np.arange(allowed.size)).tolist() == allowed.tolist()


def _handler(seqs, n_items, tst=None, sub=None):
    from sa_gnn_amd.DataHandler import DataHandler
    U = len(seqs)
    sub = sub or [sp.csr_matrix((U, n_items), dtype=np.int64)]
    return DataHandler.from_memory([sp.csr_matrix((U, n_items)), sub, None], seqs, tst, None)


def test_device_sampler_tables_on_the_host():
    """The table builder on the CPU (device='cpu'): banned rows = seen items + last + test item, sorted and unique;
    subMat rows canonical (a duplicated entry once, an explicit zero dropped); per-user counts."""
    from sa_gnn_amd.model import DeviceSampler
    sub = sp.csr_matrix((np.array([1, 1, 0, 2, 1]), np.array([3, 3, 4, 0, 5]), np.array([0, 3, 3, 5])), shape=(3, 8))
    h = _handler([[1, 2, 1, 5], [7], [6, 0, 2]], 8, [4, None, 2], [sub])
    S = DeviceSampler(h, "cpu", 8, 40, 20)
    ptr, ban = S.ban_ptr.numpy(), S.ban_items.numpy()
    assert [ban[ptr[u]:ptr[u + 1]].tolist() for u in range(3)] == [[1, 2, 4, 5], [7], [0, 2, 6]]
    assert S.samp.tolist() == [3, 0, 2]
    sp_, si = S.sub_ptr.numpy()[0], S.sub_items.numpy()
    assert [si[sp_[u]:sp_[u + 1]].tolist() for u in range(3)] == [[3], [], [0, 5]]
    assert S.npair[0].tolist() == [0, 0, 1]
    assert S.seq_ptr.numpy().tolist() == [0, 4, 5, 8] and S.seq_items.numpy().tolist() == [1, 2, 1, 5, 7, 6, 0, 2]


def test_device_sampler_rejects_bad_datasets():
    from sa_gnn_amd.model import DeviceSampler
    # the handler's trnMat cannot hold such an id, but its sequences are whatever the pickle held
    for bad in (9, -1):
        h = _handler([[1, 2], [3, 4]], 8)
        h.sequence = [[1, 2], [3, bad]]
        with pytest.raises(ValueError, match=f"user 1 holds item {bad}"):
            DeviceSampler(h, "cpu", 8, 40, 20)
    # user 1 has seen 0..3 and its test item is 4: nothing is left to draw a negative from
    with pytest.raises(ValueError, match="user 1 has training pairs"):
        DeviceSampler(_handler([[1, 2], [0, 1, 2, 3]], 5, [None, 4]), "cpu", 5, 40, 20)
    # a user with nothing to draw (one item) may ban everything
    DeviceSampler(_handler([[1, 2], [0]], 5, [None, 4]), "cpu", 5, 40, 20)
