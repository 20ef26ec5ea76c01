"""The numpy restatement of `qg_az_pack` (tests/azmodel.py) on logs whose answers are written out here, its properties on random logs, and
the C boundary: both new symbols are declared in include/qgym.h and bound in `_lib`.  No GPU."""
import os
import re

import numpy as np

from azmodel import F32, pack, returns_to_go
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_log(rng, T, E, A, monotone=True, p_zero=0.1, p_bad=0.0):
    """A log like a self-play's: every episode live for its first decisions (or, `monotone` False, at random), counts of a few visits, some
    rows of zeros and some bad ones, rewards of any sign."""
    counts = rng.integers(0, 9, size=(T, E, A)).astype(np.int32)
    if monotone:
        live = (np.arange(T)[:, None] < rng.integers(0, T + 1, size=E)[None, :]).astype(np.uint8)
    else:
        live = (rng.random((T, E)) < 0.6).astype(np.uint8)
    counts[rng.random((T, E)) < p_zero] = 0
    for t, e in zip(*np.nonzero(rng.random((T, E)) < p_bad)):
        if rng.random() < 0.5:
            counts[t, e, rng.integers(A)] = -int(rng.integers(1, 5))
        else:
            counts[t, e, rng.integers(A)] = (1 << 24) - int(rng.integers(0, 2))  # 2^24 itself, or one below it beside other visits
    reward = rng.standard_normal((T, E)).astype(np.float32)
    move = rng.integers(0, A + 1, size=(T, E)).astype(np.int32)
    return counts, reward, live, move


def test_three_decisions_two_episodes_one_ending_early():
    counts = np.array([[[1, 2, 1], [0, 3, 1]], [[2, 2, 0], [4, 0, 0]], [[1, 0, 3], [5, 5, 5]]], dtype=np.int32)
    reward = np.array([[-0.5, 0.25], [-0.25, 1.0], [1.5, 7.0]], dtype=np.float32)
    live = np.array([[1, 1], [1, 1], [1, 0]], dtype=np.uint8)  # episode 1 ends after decision 1: its row of decision 2 is dead
    move = np.array([[1, 1], [0, 0], [2, 9]], dtype=np.int32)
    words = np.arange(3 * 2 * 2, dtype=np.int64).reshape(3, 2, 2)
    p = pack(counts, reward, live, move, words)
    assert p.n.tolist() == [5, 5, 0]
    assert p.index.tolist() == [0, 1, 2, 3, 4]
    assert p.z.tolist() == [0.75, 1.25, 1.25, 1.0, 1.5]  # e0: 1.5, -0.25 + 1.5, -0.5 + 1.25; e1: 1.0, 0.25 + 1.0 -- the 7.0 is never added
    assert p.move.tolist() == [1, 1, 0, 0, 2]
    assert p.pi.tolist() == [[0.25, 0.5, 0.25], [0.0, 0.75, 0.25], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0], [0.25, 0.0, 0.75]]
    assert p.words.tolist() == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    assert p.pi.dtype == np.float32 and p.z.dtype == np.float32 and p.index.dtype == np.int32 and p.move.dtype == np.int32


def test_a_zero_row_and_a_bad_row_give_no_sample_but_their_rewards_count():
    counts = np.array([[[0, 0], [-1, 5]], [[3, 1], [1, 1]]], dtype=np.int32)
    reward = np.array([[0.5, 2.0], [1.0, -1.0]], dtype=np.float32)
    live = np.ones((2, 2), dtype=np.uint8)
    move = np.array([[0, 1], [1, 0]], dtype=np.int32)
    p = pack(counts, reward, live, move)
    assert p.n.tolist() == [2, 2, 1]
    assert p.index.tolist() == [2, 3] and p.move.tolist() == [1, 0]
    assert p.z.tolist() == [1.0, -1.0] and p.pi.tolist() == [[0.75, 0.25], [0.5, 0.5]]
    assert returns_to_go(reward, live).tolist() == [[1.5, 1.0], [1.0, -1.0]]
    # a third of a visit count is no binary fraction: the one division, rounded once
    q = pack(np.array([[[1, 2]]], dtype=np.int32), np.zeros((1, 1), np.float32), np.ones((1, 1), np.uint8), np.zeros((1, 1), np.int32))
    assert bits(q.pi).tolist() == [[0x3EAAAAAB, 0x3F2AAAAB]]


def test_total_at_the_f32_limit_is_bad_and_one_below_is_not():
    live, move, reward = np.ones((1, 2), np.uint8), np.zeros((1, 2), np.int32), np.zeros((1, 2), np.float32)
    counts = np.array([[[(1 << 24) - 1, 0], [(1 << 24) - 1, 1]]], dtype=np.int32)
    p = pack(counts, reward, live, move)
    assert p.n.tolist() == [1, 1, 1] and p.index.tolist() == [0] and p.pi.tolist() == [[1.0, 0.0]]
    counts = np.array([[[np.iinfo(np.int32).max] * 2] * 2], dtype=np.int32)  # a total past 2^32: Python integers do not wrap
    assert pack(counts, reward, live, move).n.tolist() == [0, 0, 2]


def test_an_all_dead_log_gives_nothing():
    rng = np.random.default_rng(0)
    counts, reward, live, move = random_log(rng, 4, 5, 3, p_bad=0.3)
    p = pack(counts, reward, np.zeros_like(live), move)
    assert p.n.tolist() == [0, 0, 0] and len(p.index) == 0 and p.pi.shape == (0, 3)


def test_properties_on_random_logs():
    rng = np.random.default_rng(1)
    seen_zero = seen_bad = seen_early = 0
    for trial in range(40):
        T, E, A = int(rng.integers(1, 9)), int(rng.integers(1, 12)), int(rng.integers(1, 8))
        counts, reward, live, move = random_log(rng, T, E, A, monotone=trial % 2 == 0, p_zero=0.15, p_bad=0.1 if trial % 4 < 2 else 0.0)
        p = pack(counts, reward, live, move)
        total = counts.astype(np.int64).sum(axis=2)
        bad = ((counts < 0).any(axis=2) | (total >= 1 << 24)) & (live != 0)
        valid = (live != 0) & ~bad & (total > 0)
        assert p.n.tolist() == [int(valid.sum()), int(valid.sum()), int(bad.sum())]
        assert (np.diff(p.index) > 0).all()  # strictly ascending
        np.testing.assert_array_equal(p.index, np.nonzero(valid.reshape(-1))[0])
        np.testing.assert_array_equal(p.move, move.reshape(-1)[p.index])
        s = p.pi.astype(np.float64).sum(axis=1)
        assert (np.abs(s - 1.0) <= A * 2.0 ** -23).all() and (p.pi >= 0).all()
        G = returns_to_go(reward, live)
        np.testing.assert_array_equal(bits(p.z), bits(G.reshape(-1)[p.index]))
        for e in range(E):
            ts = np.nonzero(live[:, e])[0]
            if len(ts) == 0:
                continue
            last = ts[-1]
            assert bits(G[last, e]) == bits(reward[last, e])  # the last live decision's return is its reward, bit for bit
            if valid[last, e]:
                assert bits(p.z[list(p.index).index(last * E + e)]) == bits(reward[last, e])
            # a live row without a sample (zero counts, bad) still hands its reward to the decisions before it
            for i, t in enumerate(ts[:-1]):
                nxt = ts[i + 1]
                assert bits(G[t, e]) == bits(F32(reward[t, e] + G[nxt, e]))
                if not valid[nxt, e] and valid[t, e]:
                    seen_zero += int(total[nxt, e] == 0)
                    seen_bad += int(bad[nxt, e])
            seen_early += int(last < T - 1)
        n_valid = int(valid.sum())
        for cap in {1, max(1, n_valid - 1), max(1, n_valid), T * E}:  # capacity below, at and above the valid decisions
            q = pack(counts, reward, live, move, capacity=cap)
            k = min(cap, n_valid)
            assert q.n.tolist() == [k, n_valid, int(bad.sum())]
            np.testing.assert_array_equal(q.index, p.index[:k])
            np.testing.assert_array_equal(bits(q.z), bits(p.z[:k]))
            np.testing.assert_array_equal(bits(q.pi), bits(p.pi[:k]))
    assert seen_zero > 0 and seen_bad > 0 and seen_early > 0  # the trials met what they are about


def test_both_symbols_are_declared_and_bound():
    import ctypes as C

    from qiskit_gym_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qgym.h")).read()
    assert re.search(r"^size_t qg_az_pack_scratch_bytes\(uint64_t T, uint64_t E\);", hdr, re.M)
    assert re.search(r"^int qg_az_pack\(const int32_t \*counts_dev,", hdr, re.M)
    L = _lib.load()
    for name in ("qg_az_pack", "qg_az_pack_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert len(L.qg_az_pack.argtypes) == 21 and L.qg_az_pack_scratch_bytes.restype is C.c_size_t
    # host-only: the scratch is 8 bytes per item and 8 per chunk of 256 items, 0 beyond the limits
    assert L.qg_az_pack_scratch_bytes(1, 1) == 16 and L.qg_az_pack_scratch_bytes(2, 128) == 2056 and L.qg_az_pack_scratch_bytes(257, 1) == 257 * 8 + 16
    assert L.qg_az_pack_scratch_bytes(0, 5) == 0 and L.qg_az_pack_scratch_bytes(1 << 16, 1 << 15) == 0 and L.qg_az_pack_scratch_bytes(1 << 40, 1 << 40) == 0
    # the argument checks come before any launch: they answer without a GPU
    assert L.qg_az_pack(None, 4, None, None, None, None, 0, 0, 1, 1, 4, 1, None, None, None, None, None, 4, None, None, None) == -1
    assert b"null argument" in L.qg_last_error()
