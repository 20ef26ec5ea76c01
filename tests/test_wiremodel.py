"""tests/wiremodel.py pinned on the CPU: its i64 reading (`> 0 => 1`, clifford.rs:299-304) against the CPU oracle at the values where a
narrowing compare goes wrong, its packed words against bits spelled out one by one, and encode / decode as inverses on every format
and stride the GPU tests use."""
import numpy as np
import pytest

import wiremodel as wm
from oracle import OracleEnv
from util import line_gateset

STRIDES = (0, 1, 7)  # elements past the minimum


def _states(kind, n, B, rng):
    d = wm.dim(kind, n)
    if kind == "permutation":
        return np.stack([rng.permutation(d) for _ in range(B)]).astype(np.int64)
    return rng.integers(0, 2, size=(B, d, d)).astype(np.uint8)


@pytest.mark.parametrize("kind,n", [("clifford", 3), ("linear_function", 5), ("linear_function", 9)])
def test_oracle_reads_an_i64_record_as_the_model_normalises_it(kind, n):
    rng = np.random.default_rng(n)
    env = OracleEnv(kind, n, line_gateset(kind, n), add_inverts=0, add_perms=0, track_solution=0)
    size = wm.min_elems(kind, n, "i64")
    values = np.array(wm.I64_VALUES, dtype=np.int64)
    records = [values[rng.integers(0, len(values), size=size)] for _ in range(40)]
    records += [np.full(size, v, np.int64) for v in values]  # every value alone, in every position
    for rec in records:
        env.set_state(rec)
        np.testing.assert_array_equal(env.get_state(), wm.normalise_i64(rec))
    # ... and the spread of a state over those values means the state
    states = _states(kind, n, 8, rng)
    plain = wm.encode(kind, n, "i64", states, size)
    wild = wm.spread_i64(plain, kind, n, rng)
    assert set(np.unique(wild).tolist()) <= set(wm.I64_VALUES) and len(np.unique(wild)) > 4
    np.testing.assert_array_equal(wm.normalise_i64(wild), plain)
    for b in range(len(states)):
        env.set_state(wild[b])
        np.testing.assert_array_equal(env.get_state(), plain[b])


@pytest.mark.parametrize("n", [5, 9, 17])
def test_oracle_keeps_a_permutation_record_as_it_is(n):
    rng = np.random.default_rng(n)
    env = OracleEnv("permutation", n, line_gateset("permutation", n), add_inverts=0, add_perms=0, track_solution=0)
    states = _states("permutation", n, 20, rng)
    rec = wm.encode("permutation", n, "i64", states, n)
    for b in range(len(states)):
        env.set_state(rec[b])
        np.testing.assert_array_equal(env.get_state(), states[b])


CONFIGS = [("clifford", 3), ("clifford", 16), ("clifford", 17), ("linear_function", 5), ("linear_function", 9), ("linear_function", 33),
           ("linear_function", 64), ("permutation", 9), ("permutation", 17), ("pauli", 4)]


@pytest.mark.parametrize("fmt", wm.FORMATS)
@pytest.mark.parametrize("kind,n", CONFIGS)
def test_decode_inverts_encode(kind, n, fmt):
    rng = np.random.default_rng(n + len(fmt))
    B = 5
    states = _states(kind, n, B, rng)
    m = wm.min_elems(kind, n, fmt)
    for extra in STRIDES:
        for fill in (0, -1, 1, 0x7F):
            rec = wm.encode(kind, n, fmt, states, m + extra, fill)
            assert rec.shape == (B, m + extra) and rec.dtype == wm.elem_dtype(kind, n, fmt)
            np.testing.assert_array_equal(wm.decode(kind, n, fmt, rec, m + extra, fill), states)
            np.testing.assert_array_equal(wm.decode(kind, n, fmt, rec.reshape(-1), m + extra, fill), states)  # flat, as the library sees it
            np.testing.assert_array_equal(wm.encode(kind, n, fmt, wm.decode(kind, n, fmt, rec, m + extra, fill), m + extra, fill), rec)
            if extra and fill != 1:
                with pytest.raises(AssertionError, match="padding"):
                    wm.decode(kind, n, fmt, rec, m + extra, 1)


def test_element_types_and_sizes_are_the_headers():
    assert wm.word_bytes("clifford", 16) == 4 and wm.word_bytes("clifford", 17) == 8
    assert wm.word_bytes("linear_function", 32) == 4 and wm.word_bytes("linear_function", 33) == 8
    assert wm.word_bytes("permutation", 200) == 1 and wm.word_bytes("pauli", 4) == 8
    assert wm.min_elems("clifford", 3, "i64") == 36 and wm.min_elems("clifford", 3, "u8") == 36 and wm.min_elems("clifford", 3, "packed") == 6
    assert [wm.min_elems("permutation", 9, f) for f in wm.FORMATS] == [9, 9, 9]
    assert wm.min_elems("pauli", 4, "i64") == 64 and wm.min_elems("pauli", 4, "packed") == 8


@pytest.mark.parametrize("kind,n", [("clifford", 3), ("linear_function", 33), ("linear_function", 64), ("pauli", 4)])
def test_packed_words_bit_by_bit(kind, n):
    rng = np.random.default_rng(n)
    states = _states(kind, n, 3, rng)
    d = wm.dim(kind, n)
    rec = wm.encode(kind, n, "packed", states, d + 1, -1)
    for b in range(3):
        for r in range(d):
            assert int(rec[b, r]) == sum(int(states[b, r, c]) << c for c in range(d))
        assert int(rec[b, d]) == (1 << (8 * rec.dtype.itemsize)) - 1
    with pytest.raises(AssertionError):
        bad = rec.copy()
        if d < 64:
            bad[0, 0] |= rec.dtype.type(1) << rec.dtype.type(d)
        else:
            bad[0, d] = 0
        wm.decode(kind, n, "packed", bad, d + 1, -1)


def test_permutation_bytes_are_the_entries():
    states = np.array([[2, 0, 1, 4, 3]], np.int64)
    for fmt in ("u8", "packed"):
        assert wm.encode("permutation", 5, fmt, states, 6, 0x7F).tolist() == [[2, 0, 1, 4, 3, 0x7F]]
    assert wm.encode("permutation", 5, "i64", states, 6, -1).tolist() == [[2, 0, 1, 4, 3, -1]]
