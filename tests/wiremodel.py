"""The three wire formats of `qg_vec_set_state` / `qg_vec_get_state` (include/qgym.h, `qg_state_format`) restated in numpy, for every
env kind.  Written from the header and the Rust lines it cites; shares no code with libqgym or the oracle.

A batch's states are, per kind:
  clifford         uint8 [B, 2n, 2n]   the symplectic matrix (clifford.rs:299-304: row-major, D * D entries)
  linear_function  uint8 [B, n, n]     the matrix (linear_function.rs:279-283)
  pauli            uint8 [B, 2n, 2n]   the tableau, which is all `qg_vec_get_state` returns of a PauliEnv
  permutation      int64 [B, n]        the index vector (permutation.rs:168-173)

and a record -- one env's `stride` elements, of which the first `min_elems` carry the state and the rest are padding -- is:
  i64     matrices: the D * D entries row by row as int64; permutation: the n entries as int64
  u8      matrices: the D * D entries row by row, one 0/1 byte each; permutation: n bytes, one per entry
  packed  matrices: D words, word r = row r, bit c = entry (r, c); a word is uint32 when D <= 32 and uint64 otherwise (PauliEnv: always
          uint64); permutation: n bytes, one per entry
"""
import numpy as np

KINDS = ("clifford", "linear_function", "permutation", "pauli")
FORMATS = ("i64", "u8", "packed")
FORMAT_CODE = {"i64": 0, "u8": 1, "packed": 2}
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
# what an i64 record may hold where the state has a 0 / a 1 (clifford.rs:302: `x > 0`)
I64_ZEROS = (I64_MIN, -1, 0)
I64_ONES = (1, 2, 5, 1 << 32, 1 << 40, I64_MAX)
I64_VALUES = I64_ZEROS + I64_ONES


def dim(kind, n):
    """Rows (= columns) of the kind's matrix; the number of entries of a permutation."""
    assert kind in KINDS, kind
    return 2 * n if kind in ("clifford", "pauli") else n


def word_bytes(kind, n):
    if kind == "permutation":
        return 1
    return 8 if kind == "pauli" or dim(kind, n) > 32 else 4


def elem_dtype(kind, n, fmt):
    assert fmt in FORMATS, fmt
    if fmt == "i64":
        return np.dtype(np.int64)
    if fmt == "u8":
        return np.dtype(np.uint8)
    return np.dtype({1: np.uint8, 4: np.uint32, 8: np.uint64}[word_bytes(kind, n)])


def min_elems(kind, n, fmt):
    """Elements of one record that carry the state: the least stride the library accepts."""
    d = dim(kind, n)
    if kind == "permutation" or fmt == "packed":
        return d
    return d * d


def _fill(fill, dtype):
    return np.array([fill], dtype=np.int64).astype(dtype)[0]  # (wraps: -1 is 0xFF as a byte, all ones as a word)


def encode(kind, n, fmt, states, stride, fill=0):
    """-> [B, stride] array of the format's element type: each env's record, then `stride - min_elems` elements of `fill`."""
    d, dt, m = dim(kind, n), elem_dtype(kind, n, fmt), min_elems(kind, n, fmt)
    states = np.asarray(states)
    B = states.shape[0]
    assert stride >= m, (stride, m)
    if kind == "permutation":
        assert states.shape == (B, d) and ((states >= 0) & (states < max(d, 1))).all()
        body = states.astype(dt)
    else:
        assert states.shape == (B, d, d) and ((states == 0) | (states == 1)).all()
        if fmt == "packed":
            weights = np.left_shift(np.uint64(1), np.arange(d, dtype=np.uint64))
            body = (states.astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64).astype(dt)  # distinct bits: the sum is the OR
        else:
            body = states.reshape(B, d * d).astype(dt)
    out = np.full((B, stride), _fill(fill, dt), dtype=dt)
    out[:, :m] = body
    return out


def decode(kind, n, fmt, records, stride, fill=0):
    """The inverse of `encode`: the states of a [B, stride] (or flat) array of records.  Asserts that the records hold nothing the format
    cannot (entries other than 0 / 1, bits past column D, permutation entries out of range) and that every padding element is `fill`."""
    d, dt, m = dim(kind, n), elem_dtype(kind, n, fmt), min_elems(kind, n, fmt)
    records = np.asarray(records)
    assert records.dtype.itemsize == dt.itemsize, (records.dtype, dt)
    records = records.view(dt).reshape(-1, stride)
    B = records.shape[0]
    pad = records[:, m:]
    bad = np.argwhere(pad != _fill(fill, dt))
    assert bad.size == 0, f"padding overwritten at (env, element) {bad[:4].tolist()}: {pad[tuple(bad[0])]} instead of {_fill(fill, dt)}"
    body = records[:, :m]
    if kind == "permutation":
        states = body.astype(np.int64)
        assert ((states >= 0) & (states < max(d, 1))).all(), "permutation entry out of range"
        return states
    if fmt == "packed":
        words = body.astype(np.uint64)
        if d < 64:
            assert (words >> np.uint64(d) == 0).all(), "bits set past the last column"
        return ((words[:, :, None] >> np.arange(d, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    assert ((body == 0) | (body == 1)).all(), "an entry that is neither 0 nor 1"
    return body.reshape(B, d, d).astype(np.uint8)


def normalise_i64(record):
    """What a CliffordEnv / LinearFunctionEnv makes of an i64 record: `> 0 => 1`, everything else 0 (clifford.rs:299-304,
    linear_function.rs:279-283).  PermutationEnv keeps its entries as they are (permutation.rs:168-173)."""
    return (np.asarray(record, dtype=np.int64) > 0).astype(np.int64)


def spread_i64(records, kind, n, rng):
    """An i64 matrix record with the same meaning and wild values: every 1 of the state becomes a random member of I64_ONES, every 0 a
    random member of I64_ZEROS.  Padding is left alone."""
    assert kind != "permutation"
    m = min_elems(kind, n, "i64")
    out = np.array(records, dtype=np.int64, copy=True)
    body = out[:, :m]
    ones = np.array(I64_ONES, dtype=np.int64)[rng.integers(0, len(I64_ONES), size=body.shape)]
    zeros = np.array(I64_ZEROS, dtype=np.int64)[rng.integers(0, len(I64_ZEROS), size=body.shape)]
    out[:, :m] = np.where(body > 0, ones, zeros)
    return out
