"""The observation converters, the masks and the fault word at the sizes and alignments where their kernels switch paths: chunked, ragged
and per-element `qg_expand_packed`; `qg_widen_dense`'s 16-byte path and its tail; `masks16_kernel`'s last chunk and its fall-back on a
misaligned output; the `B & 3` tail envs of `qg_vec_sync`'s fault scan.  Everything is compared bit for bit with numpy, and every output
sits between sentinel bytes that must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from paulimodel import PauliModel, to_wire  # noqa: E402
from test_paulimodel import random_labels, random_tableau  # noqa: E402
from util import line_gateset  # noqa: E402

SENT = 0xA5
# dtype -> (qg_dtype code, element size, the bit pattern of 1)
DTYPES = {"int8": (0, 1, 1), "float32": (1, 4, 0x3F800000), "bfloat16": (2, 2, 0x3F80), "float16": (3, 2, 0x3C00)}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _lib():
    from qiskit_gym_amd import _lib as lib

    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Out:
    """`count` elements of `es` bytes on the device, every byte a sentinel, with guard bytes on both sides: 16-byte aligned, or
    (`shifted`) starting one element after a 16-byte boundary."""

    def __init__(self, count, es, shifted):
        self.lead = 16 + (es if shifted else 0)
        self.nbytes, self.es = count * es, es
        self.buf = torch.full((self.lead + self.nbytes + 48,), SENT, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lead

    def read(self, what):
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[: self.lead] == SENT).all(), f"written before the output: {what}"
        assert (raw[self.lead + self.nbytes:] == SENT).all(), f"written past the output: {what}"
        return raw[self.lead: self.lead + self.nbytes].copy().view(UINT[self.es])


# ---- qg_expand_packed -----------------------------------------------------------------------------------------------------
ROWS = (1, 2, 15, 16, 17, 257)
WORD_COLS = ((4, 1), (4, 7), (4, 31), (4, 32), (8, 33), (8, 63), (8, 64), (1, 9), (1, 17))


def _dense_of(packed, word, cols):
    if word == 1:  # PermutationEnv rows: the byte is the column that is set (a byte past the last column sets none)
        return packed[:, None] == np.arange(cols, dtype=np.uint8)
    return ((packed[:, None] >> np.arange(cols, dtype=packed.dtype)) & packed.dtype.type(1)).astype(bool)


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "one-element-in"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_expand_packed_shapes_and_alignments(dtype, shifted):
    lib = _lib()
    code, es, one = DTYPES[dtype]
    rng = np.random.default_rng(es + shifted)
    for rows in ROWS:
        for word, cols in WORD_COLS:
            wdt = {1: np.uint8, 4: np.uint32, 8: np.uint64}[word]
            packed = rng.integers(0, 256, size=rows * word, dtype=np.uint8).view(wdt)  # (bits past `cols` are set too: they are no column)
            if word == 1:
                packed[: rows // 2] %= cols
            src = torch.from_numpy(packed.view({1: np.uint8, 4: np.int32, 8: np.int64}[word])).cuda()
            out = _Out(rows * cols, es, shifted)
            lib.check(lib.load().qg_expand_packed(src.data_ptr(), word, rows, cols, out.ptr, code, _stream()))
            what = f"{dtype} rows {rows} word {word} cols {cols}"
            want = np.where(_dense_of(packed, word, cols), one, 0).astype(UINT[es]).reshape(-1)
            np.testing.assert_array_equal(out.read(what), want, err_msg=what)


# ---- qg_widen_dense -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_shifted", [False, True], ids=["out-aligned", "out-one-element-in"])
@pytest.mark.parametrize("in_shifted", [False, True], ids=["in-aligned", "in-one-element-in"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_widen_dense_sizes_and_alignments(dtype, in_shifted, out_shifted):
    lib = _lib()
    code, es, one = DTYPES[dtype]
    rng = np.random.default_rng(es)
    for n in (1, 15, 16, 17, 4101):
        bits = rng.integers(0, 2, size=n).astype(np.uint8)
        bits[-1] = 1  # (the last element is a 1: a dropped tail shows)
        holder = torch.zeros(n + 17, dtype=torch.uint8, device="cuda")
        src = holder[16 + int(in_shifted): 16 + int(in_shifted) + n]
        src.copy_(torch.from_numpy(bits))
        assert src.data_ptr() % 16 == int(in_shifted)
        out = _Out(n, es, out_shifted)
        lib.check(lib.load().qg_widen_dense(src.data_ptr(), n, out.ptr, code, _stream()))
        what = f"{dtype} n {n}"
        np.testing.assert_array_equal(out.read(what), np.where(bits > 0, one, 0).astype(UINT[es]), err_msg=what)


# ---- observe_as on rows of 11 columns -------------------------------------------------------------------------------------
def test_pauli_observe_as_rows_that_are_no_multiple_of_a_chunk():
    from qiskit_gym_amd.vec import VecEnv

    n, B, rot = 4, 65, 3
    gs = line_gateset("pauli", n)
    cfg = dict(add_perms=False, track_solution=False, max_rotations=rot)
    gv = VecEnv("pauli", n, gs, B, **cfg)
    m = PauliModel(n, gs, B, max_rotations=rot, add_perms=False, track_solution=False)
    assert gv.obs_shape_ == (2 * n, 2 * n + rot) == (8, 11)
    rng = np.random.default_rng(11)
    wires = [to_wire(random_tableau(rng, n, int(rng.integers(1, 2 * n))), random_labels(rng, n, int(rng.integers(0, rot + 1)), 4)) for _ in range(B)]
    width = max(len(w) for w in wires)
    gv.set_state(np.array([w + [0] * (width - len(w)) for w in wires], np.int64))
    m.set_state(wires)
    want = m.observe()
    assert want[:, 8:11].any() and want.shape == (B, 88)
    for dtype, (code, es, one) in DTYPES.items():
        got = gv.observe_as(getattr(torch, dtype))
        bits = got.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[es]).cpu().numpy().view(UINT[es])
        np.testing.assert_array_equal(bits, np.where(want > 0, one, 0).astype(UINT[es]), err_msg=dtype)


# ---- qg_vec_masks ---------------------------------------------------------------------------------------------------------
def _clifford_gates(n, count):
    """`count` distinct gates on n qubits (count <= 5 n + 3 n (n - 1))."""
    gates = [(k, (q,)) for q in range(n) for k in ("H", "S", "Sdg", "SX", "SXdg")]
    gates += [(k, (a, b)) for a in range(n) for b in range(n) if a != b for k in ("CX", "CZ", "SWAP")]
    assert count <= len(gates)
    return gates[:count]


@pytest.mark.parametrize("pattern", ["first", "last", "alternating"])
@pytest.mark.parametrize("A,B", [(3, 65), (15, 17), (16, 5), (17, 3), (170, 3)])
def test_masks_chunk_tails_and_misaligned_output(A, B, pattern):
    from qiskit_gym_amd.vec import VecEnv

    lib = _lib()
    n, d = 8, 16
    gv = VecEnv("clifford", n, _clifford_gates(n, A), B, add_inverts=False, add_perms=False, track_solution=False)
    assert gv.num_actions() == A
    solved = np.zeros(B, bool)
    solved[{"first": slice(0, 1), "last": slice(B - 1, B), "alternating": slice(0, B, 2)}[pattern]] = True
    other = np.eye(d, dtype=np.int64)[::-1]  # (any matrix that is not the identity: nothing is stepped)
    gv.set_state(np.where(solved[:, None, None], np.eye(d, dtype=np.int64), other).reshape(B, -1))
    gv.sync()
    np.testing.assert_array_equal(gv.success.cpu().numpy(), solved)
    want = np.repeat(~solved[:, None], A, axis=1).astype(np.uint8)
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), want)
    for shift in (0, 1):  # one byte in: masks16_kernel's 16-byte stores do not apply, the byte kernel runs at every A
        out = _Out(A * B, 1, bool(shift))
        lib.check(gv._L.qg_vec_masks(gv._h, out.ptr, gv._stream()))
        np.testing.assert_array_equal(out.read(f"A {A} B {B} shift {shift}").reshape(B, A), want, err_msg=f"shift {shift}")


# ---- qg_vec_sync / faults -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["last", "first-of-tail"])
@pytest.mark.parametrize("B", [5, 6, 7, 67])
def test_sync_sees_a_fault_in_the_tail_envs(B, where):
    """One env of the batch holds a singular matrix; a step whose coin inverts it sets that env's status word (QG_FAULT_SINGULAR), and
    nothing else.  The env is one of the `B & 3` envs past the last whole group of four, which only workgroup 0's tail lanes read."""
    from qiskit_gym_amd.vec import VecEnv

    lib = _lib()
    n, d = 4, 8
    gs = line_gateset("clifford", n)
    gv = VecEnv("clifford", n, gs, B, add_inverts=True, add_perms=False, track_solution=False)
    env = B - 1 if where == "last" else B - (B & 3)
    assert B & 3 and B - (B & 3) <= env < B
    states = np.broadcast_to(np.eye(d, dtype=np.int64), (B, d, d)).copy()
    states[env, d - 1] = states[env, 0]  # two equal rows
    gv.set_state(states.reshape(B, -1))
    gv.sync()  # nothing has been inverted yet
    assert not gv.faults().any()
    gv.step(torch.zeros(B, dtype=torch.int32, device="cuda"), torch.ones(B, dtype=torch.uint8, device="cuda"))  # coin 1: every env inverts
    with pytest.raises(lib.QGymError, match=f"env {env}: singular"):
        gv.sync()
    faults = gv.faults()
    assert faults[env] == 1 and not np.delete(faults, env).any()
